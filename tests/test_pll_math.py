"""pll_sinf / pll_cosf (sdrangel_amd/csrc/pll_math.hpp, the cos / sin of PhaseLockComplex::feed and FreqLockComplex::feed on the
host and the device) against the host's sinf, cosf and sincosf: tests/pll_math_check.cpp.  3 * 10^7 inputs per seed in three
random sets (|x| < 7, where the PLL stays; |x| < 3 * 10^6 and exponents 2^6 .. 2^125, where the FLL's unwrapped phase goes) and
the specials.  The routine is glibc's from 2.28 on in the build a CPU with FMA is given: on such a host every result is the
libm's very bits; elsewhere (another libm, or the unfused build) results are at most 1 ulp away."""
import os
import platform
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sdrangel_amd", "csrc")


@pytest.fixture(scope="module")
def check():
    exe = os.path.join(tempfile.mkdtemp(), "pll_math_check")
    # plain g++, no ROCm include path: the header compiles for the host on its own; no builtin may stand in for the libm
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-builtin", "-Wall", "-Werror", "-I" + CSRC,
                           os.path.join(ROOT, "tests", "pll_math_check.cpp"), "-o", exe, "-lm"])
    return exe


def _exact_expected() -> bool:
    """an x86-64 glibc (2.28 .. 2.40) host whose CPU has FMA: the ifunc picks the fused build this routine restates"""
    name, ver = platform.libc_ver()
    if name != "glibc" or platform.machine() not in ("x86_64", "AMD64"):
        return False
    v = tuple(int(p) for p in ver.split(".")[:2])
    if not ((2, 28) <= v <= (2, 40)):
        return False
    try:
        flags = next(l for l in open("/proc/cpuinfo") if l.startswith("flags")).split()
    except (OSError, StopIteration):
        return False
    return "fma" in flags and "avx2" in flags


def _run(check, name, seed, n):
    out = subprocess.run([check, name, str(seed), str(n)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout + out.stderr
    count, differ, worst = (int(v) for v in out.stdout.split()[1:4])
    exact = _exact_expected()
    print(f"{name} seed {seed}: {count} inputs, {differ} differ, worst {worst} ulp; rule: {'the very bits' if exact else 'at most 1 ulp'} "
          f"({platform.libc_ver()}, {platform.machine()})")
    if exact:
        assert differ == 0 and worst == 0, out.stdout
    else:
        assert worst <= 1, out.stdout
    return count


@pytest.mark.parametrize("seed", [1, 20261020])
@pytest.mark.parametrize("name", ["small", "mid", "exp"])
def test_sinf_cosf_equal_the_host_libm(check, name, seed):
    assert _run(check, name, seed, 10_000_000) == 10_000_000


def test_specials(check):
    """+-0, subnormals, +-inf, NaN, the three thresholds of the routine and every exponent at three mantissas"""
    assert _run(check, "special", 0, 0) > 1500
