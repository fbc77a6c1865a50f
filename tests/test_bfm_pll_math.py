"""CPU: the host build of the stereo pilot loop's step (sdrangel_amd/csrc/bfm_pll.hpp, what bfm_walk_kernel runs) against a plain
C++ transcription of PhaseLock::process that calls the host libm's sinf / cosf: tests/bfm_pll_check.cpp, a stand-alone program.
The loop feeds back what sinf / cosf return, so the comparison means something only where pll_sinf / pll_cosf are the host libm's
very routines: an x86-64 glibc 2.28 .. 2.40 on a CPU with FMA (tests/test_pll_math.py checks that equality by itself).  Elsewhere
the test skips and says so."""
import os
import subprocess
import tempfile

import pytest

from tests.test_pll_math import _exact_expected

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sdrangel_amd", "csrc")


@pytest.fixture(scope="module")
def check():
    if not _exact_expected():
        pytest.skip("the host libm is not the fused glibc 2.28 .. 2.40 build whose sinf / cosf the step restates")
    exe = os.path.join(tempfile.mkdtemp(), "bfm_pll_check")
    # plain g++, no ROCm include path: the header compiles for the host on its own; no builtin may stand in for the libm
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-builtin", "-Wall", "-Werror", "-I" + CSRC,
                           os.path.join(ROOT, "tests", "bfm_pll_check.cpp"), "-o", exe, "-lm"])
    return exe


def _run(check, name, seed, n, rate):
    out = subprocess.run([check, name, str(seed), str(n), str(rate)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout + out.stderr
    v = [int(x) for x in out.stdout.split()[1:]]
    probe = dict(zip(("ratio", "plus", "minus", "clamp_lo", "clamp_hi", "wrap", "lock_up", "lock_reset"), v[2:]))
    print(f"{name} seed {seed} at {rate}: {v[0]} steps, {v[1]} differ, {probe}")
    assert v[0] == n and v[1] == 0, out.stdout
    return probe


@pytest.mark.parametrize("rate", [96000, 240000, 384000])
@pytest.mark.parametrize("name,seed", [("tone", 1), ("tone", 20261020), ("noise", 2)])
def test_step_equals_the_transcription(check, name, seed, rate):
    probe = _run(check, name, seed, 400_000, rate)
    assert probe["wrap"] > 0 and probe["minus"] > 0 and probe["plus"] > 0 and probe["ratio"] > 0, probe


def test_specials(check):
    """+-0, subnormals, the largest floats and +-1 in between stretches of a clean pilot, with m_lock_delay cut to 40"""
    probe = _run(check, "special", 0, 20_000, 240000)
    assert probe["lock_up"] > 0 and probe["lock_reset"] > 0, probe
