"""The squelch of UDPSrc as maps on one chain of positions (sdrangel_amd/csrc/udpsrc_scan.hpp: UdpSq, closed under composition)
on the host, against the literal calculateSquelch with its flag and two counters: tests/udpsrc_scan_check.cpp.  Exhaustive over
G, R in 0..6, every start state and every boolean string up to length 12 (folded from the left, from the right and as a balanced
tree), then random long strings at G, R up to 5000 in the kernel's grouping, cut into feeds."""
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sdrangel_amd", "csrc")


@pytest.fixture(scope="module")
def check():
    exe = os.path.join(tempfile.mkdtemp(), "udpsrc_scan_check")
    # plain g++, no ROCm include path: the header compiles for the host on its own
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-I" + CSRC,
                           os.path.join(ROOT, "tests", "udpsrc_scan_check.cpp"), "-o", exe])
    return exe


def test_composed_maps_equal_the_literal_automaton_exhaustively(check):
    out = subprocess.run([check, "exhaustive"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout + out.stderr
    # 49 (G, R) pairs, 8191 strings each, at least two start states
    assert int(out.stdout.split()[1]) > 49 * 8191 * 2


@pytest.mark.parametrize("seed", [1, 2, 20261018])
def test_block_scan_with_a_carried_state_equals_the_literal_automaton(check, seed):
    out = subprocess.run([check, "random", str(seed), "60"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout + out.stderr
    assert int(out.stdout.split()[1]) > 200000


@pytest.mark.parametrize("seed", [1, 20261018])
def test_agc_counter_scans_with_independent_gate_delay_and_step(check, seed):
    """MagAGC as UDPSrc sets it up: ssb_scan.hpp's maps with the step-down delay and the step length as parameters of their own"""
    out = subprocess.run([check, "agc", str(seed), "300"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout + out.stderr
    assert int(out.stdout.split()[1]) > 100000


@pytest.mark.parametrize("seed", [1, 20261019])
def test_arg_of_the_discriminator_is_the_host_libm_atan2f(check, seed):
    """udp_atan2f (formats 2 and 3) restates the fdlibm float routines that glibc's atan2f was up to 2.40: never more than 2 ulp
    from the host's atan2f, which is also what tests/udpsrc_oracle.c calls, and its very bits where the libm is such a glibc
    (checked against 2.35)"""
    import platform
    out = subprocess.run([check, "arg", str(seed), "30000000"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout + out.stderr
    n, differ, worst = (int(v) for v in out.stdout.split()[1:4])
    print(platform.libc_ver(), n, differ, worst)
    assert n == 30000000 and worst <= 2, out.stdout
    name, ver = platform.libc_ver()
    if name == "glibc" and tuple(int(v) for v in ver.split(".")[:2]) <= (2, 35):
        assert differ == 0, out.stdout
