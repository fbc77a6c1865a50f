"""The block schedule of the UDPSrc bank's SSB formats (sdrangel_amd/csrc/udpsrc_ssb_sched.hpp: which resampled sample completes
which block, where a block and format 4's raw elements land in the payload, what is carried) on the host against a literal
sample-by-sample loop: tests/udpsrc_ssb_scan_check.cpp, every pending count against the edge lengths and random walks of feeds.
The stand-alone program is built twice, plainly and with -fsanitize=address,undefined, and both are run directly."""
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sdrangel_amd", "csrc")


def _build(extra):
    exe = os.path.join(tempfile.mkdtemp(), "udpsrc_ssb_scan_check")
    # plain g++, no ROCm include path: the header compiles for the host on its own
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-I" + CSRC] + extra +
                          [os.path.join(ROOT, "tests", "udpsrc_ssb_scan_check.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def check():
    return _build([])


@pytest.fixture(scope="module")
def check_sanitized():
    return _build(["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])


@pytest.mark.parametrize("seed", [1, 2, 20261020])
def test_schedule_equals_the_literal_loop(check, seed):
    out = subprocess.run([check, str(seed), "400"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout + out.stderr
    assert int(out.stdout.split()[1]) > 1000000


def test_schedule_under_address_and_undefined_behaviour_sanitizers(check_sanitized):
    out = subprocess.run([check_sanitized, "7", "150"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.startswith("ok ") and not out.stderr, out.stdout + out.stderr
