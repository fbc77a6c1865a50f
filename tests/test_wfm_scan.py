"""The scan operators of the WFM demodulator (sdrangel_amd/csrc/wfm_scan.hpp: squelch counter as composed clamp maps,
m_prevArg as a last-open index scan) on the host, against the serial loop: tests/wfm_scan_check.cpp."""
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sdrangel_amd", "csrc")


@pytest.fixture(scope="module")
def check():
    exe = os.path.join(tempfile.mkdtemp(), "wfm_scan_check")
    # plain g++, no ROCm include path: the header compiles for the host on its own
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-I" + CSRC,
                           os.path.join(ROOT, "tests", "wfm_scan_check.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("seed", [1, 2, 3, 20261017])
def test_scans_equal_the_serial_loop(check, seed):
    out = subprocess.run([check, str(seed), "300"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout + out.stderr
    assert int(out.stdout.split()[1]) > 500000
