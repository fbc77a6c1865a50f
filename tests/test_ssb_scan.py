"""The cut of the SSB demodulator's recurrences (sdrangel_amd/csrc/ssb_scan.hpp: the gate counter, m_count and the step pair as
three scans of composed maps, the factor and the step value from the pair before and after a step, the spectrum-group index
arithmetic, the delay-line index with the clamped readBack) on the host, against the serial loop with the reference's ifs and a
DoubleBufferFIFO-shaped array: tests/ssb_scan_check.cpp.  Rounds cycle hn through 2, 16 and 6144 and the gate through 0, small,
around hn and up to 300; chunk boundaries fall at every offset."""
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sdrangel_amd", "csrc")


@pytest.fixture(scope="module")
def check():
    exe = os.path.join(tempfile.mkdtemp(), "ssb_scan_check")
    # plain g++, no ROCm include path: the header compiles for the host on its own
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-I" + CSRC,
                           os.path.join(ROOT, "tests", "ssb_scan_check.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("seed", [1, 2, 20261017])
def test_cut_equals_the_serial_loop(check, seed):
    out = subprocess.run([check, str(seed), "36"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout + out.stderr
    assert int(out.stdout.split()[1]) > 2000000
