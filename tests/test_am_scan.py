"""The cut of the AM demodulator's recurrences (sdrangel_amd/csrc/am_scan.hpp: moving-average and AGC terms, the gate's
compaction, the history indexing across feeds with the AGC's 0.003f prefix, the Bandpass over the compacted sequence) on the
host, against the serial loop with the reference's containers: tests/am_scan_check.cpp."""
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sdrangel_amd", "csrc")


@pytest.fixture(scope="module")
def check():
    exe = os.path.join(tempfile.mkdtemp(), "am_scan_check")
    # plain g++, no ROCm include path: the header compiles for the host on its own
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-I" + CSRC,
                           os.path.join(ROOT, "tests", "am_scan_check.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("seed", [1, 2, 3, 20261017])
def test_cut_equals_the_serial_loop(check, seed):
    out = subprocess.run([check, str(seed), "120"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout + out.stderr
    assert int(out.stdout.split()[1]) > 200000
