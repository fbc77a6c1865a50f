"""The cut of the NFM demodulator's recurrences (sdrangel_amd/csrc/nfm_scan.hpp: discriminator from neighbouring arguments,
moving-average terms, the counter as composed clamp maps with cap 2 * gate, the delay-line stream with the clamped readBack,
the Bandpass over the compacted sequence, the history indexing across feeds) on the host, against the serial loop with the
reference's containers: tests/nfm_scan_check.cpp."""
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sdrangel_amd", "csrc")


@pytest.fixture(scope="module")
def check():
    exe = os.path.join(tempfile.mkdtemp(), "nfm_scan_check")
    # plain g++, no ROCm include path: the header compiles for the host on its own
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-I" + CSRC,
                           os.path.join(ROOT, "tests", "nfm_scan_check.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("seed", [1, 2, 20261017])
def test_cut_equals_the_serial_loop(check, seed):
    out = subprocess.run([check, str(seed), "44"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout + out.stderr
    assert int(out.stdout.split()[1]) > 200000
