"""The cut of the NFM demodulator's CTCSS branch (sdrangel_amd/csrc/nfm_tone_scan.hpp: the Lowpass at the detector's samples,
detector blocks cut by the carried fill, Goertzel per block and tone, evaluatePower, m_ctcssIndex as a last-writer scan, the
history indexing across feeds) on the host, against the serial loop with the reference's containers:
tests/nfm_tone_scan_check.cpp.  Built with plain g++, and once more with the address and undefined-behaviour sanitizers; the
stand-alone program alone runs under them."""
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sdrangel_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "nfm_tone_scan_check.cpp")


def _build(name, extra):
    exe = os.path.join(tempfile.mkdtemp(), name)
    # plain g++, no ROCm include path: the header compiles for the host on its own
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-I" + CSRC] + extra + [SRC, "-o", exe])
    return exe


@pytest.fixture(scope="module")
def check():
    return _build("nfm_tone_scan_check", ["-O2"])


@pytest.mark.parametrize("seed", [1, 2, 20261020])
def test_cut_equals_the_serial_loop(check, seed):
    out = subprocess.run([check, str(seed), "44"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout + out.stderr
    checked, blocks, changes = (int(v) for v in out.stdout.split()[1:4])
    assert checked > 200000 and blocks > 2000 and changes > 100, out.stdout


def test_cut_is_clean_under_the_host_sanitizers():
    exe = _build("nfm_tone_scan_check_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    out = subprocess.run([exe, "3", "12"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout + out.stderr
