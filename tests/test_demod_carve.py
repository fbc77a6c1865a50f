"""The arena carver of the demodulator banks (sdrangel_amd/csrc/demod_carve.hpp: one layout description sizes an allocation
in counting mode and hands out its pointers in placing mode) on the host: tests/demod_carve_check.cpp."""
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sdrangel_amd", "csrc")


@pytest.fixture(scope="module")
def check():
    exe = os.path.join(tempfile.mkdtemp(), "demod_carve_check")
    # plain g++, no ROCm include path: the header compiles for the host on its own
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I" + CSRC,
                           os.path.join(ROOT, "tests", "demod_carve_check.cpp"), "-o", exe])
    return exe


def test_placing_ends_where_counting_said(check):
    out = subprocess.run([check], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout + out.stderr
    # 8 counts x 3 element sizes, at two bases, plus the two history pairs
    assert int(out.stdout.split()[1]) == 2 * 24 + 2
