"""The arena carver of the demodulator banks (sdrangel_amd/csrc/demod_carve.hpp: one layout description sizes an allocation
in counting mode and hands out its pointers in placing mode, and lists the ranges that carry state) on the host:
tests/demod_carve_check.cpp."""
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sdrangel_amd", "csrc")

# 8 counts x 3 element sizes, at two bases, plus the two history pairs, plus two kept arrays at two capacities and their two moves
CHECKED = 2 * 24 + 2 + 2 * 2 + 2


def build(*flags):
    exe = os.path.join(tempfile.mkdtemp(), "demod_carve_check")
    # plain g++, no ROCm include path: the header compiles for the host on its own
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", *flags, "-I" + CSRC,
                           os.path.join(ROOT, "tests", "demod_carve_check.cpp"), "-o", exe])
    return exe


def run(exe):
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout + out.stderr
    assert int(out.stdout.split()[1]) == CHECKED


def test_placing_ends_where_counting_said():
    run(build())


def test_the_same_check_under_the_address_and_undefined_behaviour_sanitizers():
    """a stand-alone program with its own main: every byte the check writes or moves is inside its arenas"""
    run(build("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
