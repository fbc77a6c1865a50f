"""CPU: tests/atv_check.cpp, a stand-alone program over sdrangel_amd/csrc/atv_scan.hpp -- the design integers, the discriminators
and the per-sample step that the device runs -- compiled with plain g++, once as it is and once with
-fsanitize=address,undefined, and run on every case of tests/atv_cases.py.  What it writes equals the oracle's output
(tests/atv_oracle.cpp, which shares none of that code) for every feed: design, events, stored frames, screen, scope and state."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

from tests import atv_cases as ac

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "atv_check.cpp")


def build(extra) -> str:
    exe = os.path.join(tempfile.mkdtemp(), "atv_check")
    if not os.path.exists(os.path.join(ac.ORACLE_DIR, "libsdro.so")):
        subprocess.check_call(["make", "-C", ac.ORACLE_DIR, "libsdro.so"])
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-I" + ac.CSRC] + extra + [SRC, "-o", exe,
                           "-L" + ac.ORACLE_DIR, "-lsdro", "-Wl,-rpath," + ac.ORACLE_DIR, "-lm"])
    return exe


@pytest.fixture(scope="module")
def oracle():
    return ac.build_oracle()


def run_check(exe: str, case: dict) -> dict:
    d = tempfile.mkdtemp()
    fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
    x, splits = ac.inputs(case), case["splits"]
    with open(fin, "wb") as f:
        f.write(bytes(ac.as_struct(case["cfg"])))
        f.write(np.array([len(splits)] + list(splits), np.int64).tobytes())
        f.write(x.tobytes())
    env = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1", ASAN_OPTIONS="detect_leaks=1")
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "ERROR" not in r.stderr, (case["name"], r.returncode, r.stderr[-2000:])
    raw = open(fout, "rb").read()
    pos = 0

    def take(dtype, n):
        nonlocal pos
        a = np.frombuffer(raw, dtype, n, pos).copy()
        pos += a.nbytes
        return a

    design = take(np.int32, 12).tolist()
    rows, cols = design[10], design[9]
    feeds = []
    for _ in splits:
        ne = int(take(np.int64, 1)[0]); events = take(np.int32, ne)
        ns = int(take(np.int64, 1)[0]); frames = [take(np.uint8, rows * cols).reshape(rows, cols) for _ in range(ns)]
        screen = take(np.uint8, rows * cols).reshape(rows, cols)
        nsc = int(take(np.int64, 1)[0]); scope = take(np.int16, nsc)
        st = take(np.uint32, 28)
        state = st[:10].view(np.int32).tolist() + st[10:].tolist()
        feeds.append({"events": events, "frames": frames, "screen": screen, "scope": scope, "state": state})
    assert pos == len(raw)
    return {"design": design, "feeds": feeds}


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-omit-frame-pointer"]], ids=["plain", "asan_ubsan"])
def test_the_scan_header_equals_the_oracle_on_every_case(oracle, flags):
    exe = build(flags)
    for case in ac.CASES:
        got, want = run_check(exe, case), ac.run_oracle(oracle, case)
        assert got["design"] == want["design"], case["name"]
        for i, (g, w) in enumerate(zip(got["feeds"], want["feeds"])):
            what = (case["name"], "feed", i)
            assert np.array_equal(g["events"], w["events"]), what
            assert len(g["frames"]) == len(w["frames"]) and all(np.array_equal(a, b) for a, b in zip(g["frames"], w["frames"])), what
            assert np.array_equal(g["screen"], w["screen"]), what
            assert np.array_equal(g["scope"], w["scope"]), what
            assert g["state"] == w["state"], (what, g["state"], w["state"])
