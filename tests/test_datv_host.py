"""CPU: sdrangel_amd/csrc/datv_scan.hpp and datv_design.hpp -- the per-symbol and per-chunk step the walk kernel runs and the
design the handle builds -- on the host, through tests/datv_check.cpp: a stand-alone program that runs them, with a scalar interp,
on a trace of filtered samples and compares symbols, points, the device half of every measurement and the state with what
tests/datv_oracle.cpp gave for the same stream.  The program is built plain and with -fsanitize=address,undefined and run as a
program; nothing is preloaded.  The tables come from the restated sinf / cosf / atan2f there and from this machine's libm in the
oracle: equal outputs say the two agree here."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import datv_cases as dc

NAMES = ("nearest", "linear", "rrc", "mod_bpsk", "mod_apsk32", "mod_qam256", "hard_metric", "viterbi", "allow_drift", "ratio_1p2_taps3",
         "ratio_8_taps63", "ratio_8_taps64", "omega_300_no_symbol", "omega_300_linear", "ratio_1p05_mu_negative", "ratio_1p05_linear", "meas_100", "meas_128", "drift_reset_down", "timing_fast", "silence",
         "noise", "silence_then_full")


@pytest.fixture(scope="module")
def oracle():
    return dc.build_oracle()


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def checker(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("datv_check") / ("datv_check_" + request.param))
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if request.param == "sanitized" else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-I" + dc.CSRC] + flags +
                          [os.path.join(dc.ROOT, "tests", "datv_check.cpp"), "-o", exe, "-lm"])
    return exe


@pytest.fixture(scope="module")
def traces(oracle, tmp_path_factory):
    """per case the stream fed whole: the trace file and the oracle's counts"""
    d = tmp_path_factory.mktemp("datv_traces")
    out = {}
    for name in NAMES:
        case = dc.BY_NAME[name]
        o = dc.OracleDatv(oracle, case["cfg"])
        f = o.feed(dc.inputs(case))
        x = o.written()
        st = dc.State()
        oracle.dto_state(o.h, C.byref(st))
        o.close()
        m = np.stack([f["meas"][k] for k in ("freq", "est_insp", "est_sp", "est_ep")], axis=1).astype(np.uint32) if f["meas"].size else np.zeros((0, 4), np.uint32)
        path = str(d / (name + ".bin"))
        with open(path, "wb") as fh:
            fh.write(bytes(dc.as_struct(case["cfg"])))
            fh.write(np.array([x.size // 2, f["cost"].size, f["points"].size // 2, f["meas"].size], np.int64).tobytes())
            for a in (x, f["cost"], f["symbol"], f["points"], m):
                fh.write(np.ascontiguousarray(a).tobytes())
            fh.write(bytes(st))
        out[name] = (path, f["cost"].size)
    return out


@pytest.mark.parametrize("name", NAMES)
def test_the_step_on_a_trace_equals_the_oracle(checker, traces, name):
    path, n_sym = traces[name]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([checker, path], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and r.stdout.startswith(f"ok {n_sym} symbols"), (name, r.returncode, r.stdout[-300:], r.stderr[-1500:])
    assert n_sym > 0


def test_a_wrong_trace_is_told_apart(checker, traces, tmp_path):
    path, _ = traces["rrc"]
    raw = bytearray(open(path, "rb").read())
    raw[C.sizeof(dc.Cfg) + 32 + 8 * 700 + 3] ^= 0x80            # the sign of one filtered sample
    bad = tmp_path / "bad.bin"
    bad.write_bytes(bytes(raw))
    r = subprocess.run([checker, str(bad)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and r.stdout.startswith("FAIL"), (r.returncode, r.stdout, r.stderr[-500:])
