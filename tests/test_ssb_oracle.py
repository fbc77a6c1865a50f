"""The C restatement of SSBDemod::feed (tests/ssb_oracle.c, the checker of the GPU demodulator bank) against the reference's own
NCO, Interpolator, fftfilt, MagAGC, DoubleBufferFIFO and StepFunctions: every case of tests/ssb_cases.py recorded by
tests/golden/make_golden_ssb.py into tests/golden/ssb_golden.npz (audio and spectrum counts of every feed, both streams bit for
bit or their sha256, m_magsq, m_magsqSum, m_magsqPeak, m_magsqCount, m_audioActive, m_undersampleCount and the AGC's getValue(),
getStepValue(), getStepDownValue()).  The probe counters of the oracle show that each case reaches the branch it is named
after.  Where the reference tree and Qt are present, a `ref` test rebuilds the recorder and compares 100 random configurations
sample for sample."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

from tests import ssb_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ssb_golden.npz")
REF = "/root/reference"
BY = {c["name"]: c for c in sc.CASES}


@pytest.fixture(scope="module")
def oracle():
    return sc.build_oracle()


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def runs(oracle):
    """every case through the oracle once, shared by the tests below"""
    return {c["name"]: sc.run_oracle(oracle, c) for c in sc.CASES}


def _cat(parts):
    return np.concatenate(parts) if parts else np.zeros((0, 2), np.int16)


def _agc_state(r):
    """what the recorder reads off MagAGC's public face: (Real) m_u0, getStepValue(), getStepDownValue()"""
    st = r["state"]
    return float(np.float32(st[6])), st[8], st[9]


def test_golden_covers_every_case(golden):
    names = {k.split("/")[0] for k in golden.files}
    assert names == {c["name"] for c in sc.CASES}


@pytest.mark.parametrize("case", sc.CASES, ids=[c["name"] for c in sc.CASES])
def test_oracle_matches_reference_recording(runs, golden, case):
    name = case["name"]
    r = runs[name]
    assert [[a.shape[0], s.shape[0]] for a, s in zip(r["audio"], r["spec"])] == golden[f"{name}/counts"].tolist()
    for key in ("audio", "spec"):
        full = _cat(r[key])
        if f"{name}/{key}" in golden.files:
            assert np.array_equal(full, golden[f"{name}/{key}"]), key
        else:
            assert hashlib.sha256(full.tobytes()).hexdigest() == str(golden[f"{name}/{key}_sha256"]), key
    m, s, p = golden[f"{name}/levels"].tolist()
    cnt, act, usc = golden[f"{name}/state"].tolist()
    # the restatement adds in the reference's order: the sum is exact too
    assert (r["magsq"], r["sum"], r["peak"], r["count"], int(r["active"]), int(r["state"][4])) == (m, s, p, cnt, act, usc)
    u0, sv, sdv = golden[f"{name}/agc"].tolist()
    got = _agc_state(r)
    assert got[1:] == (sv, sdv)
    assert got[0] == u0 or (np.isnan(got[0]) and np.isnan(u0))


def test_cases_cover_what_they_claim():
    assert {c["name"] for c in sc.CASES} >= {"default_usb", "lsb", "dsb", "binaural", "binaural_flip", "mute", "agc_off", "threshold_disabled", "gate",
                                             "clamping", "step_down_and_back", "short_history", "long_history", "span1", "span8",
                                             "resample_60k_48k", "resample_96k_8k", "zero", "first_block_only"}
    for c in sc.CASES:
        assert c["n"] <= 120000, c["name"]
    assert sc.hn_of(BY["short_history"]["cfg"]) == 16 and sc.hn_of(BY["default_usb"]["cfg"]) == 6144
    assert sc.hn_of(BY["long_history"]["cfg"]) == 98304 > 96000
    assert sc.gate_of(BY["gate"]["cfg"]) == 192
    strong = [r * 4 // 5 for r in sc.GATE_RUNS[0::2]]                      # audio-rate lengths; runs alternate strong, weak
    weak = [r * 4 // 5 for r in sc.GATE_RUNS[1::2]]
    assert min(strong) < 192 < max(strong) and sum(1 for r in strong if r < 192) >= 3
    assert max(weak) > 6144 + 3072 and min(weak) < 6144
    for s in (0, 1, 300, 700, 2000):
        assert s in BY["default_usb"]["splits"]
    assert BY["first_block_only"]["n"] == 700


def test_every_case_reaches_its_branch(runs):
    for c in sc.CASES:
        p = runs[c["name"]]["probe"]
        for key in c["reach"]:
            assert p[key] > 0, (c["name"], key, p)
    g = runs["gate"]["probe"]
    assert g["up_to_down"] >= 2 and g["count_full"] >= 2 and g["gate_full"] >= 3, g
    sd = runs["step_down_and_back"]["probe"]
    assert sd["down_to_up"] >= 2 and sd["down_to_up_early"] >= 1 and sd["step_down_zero"] >= 1, sd
    cl = runs["clamping"]["probe"]
    n_cl = sum(a.shape[0] for a in runs["clamping"]["audio"])
    assert 0 < cl["clamped"] < n_cl, cl                                     # both sides of clampMax
    assert runs["long_history"]["probe"]["dl_wraps"] == 1
    z = runs["zero"]
    assert z["probe"]["nan_writes"] == sc.hn_of(BY["zero"]["cfg"]) + sc.hn_of(BY["zero"]["cfg"]) // 2 - 1, z["probe"]


def test_feed_shapes(runs):
    """feeds that emit nothing, one block and three blocks; the first spectrum group holds one sample"""
    r = runs["default_usb"]
    counts = [a.shape[0] for a in r["audio"]]
    assert counts[:9] == [0, 0, 0, 512, 0, 0, 1536, 0, 512], counts[:9]
    assert all(c % 512 == 0 for c in counts)
    assert all(a.shape[0] % 1024 == 0 for a in runs["dsb"]["audio"])
    f = runs["first_block_only"]
    assert [a.shape[0] for a in f["audio"]] == [0, 0, 512, 0] and sum(s.shape[0] for s in f["spec"]) == 128
    assert sum(s.shape[0] for s in runs["span1"]["spec"]) == sum(a.shape[0] for a in runs["span1"]["audio"])
    n8 = sum(a.shape[0] for a in runs["span8"]["audio"])
    assert sum(s.shape[0] for s in runs["span8"]["spec"]) == (n8 - 1) // 128 + 1


def test_silence_with_the_agc_off_and_with_the_threshold_disabled(runs):
    """m_agc = false never feeds the AGC: m_stepUpCounter stays 0 and getStepValue() is smootherstep(0) = 0.  With the threshold
    disabled feedAndGetValue returns m_u0 and moves no counter.  Either way the audio is silence while the delay line runs."""
    for name in ("agc_off", "threshold_disabled"):
        r = runs[name]
        assert not _cat(r["audio"]).any() and r["active"], name
        assert r["state"][2] == 0 and r["state"][8] == 0.0, name           # m_stepUpCounter, getStepValue()
        assert _cat(r["spec"]).any(), name
    assert _cat(runs["default_usb"]["audio"]).any()
    assert not _cat(runs["mute"]["audio"]).any() and not _cat(runs["zero"]["audio"]).any()


def test_stereo_outputs(runs):
    b, f, m = _cat(runs["binaural"]["audio"]), _cat(runs["binaural_flip"]["audio"]), _cat(runs["default_usb"]["audio"])
    assert np.array_equal(b[:, 0], f[:, 1]) and np.array_equal(b[:, 1], f[:, 0])
    assert np.count_nonzero(b[:, 0] != b[:, 1]) > b.shape[0] // 4
    assert np.array_equal(m[:, 0], m[:, 1])


def test_mono_audio_equals_the_audio_tail_restatement(oracle, runs):
    """independent of tests/ssb_oracle.c: oracle/libsdro.so's sdro_ssbtail_* (the checker of sdrx_audiotail_* kind 1) on the
    sideband stream of libsdro's own front gives the left channel of every mono, unmuted case"""
    L = C.CDLL(os.path.join(sc.ORACLE_DIR, "libsdro.so"))
    L.sdro_backend_new.restype = C.c_void_p
    L.sdro_backend_new.argtypes = [C.c_float, C.c_float, C.c_float, C.c_int32, C.c_float, C.c_float]
    L.sdro_backend_feed.restype = C.c_int64
    L.sdro_backend_feed.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    L.sdro_fftfilt_new.restype = C.c_void_p
    L.sdro_fftfilt_new.argtypes = [C.c_float, C.c_float, C.c_int32]
    L.sdro_fftfilt_run.restype = C.c_int64
    L.sdro_fftfilt_run.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]
    L.sdro_ssbtail_new.restype = C.c_void_p
    L.sdro_ssbtail_new.argtypes = [C.c_int32, C.c_int32, C.c_double, C.c_int32, C.c_int32, C.c_int32, C.c_float]
    L.sdro_ssbtail_process.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    checked = 0
    for case in sc.CASES:
        k = case["cfg"]
        if k["audio_binaural"] or k["audio_mute"] or k["dsb"] or k["rf_bandwidth"] < 0:
            continue
        x = sc.inputs(case)
        n = x.size // 2
        fr = L.sdro_backend_new(float(k["nco_freq"]), float(k["in_rate"]), float(k["audio_rate"]), 16, np.float32(k["rf_bandwidth"]) * np.float32(1.5), 2.0)
        ci = np.zeros(2 * (n + 16), np.float32)
        m = L.sdro_backend_feed(fr, x.ctypes.data, n, ci.ctypes.data)
        rate = np.float32(k["audio_rate"])
        ff = L.sdro_fftfilt_new(np.float32(k["low_cutoff"]) / rate, np.float32(k["rf_bandwidth"]) / rate, 1024)
        sb = np.zeros(2 * (m + 1024), np.float32)
        q = L.sdro_fftfilt_run(ff, 1, ci.ctypes.data, m, sb.ctypes.data)
        tail = L.sdro_ssbtail_new(k["agc"], sc.hn_of(k), 10.0 ** (k["agc_power_threshold"] / 10.0) * 32768.0 ** 2, int(k["agc_power_threshold"] != 100),
                                  sc.gate_of(k), k["agc_clamping"], np.float32(k["volume"] / 4.0))
        audio = np.zeros(max(q, 1), np.int16)
        L.sdro_ssbtail_process(tail, sb.ctypes.data, q, audio.ctypes.data)
        got = _cat(runs[case["name"]]["audio"])
        assert got.shape[0] == q and np.array_equal(got[:, 0], audio[:q]), case["name"]
        checked += 1
    assert checked >= 12


def test_random_cases_cover_the_branches(oracle):
    """the 100 random cases (the GPU banks of tests/test_demod_random_gpu.py run them too) through the oracle: floors on how
    many carry audio and how many send the AGC from up to down.  With the generator and seed of tests/ssb_cases.py 46 are
    audible, 40 go up_to_down, 17 down_to_up, 21 clamp, 35 fill the gate; none wraps the delay line, so `dl_wraps` stays with
    the named case long_history"""
    runs = [sc.run_oracle(oracle, case) for case in sc.random_cases()]
    loud = sum(bool(_cat(r["audio"]).any()) for r in runs)
    moved = sum(r["probe"]["up_to_down"] > 0 for r in runs)
    print("audible", loud, {k: sum(r["probe"][k] > 0 for r in runs) for k in ("up_to_down", "down_to_up", "clamped", "gate_full", "dl_wraps")})
    assert loud >= 40 and moved >= 10, (loud, moved)


@pytest.mark.ref
@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "sdrbase", "dsp")), reason="no reference tree here")
def test_oracle_vs_rebuilt_recorder_random(oracle):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_golden_ssb as mg
    if not mg.available(REF):
        pytest.skip("Qt headers not available")
    exe = mg.build_recorder(REF)
    cases = sc.random_cases()
    assert len(cases) == 100
    for case in cases:
        want = mg.record(exe, case["cfg"], sc.inputs(case), case["splits"])
        got = sc.run_oracle(oracle, case)
        for key in ("audio", "spec"):
            assert [f.shape[0] for f in got[key]] == [f.shape[0] for f in want[key]], (key, case)
            for g, w in zip(got[key], want[key]):
                assert np.array_equal(g, w), (key, case)
        assert (got["magsq"], got["sum"], got["peak"], got["count"], got["active"], int(got["state"][4])) == \
               (want["magsq"], want["sum"], want["peak"], want["count"], want["active"], want["usc"]), case
        a, w = _agc_state(got), want["agc"]
        assert a[1:] == w[1:] and (a[0] == w[0] or (np.isnan(a[0]) and np.isnan(w[0]))), case
