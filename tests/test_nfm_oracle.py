"""The C restatement of NFMDemod::feed (tests/nfm_oracle.c, the checker of the GPU demodulator bank) against the reference's own
NCO, Interpolator, PhaseDiscriminators, MovingAverageUtil, DoubleBufferFIFO and Bandpass: every case of tests/nfm_cases.py
recorded by tests/golden/make_golden_nfm.py into tests/golden/nfm_golden.npz (audio counts of every feed, audio bit for bit or
its sha256, the moving average, m_magsqSum, m_magsqPeak, m_magsqCount, final squelch state).  The probe counters of the oracle
show that each case reaches the branch it is named after.  Where the reference tree and Qt are present, a `ref` test rebuilds the
recorder and compares 100 random configurations sample for sample."""
import hashlib
import os

import numpy as np
import pytest

from tests import nfm_cases as nc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "nfm_golden.npz")
REF = "/root/reference"
BY = {c["name"]: c for c in nc.CASES}


@pytest.fixture(scope="module")
def oracle():
    return nc.build_oracle()


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def runs(oracle):
    """every case through the oracle once, shared by the tests below"""
    return {c["name"]: nc.run_oracle(oracle, c) for c in nc.CASES}


def test_golden_covers_every_case(golden):
    names = {k.split("/")[0] for k in golden.files}
    assert names == {c["name"] for c in nc.CASES}


@pytest.mark.parametrize("case", nc.CASES, ids=[c["name"] for c in nc.CASES])
def test_oracle_matches_reference_recording(runs, golden, case):
    name = case["name"]
    r = runs[name]
    assert [f.size for f in r["feeds"]] == golden[f"{name}/counts"].tolist()
    audio = np.concatenate(r["feeds"]) if r["feeds"] else np.zeros(0, np.int16)
    if f"{name}/audio" in golden.files:
        assert np.array_equal(audio, golden[f"{name}/audio"])
    else:
        assert hashlib.sha256(audio.tobytes()).hexdigest() == str(golden[f"{name}/sha256"])
    m, s, p = golden[f"{name}/levels"].tolist()
    cnt, op, st = golden[f"{name}/state"].tolist()
    # the restatement adds in the reference's order: the sum is exact too
    assert (r["magsq"], r["sum"], r["peak"], r["count"], int(r["open"]), r["state"]) == (m, s, p, cnt, op, st)


def test_cases_cover_what_they_claim():
    assert len(nc.CASES) == 16
    for c in nc.CASES:
        assert 60000 <= c["n"] <= 120000, c["name"]
    for name in ("default_60k", "burst_gate5", "burst_gate1", "gate60_clamped", "zero_gap", "nondyadic_62500"):
        for s in (0, 1, 31, 32, 33):
            assert s in BY[name]["splits"], (name, s)
    for s in (1, 31, 32, 33, 0):
        assert s in BY["splits_edges"]["splits"]
    assert BY["one_long_feed"]["splits"] == [BY["one_long_feed"]["n"]]
    assert nc.gate_samples(BY["gate60_clamped"]["cfg"]) == 28800 > 24000
    assert nc.gate_samples(BY["r96k_to_44k1"]["cfg"]) == 2205
    # bursts: audio-rate runs on both sides of the opening count and of the counter's cap
    for name, runs_in in (("burst_gate5", nc.BURST_RUNS_5), ("burst_gate1", nc.BURST_RUNS_1)):
        g = nc.gate_samples(BY[name]["cfg"])
        audio_runs = [r * 4 // 5 for r in runs_in]
        assert min(audio_runs) < g < 2 * g < max(audio_runs), name
        assert any(g < r < 2 * g for r in audio_runs), name
    # 62500 / 48000 is not dyadic: the resampler schedule of that case is the serial one
    step = np.float32(62500) / np.float32(48000)
    assert all(float(step * np.float32(1 << q)) != np.floor(float(step * np.float32(1 << q))) for q in range(11))


def test_first_input_already_emits_an_output(oracle):
    o = nc.OracleNfm(oracle, BY["default_60k"]["cfg"])
    assert o.feed(np.zeros(2, np.int16)).size == 1
    assert o.feed(np.zeros(2 * 299999, np.int16)).size == 240000           # 300 000 inputs at 60000 -> 48000: 240 001 outputs


def test_splits_do_not_change_the_stream(runs):
    a, b = runs["splits_edges"], runs["one_long_feed"]
    assert np.array_equal(np.concatenate(a["feeds"]), np.concatenate(b["feeds"]))
    assert (a["magsq"], a["sum"], a["peak"], a["count"], a["state"]) == (b["magsq"], b["sum"], b["peak"], b["count"], b["state"])


def test_every_case_reaches_its_branch(runs):
    p = {name: r["probe"] for name, r in runs.items()}
    for name in ("burst_gate5", "burst_gate1"):
        assert p[name]["transitions"] >= 6, p[name]                         # opens and closes three times at least
        assert p[name]["count_zero"] > 0 and p[name]["count_cap"] > 0, p[name]
        assert p[name]["below_changes"] >= 6 and p[name]["open"] > 20000, p[name]
    for name in ("default_60k", "nondyadic_62500", "step1_48k", "r96k_to_44k1", "wide_25k", "fullscale_noise", "one_long_feed"):
        assert p[name]["transitions"] == 1 and p[name]["open"] > 40000 and p[name]["count_cap"] > 0, (name, p[name])
        assert p[name]["clamped_reads"] == 0
    g = p["gate60_clamped"]
    assert g["open"] > 60000 and g["clamped_reads"] == g["open"], g         # every read of that case is a clamped one
    assert p["wrap_vol10"]["wraps"] > 1000, p["wrap_vol10"]                 # jumps across the int16 range between neighbours
    assert p["zero_gap"]["zero_ci"] >= 50 and p["zero_gap"]["below_changes"] >= 3 and runs["zero_gap"]["open"], p["zero_gap"]
    assert p["level_edge"]["below_changes"] >= 1000, p["level_edge"]
    assert p["all_zero"]["zero_ci"] == runs["all_zero"]["count"] and p["all_zero"]["open"] == 0


def test_clamped_read_hands_over_the_current_sample(oracle):
    """readBack(28800) on a line of 24000 entries names the slot just written.  A gate of exactly 24000 reads the same slot
    without the clamp, so once both squelches are open and both Bandpass rings hold 301 inputs of the same stretch the two
    audio streams are equal; a gate of 23520 reads 23520 samples back and gives another stream."""
    case = BY["gate60_clamped"]
    x = nc.inputs(case)
    cfg = list(case["cfg"])
    outs = {}
    for gate in (60, 50, 49):
        cfg[8] = gate
        outs[gate] = nc.OracleNfm(oracle, tuple(cfg)).feed(x)
    a, b, c = outs[60], outs[50], outs[49]
    first = int(np.flatnonzero(a)[0])
    assert 28800 <= first <= 28800 + 301 and not b[:24000].any() and b[24001:28000].any()
    assert np.array_equal(a[first + 400:], b[first + 400:])
    assert np.count_nonzero(a[first + 400:] != c[first + 400:]) > a.size // 4


def test_mute_and_zero_cases_are_silent(runs):
    for name in ("audio_mute", "all_zero"):
        assert not np.concatenate(runs[name]["feeds"]).any()
    assert runs["audio_mute"]["open"] and not runs["all_zero"]["open"]
    assert runs["audio_mute"]["probe"]["open"] == 0                         # muted: the Bandpass is never advanced


def test_random_cases_cover_the_branches(oracle):
    """the 100 random cases (the GPU banks of tests/test_demod_random_gpu.py run them too) through the oracle: a floor on how
    many open the squelch.  With the generator and seed of tests/nfm_cases.py 51 open, 17 wrap the conversion and 61 reach
    the counter's cap; none has a gate of 24000 samples or more, so `clamped_reads` stays with the named case gate60_clamped"""
    probes = [nc.run_oracle(oracle, case)["probe"] for case in nc.random_cases()]
    opened = sum(p["open"] > 0 for p in probes)
    print("open", opened, {k: sum(p[k] > 0 for p in probes) for k in ("wraps", "count_cap", "clamped_reads")})
    assert opened >= 30, opened


@pytest.mark.ref
@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "sdrbase", "dsp")), reason="no reference tree here")
def test_oracle_vs_rebuilt_recorder_random(oracle):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_golden_nfm as mg
    if not mg.available(REF):
        pytest.skip("Qt headers not available")
    exe = mg.build_recorder(REF)
    cases = nc.random_cases()
    assert len(cases) == 100
    for case in cases:
        want = mg.record(exe, case["cfg"], nc.inputs(case), case["splits"])
        got = nc.run_oracle(oracle, case)
        assert [f.size for f in got["feeds"]] == [f.size for f in want["feeds"]], case
        for g, w in zip(got["feeds"], want["feeds"]):
            assert np.array_equal(g, w), case
        assert (got["magsq"], got["sum"], got["peak"], got["count"], got["open"], got["state"]) == \
               (want["magsq"], want["sum"], want["peak"], want["count"], want["open"], want["state"]), case
