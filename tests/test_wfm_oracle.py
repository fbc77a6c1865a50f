"""The C restatement of WFMDemod::feed (tests/wfm_oracle.c, the checker of the GPU demodulator bank) against the reference's
own NCO, fftfilt, PhaseDiscriminators and Interpolator: every case of tests/wfm_cases.py recorded by
tests/golden/make_golden_wfm.py into tests/golden/wfm_golden.npz (audio counts of every feed, audio bit for bit or its sha256,
m_magsqPeak, m_magsqCount, m_magsqSum, final squelch state).  Where the reference tree and Qt are present, a `ref` test rebuilds
the recorder and compares 100 random configurations sample for sample."""
import hashlib
import os

import numpy as np
import pytest

from tests import wfm_cases as wc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "wfm_golden.npz")
REF = "/root/reference"


@pytest.fixture(scope="module")
def oracle():
    return wc.build_oracle()


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def test_golden_covers_every_case(golden):
    names = {k.split("/")[0] for k in golden.files}
    assert names == {c["name"] for c in wc.CASES}


def test_cases_cover_what_they_claim():
    by = {c["name"]: c for c in wc.CASES}
    for s in (1, 511, 512, 513, 0):
        assert s in by["splits_edges"]["splits"]
    assert by["one_long_feed"]["splits"] == [by["one_long_feed"]["n"]]
    assert wc.required_bw(80000) == 120000 and wc.required_bw(12500) == 48000 and wc.required_bw(48000) == 48000
    # steps 5, 2.5, 1 and 8 are dyadic, 250000 / 48000 and 384000 / 44100 are not: both schedules have their cases
    dyadic = {c["name"] for c in wc.DYADIC_CASES}
    assert len(dyadic) >= 3 and {"default_240k", "default_120k", "nbfm_48k_step1", "wide_rf250k_384k", "burst_240k_fraccap"} <= dyadic
    assert not dyadic & {"nondyadic_250k", "r384k_to_44k1"}
    assert len({c["cfg"][0] / c["cfg"][2] for c in wc.DYADIC_CASES}) >= 3


@pytest.mark.parametrize("case", wc.CASES, ids=[c["name"] for c in wc.CASES])
def test_oracle_matches_reference_recording(oracle, golden, case):
    r = wc.run_oracle(oracle, case)
    name = case["name"]
    assert [f.size for f in r["feeds"]] == golden[f"{name}/counts"].tolist()
    audio = np.concatenate(r["feeds"]) if r["feeds"] else np.zeros(0, np.int16)
    if f"{name}/audio" in golden.files:
        assert np.array_equal(audio, golden[f"{name}/audio"])
    else:
        assert hashlib.sha256(audio.tobytes()).hexdigest() == str(golden[f"{name}/sha256"])
    s, p = golden[f"{name}/levels"].tolist()
    cnt, op, st = golden[f"{name}/state"].tolist()
    # the restatement adds in the reference's order: the sum is exact too
    assert (r["sum"], r["peak"], r["count"], int(r["open"]), r["state"]) == (s, p, cnt, op, st)


def test_splits_do_not_change_the_stream(oracle):
    by = {c["name"]: c for c in wc.CASES}
    a = wc.run_oracle(oracle, by["splits_edges"])
    b = wc.run_oracle(oracle, by["one_long_feed"])
    assert np.array_equal(np.concatenate(a["feeds"]), np.concatenate(b["feeds"]))
    assert (a["sum"], a["peak"], a["count"], a["state"]) == (b["sum"], b["peak"], b["count"], b["state"])
    # feeds that complete no block produce no audio
    sizes = [f.size for f in a["feeds"]]
    assert sizes[0] == 0 and sizes[1] > 0 and sizes[4:10] == [0] * 6     # 1 sample; 1 + 511 fills the first block; 2, 3, 5 ... do not


def test_level_edge_case_straddles_the_level(oracle):
    r = wc.run_oracle(oracle, {c["name"]: c for c in wc.CASES}["level_edge"])
    frac = r["ge"] / r["count"]
    assert 0.3 < frac < 0.7, frac                       # samples fall on both sides of m_squelchLevel all the time
    assert r["peak"] < 1.2 * 10 ** -0.6                 # ... while the power never moves away from it


def test_burst_cases_saturate_and_reopen(oracle):
    for name, cap in (("burst_48k", 1250), ("burst_240k_fraccap", 8001)):
        c = {c["name"]: c for c in wc.CASES}[name]
        o = wc.OracleWfm(oracle, c["cfg"])
        iq = wc.inputs(c)
        states, opens = [], []
        for k in range(0, c["n"], 64):
            o.feed(iq[2 * k: 2 * (k + 64)])
            states.append(o.squelch_state()); opens.append(o.squelch_open())
        assert max(states) == cap and min(states[len(states) // 4:]) == 0
        flips = int(np.count_nonzero(np.diff(np.array(opens, int))))
        assert flips >= 6, flips


def test_wrap_case_wraps(oracle):
    r = wc.run_oracle(oracle, {c["name"]: c for c in wc.CASES}["vol10_fullscale_noise"])
    a = np.concatenate(r["feeds"]).astype(np.int32)
    assert np.abs(np.diff(a)).max() > 40000             # jumps across the int16 range: the conversion wrapped


def test_random_cases_cover_the_branches(oracle):
    """the 100 random cases (the GPU banks of tests/test_demod_random_gpu.py run them too) through the oracle: a floor on how
    many carry audio.  57 do with the generator and seed of tests/wfm_cases.py; the floor is a condition on the inputs"""
    audible = sum(bool(np.concatenate(wc.run_oracle(oracle, case)["feeds"]).any()) for case in wc.random_cases())
    assert audible >= 40, audible


@pytest.mark.ref
@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "sdrbase", "dsp")), reason="no reference tree here")
def test_oracle_vs_rebuilt_recorder_random(oracle):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_golden_wfm as mg
    if not mg.available(REF):
        pytest.skip("Qt headers not available")
    exe = mg.build_recorder(REF)
    cases = wc.random_cases()
    assert len(cases) == 100
    for case in cases:
        want = mg.record(exe, case["cfg"], wc.inputs(case), case["splits"])
        got = wc.run_oracle(oracle, case)
        assert [f.size for f in got["feeds"]] == [f.size for f in want["feeds"]], case
        for g, w in zip(got["feeds"], want["feeds"]):
            assert np.array_equal(g, w), case
        assert (got["sum"], got["peak"], got["count"], got["open"], got["state"]) == (want["sum"], want["peak"], want["count"], want["open"], want["state"]), case
