"""The C restatement of AMDemod::processOneSample (tests/am_oracle.c, the checker of the GPU demodulator bank) against the
reference's own NCO, Interpolator, MovingAverageUtil, DoubleBufferFIFO, SimpleAGC, Bandpass and StepFunctions: every case of
tests/am_cases.py recorded by tests/golden/make_golden_am.py into tests/golden/am_golden.npz (audio counts of every feed,
audio bit for bit or its sha256, m_magsq, m_magsqSum, m_magsqPeak, m_magsqCount, final squelch state).  Where the reference
tree and Qt are present, a `ref` test rebuilds the recorder and compares 100 random configurations sample for sample."""
import hashlib
import os

import numpy as np
import pytest

from tests import am_cases as ac

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "am_golden.npz")
REF = "/root/reference"
BY = {c["name"]: c for c in ac.CASES}


@pytest.fixture(scope="module")
def oracle():
    return ac.build_oracle()


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def runs(oracle):
    """every case through the oracle once, shared by the tests below"""
    return {c["name"]: ac.run_oracle(oracle, c) for c in ac.CASES}


def test_golden_covers_every_case(golden):
    names = {k.split("/")[0] for k in golden.files}
    assert names == {c["name"] for c in ac.CASES}


@pytest.mark.parametrize("case", ac.CASES, ids=[c["name"] for c in ac.CASES])
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
    for c in ac.CASES:
        assert 60000 <= c["n"] <= 150000, c["name"]
    for name in ("default_airband", "burst", "burst_bandpass", "zero_gap", "nondyadic_62500"):
        for s in (0, 1, 2):
            assert s in BY[name]["splits"], (name, s)
    for s in (1, 15, 16, 17, 0):
        assert s in BY["splits_edges"]["splits"]
    assert BY["one_long_feed"]["splits"] == [BY["one_long_feed"]["n"]]
    assert BY["burst"]["sig"] == BY["burst_bandpass"]["sig"] and BY["burst_bandpass"]["cfg"][7] == 1 and BY["burst"]["cfg"][7] == 0
    c = BY["r96k_to_44k1"]["cfg"]
    assert (c[2] // 20, c[2] // 10, c[2] // 5, c[2] // 24) == (2205, 4410, 8820, 1837)
    # 62500 / 48000 is not dyadic: the resampler schedule of that case is the serial one
    step = np.float32(62500) / np.float32(48000)
    assert all(float(step * np.float32(1 << q)) != np.floor(float(step * np.float32(1 << q))) for q in range(11))


def test_first_input_already_emits_an_output(oracle):
    o = ac.OracleAm(oracle, BY["default_airband"]["cfg"])
    assert o.feed(np.zeros(2, np.int16)).size == 1
    assert o.feed(np.zeros(2 * 299999, np.int16)).size == 240000           # 300 000 inputs at 60000 -> 48000: 240 001 outputs


def test_splits_do_not_change_the_stream(runs):
    a, b = runs["splits_edges"], runs["one_long_feed"]
    assert np.array_equal(np.concatenate(a["feeds"]), np.concatenate(b["feeds"]))
    assert (a["magsq"], a["sum"], a["peak"], a["count"], a["state"]) == (b["magsq"], b["sum"], b["peak"], b["count"], b["state"])


def test_burst_cases_open_close_and_wrap_the_agc_history(runs):
    for name in ("burst", "burst_bandpass"):
        rate = BY[name]["cfg"][2]
        p = runs[name]["probe"]
        assert p["transitions"] >= 6, p
        assert p["count_zero"] > 0 and p["count_cap"] > 0, p                # the counter reaches 0 and rate / 10
        assert p["fed"] > rate // 10, p                                     # more than H fed samples: the AGC history wraps ...
        assert p["fed_after_closure"] > 0, p                                # ... and keeps being fed after a closure
    # the Bandpass ring has to survive closures: the filtered case reopens (its ring then still holds the samples from before the
    # closure), and the filter is really in the path
    a, b = np.concatenate(runs["burst"]["feeds"]), np.concatenate(runs["burst_bandpass"]["feeds"])
    assert runs["burst_bandpass"]["probe"]["transitions"] >= 3
    assert a.size == b.size and np.count_nonzero(a != b) > a.size // 4


def test_wrap_case_wraps(runs):
    a = np.concatenate(runs["wrap_vol10"]["feeds"]).astype(np.int32)
    assert np.abs(np.diff(a)).max() > 40000             # a jump across the int16 range between neighbours: the conversion wrapped


def test_zero_gap_keeps_the_squelch_open_and_skips_the_agc(runs):
    p = runs["zero_gap"]["probe"]
    assert p["transitions"] == 1 and runs["zero_gap"]["open"], p            # opened once, never closed
    assert p["open_root_zero"] >= 1 and p["fed"] == p["open"] - p["open_root_zero"], p


def test_level_edge_case_straddles_the_level(runs):
    p = runs["level_edge"]["probe"]
    assert p["below_changes"] >= 1000, p


def test_earliest_open_reads_one_unwritten_slot(runs):
    r = runs["earliest_open"]
    rate = BY["earliest_open"]["cfg"][2]
    assert r["probe"]["first_open"] == rate // 20 - 1 and r["probe"]["unwritten_reads"] == 1, r["probe"]
    a = np.concatenate(r["feeds"])
    assert not a[: rate // 20].any()                    # the ruling: that slot holds 0, the sample is 0


def test_mute_and_zero_cases_are_silent(runs):
    for name in ("audio_mute", "all_zero"):
        assert not np.concatenate(runs[name]["feeds"]).any()
    assert runs["audio_mute"]["open"] and not runs["all_zero"]["open"]
    assert runs["audio_mute"]["probe"]["fed"] == 0


def test_random_cases_cover_the_branches(oracle):
    """the 100 random cases (the GPU banks of tests/test_demod_random_gpu.py run them too) through the oracle: a floor on how
    many open the squelch.  With the generator and seed of tests/am_cases.py 67 open, 8 feed the AGC after a closure and 16
    read an unwritten slot; the floor is a condition on the inputs"""
    probes = [ac.run_oracle(oracle, case)["probe"] for case in ac.random_cases()]
    opened = sum(p["open"] > 0 for p in probes)
    print("open", opened, "fed_after_closure", sum(p["fed_after_closure"] > 0 for p in probes), "unwritten_reads", sum(p["unwritten_reads"] > 0 for p in probes))
    assert opened >= 40, opened


@pytest.mark.ref
@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "sdrbase", "dsp")), reason="no reference tree here")
def test_oracle_vs_rebuilt_recorder_random(oracle):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_golden_am as mg
    if not mg.available(REF):
        pytest.skip("Qt headers not available")
    exe = mg.build_recorder(REF)
    cases = ac.random_cases()
    assert len(cases) == 100
    for case in cases:
        want = mg.record(exe, case["cfg"], ac.inputs(case), case["splits"])
        got = ac.run_oracle(oracle, case)
        assert [f.size for f in got["feeds"]] == [f.size for f in want["feeds"]], case
        for g, w in zip(got["feeds"], want["feeds"]):
            assert np.array_equal(g, w), case
        assert (got["magsq"], got["sum"], got["peak"], got["count"], got["open"], got["state"]) == \
               (want["magsq"], want["sum"], want["peak"], want["count"], want["open"], want["state"]), case
