"""CPU: the synchronous branch of tests/am_oracle.c (amo_create_ex with pll set: AMDemod::processOneSample with m_pll, one open sample
at a time) against the reference.  Every case of tests/golden/am_sync_golden.npz bit for bit: the audio of every feed, after every
feed m_magsq, m_magsqSum (the oracle adds in the reference's order), m_magsqPeak, m_magsqCount, the squelch state, getPllLocked()
and the bits of getPllFrequency(), the design products, `opens`, the loop's probe counts, and for the trace case the recorder's
per-open-sample trace column by column.  amo_create_ex with pll = 0 is amo_create.  The 100 cases of
am_sync_cases.random_cases() against tests/golden/am_sync_random_golden.npz (digests, recorded with the rebuilt recorder), and,
where the reference tree and Qt are present, against the rebuilt recorder in full (`ref`).  The shares the draw must reach are
asserted on the oracle's probes."""
import os
import sys
import tempfile

import numpy as np
import pytest

from tests import am_cases as ac
from tests import am_sync_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
GOLDEN = os.path.join(ROOT, "tests", "golden", "am_sync_golden.npz")
RANDOM_GOLDEN = os.path.join(ROOT, "tests", "golden", "am_sync_random_golden.npz")


@pytest.fixture(scope="module")
def oracle():
    return sc.build_oracle()


@pytest.fixture(scope="module")
def gold():
    g = np.load(GOLDEN)
    return {k: g[k] for k in g.files}


@pytest.fixture(scope="module")
def rgold():
    g = np.load(RANDOM_GOLDEN)
    return {k: g[k] for k in g.files}


@pytest.fixture(scope="module")
def random_runs(oracle):
    """the oracle over the 100 random cases, once"""
    cases = sc.random_cases()
    return cases, [sc.run_oracle(oracle, c) for c in cases]


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("case", sc.CASES, ids=[c["name"] for c in sc.CASES])
def test_oracle_matches_the_recording(oracle, gold, case):
    name = case["name"]
    x = sc.inputs(case)
    assert sc.sha(x) == str(gold[name + "/in_sha256"])
    trace = None
    if case["expect"].get("trace"):
        d = tempfile.mkdtemp()
        trace = (os.path.join(d, "trace.bin"), os.path.join(d, "trace.bin.sb"))
    got = sc.run_oracle(oracle, case, trace=trace, x=x)
    assert [f.size for f in got["feeds"]] == list(gold[name + "/counts"])
    audio = np.concatenate(got["feeds"])
    want = gold[name + "/audio"]
    assert np.array_equal(audio, want), (name, int(np.flatnonzero(audio != want)[0]))
    # m_magsq, m_magsqSum and m_magsqPeak after every feed, to the bit: the sum too
    assert bits_equal(got["levels"], gold[name + "/levels"].astype(np.float64)), name
    assert np.array_equal(got["state"], gold[name + "/state"]), name
    assert np.array_equal(got["opens"], gold[name + "/opens"]), name
    for part, key in zip(got["design"], ("taps", "filter", "coef")):
        assert bits_equal(part, gold[f"{name}/{key}"].astype(np.float32)), (name, key)
    sp = got["sync_probe"]
    assert [sp["sat_hi"], sp["sat_lo"], sp["lock_up"], sp["lock_down"]] == list(gold[name + "/probe"]), name
    if trace:
        tr, sb = np.fromfile(trace[0], np.float32).reshape(-1, 7), np.fromfile(trace[1], np.float32).reshape(-1, 2)
        want_tr, want_sb = gold[name + "/trace"].astype(np.float32), gold[name + "/trace_sb"].astype(np.float32)
        assert tr.shape == want_tr.shape and sb.shape == want_sb.shape and tr.shape[0] == sp["open"] > 2000
        for col, what in enumerate(("re", "im", "filtered re", "filtered im", "m_yRe", "m_yIm", "demod")):
            assert bits_equal(tr[:, col], want_tr[:, col]), (what, int(np.flatnonzero(tr[:, col].view(np.uint32) != want_tr[:, col].view(np.uint32))[0]))
        for col, what in enumerate(("sideband re", "sideband im")):
            assert bits_equal(sb[:, col], want_sb[:, col]), what


@pytest.mark.parametrize("case", ac.CASES, ids=[c["name"] for c in ac.CASES])
def test_pll_off_is_the_envelope_oracle(oracle, case):
    """amo_create_ex with pll = 0, whatever the other three arguments, gives what amo_create gives"""
    want = ac.run_oracle(oracle, case)
    got = sc.run_oracle(oracle, dict(case, sync=(0, 2, 8000, 2400.0)), x=ac.inputs(case))
    assert [f.size for f in got["feeds"]] == [f.size for f in want["feeds"]]
    for g, w in zip(got["feeds"], want["feeds"]):
        assert np.array_equal(g, w)
    assert (got["magsq"], got["sum"], got["peak"], got["count"], got["open"], int(got["state"][-1, 2])) == \
           (want["magsq"], want["sum"], want["peak"], want["count"], want["open"], want["state"])
    assert got["probe"] == want["probe"] and got["pll"] == (False, 0.0) and got["sync_probe"]["open"] == 0


def test_random_draw_reaches_its_shares(random_runs):
    cases, runs = random_runs
    assert len(cases) == 100 and len({c["name"] for c in cases}) == 100
    sh = sc.assert_random_shares(cases, runs)
    assert sh["sync"] + sh["envelope"] == 100
    # the rates, squelch levels and design values the draw is for all occur
    assert {(c["cfg"][0], c["cfg"][2]) for c in cases} == set(sc.RATES)
    assert {c["cfg"][5] for c in cases} == {-100.0, -60.0, -40.0, -25.5, -10.0}
    assert {c["sync"][2] for c in cases} == {0, 8000, 44100, 48000} and {c["sync"][3] for c in cases} == {0.0, 2400.0, 3000.0, 5000.0}
    assert max(c["n"] for c in cases) <= sc.MAX_N


def compare_with_record(case, got, counts, audio_sha, levels, state, opens_last):
    name = case["name"]
    assert [f.size for f in got["feeds"]] == list(counts), name
    for i, f in enumerate(got["feeds"]):
        assert sc.sha(f) == audio_sha[i], (name, "audio of feed", i, case)
    assert bits_equal(got["levels"], np.asarray(levels, np.float64).reshape(-1, 3)), (name, "levels", case)
    assert np.array_equal(got["state"], np.asarray(state).reshape(-1, 5)), (name, "state", case)
    assert int(got["opens"][-1]) == int(opens_last), (name, "opens", case)


def test_oracle_matches_the_random_recording(random_runs, rgold):
    """runs anywhere: the committed digests of what the rebuilt recorder gave for the 100 random cases"""
    cases, runs = random_runs
    assert [k for k in sorted({k.split("/")[0] for k in rgold if k != "host"})] == sorted(c["name"] for c in cases)
    host = str(rgold["host"])
    assert host.startswith("glibc 2.") and host.endswith("fma=1"), host
    assert os.path.getsize(RANDOM_GOLDEN) < 547302
    for c, r in zip(cases, runs):
        name = c["name"]
        assert sc.sha(sc.inputs(c)) == str(rgold[name + "/in_sha256"]), name
        compare_with_record(c, r, rgold[name + "/counts"], [str(v) for v in rgold[name + "/audio_sha256"]], rgold[name + "/levels"],
                            rgold[name + "/state"], rgold[name + "/opens"][-1])


@pytest.mark.ref
@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "sdrbase", "dsp")), reason="no reference tree here")
def test_oracle_vs_rebuilt_recorder_random(random_runs):
    """the proof: the recorder rebuilt from the reference tree, all 100 random cases feed by feed and sample for sample, the state
    after every feed and the design products"""
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_golden_am_sync as mg
    if not mg.available(REF):
        pytest.skip("Qt headers not available")
    exe = mg.build_recorder(REF)
    cases, runs = random_runs
    assert len(cases) == 100
    for c, got in zip(cases, runs):
        want = mg.record(exe, c, sc.inputs(c))
        assert [f.size for f in got["feeds"]] == [f.size for f in want["feeds"]], c
        for i, (g, w) in enumerate(zip(got["feeds"], want["feeds"])):
            assert np.array_equal(g, w), (c, i, int(np.flatnonzero(g != w)[0]))
        assert bits_equal(got["levels"], want["levels"]), c
        assert np.array_equal(got["state"], want["state"][:, :5]), c
        assert np.array_equal(got["opens"], want["opens"]), c
        if c["sync"][0]:
            assert int(want["state"][-1, 6]) == got["sync_probe"]["reopenings"] and int(want["state"][-1, 7]) == got["sync_probe"]["bad"], c
            for part, key in zip(got["design"], ("taps", "filt", "coef")):
                assert bits_equal(part, want[key]), (c, key)
