"""CPU: tests/bfm_oracle.c against the recording of the reference's own classes (tests/golden/bfm_golden.npz, made by
tests/golden/make_golden_bfm.py): audio, sink stream and state after every feed, bit for bit; the generator still gives the
recorded inputs; the case set drives the pilot loop through every branch of its step.

The 100 random configurations of bfm_cases.random_cases() (audio rates other than 48000, steps at and just above 1, both resampler
schedules; tests/test_bfm_random_gpu.py runs them on the GPU): the oracle packed as the recorder's results were against the digests
of tests/golden/bfm_random_golden.npz anywhere, and feed by feed in full against the rebuilt recorder where the reference is (`ref`)."""
import os
import sys

import numpy as np
import pytest

from tests import bfm_cases as bc

REF = "/root/reference"


@pytest.fixture(scope="module")
def oracle():
    return bc.build_oracle()


@pytest.fixture(scope="module")
def gold():
    return bc.golden()


@pytest.fixture(scope="module")
def runs(oracle):
    """every case through the oracle, once"""
    return {c["name"]: bc.run_oracle(oracle, c) for c in bc.CASES}


def test_fixture_names_its_host(gold):
    host = str(gold["host"])
    assert host.startswith("glibc 2.") and host.endswith("fma=1"), host


@pytest.mark.parametrize("case", bc.CASES, ids=[c["name"] for c in bc.CASES])
def test_generator_gives_the_recorded_inputs(gold, case):
    want = bc.golden_case(gold, case)
    x = bc.inputs(case)
    assert x.size == 2 * case["n"] and bc.sha(x) == want["in_sha"]
    assert (want["in"] is None) == (case["n"] > bc.IN_FULL)
    if want["in"] is not None:
        assert np.array_equal(x, want["in"])


@pytest.mark.parametrize("case", bc.CASES, ids=[c["name"] for c in bc.CASES])
def test_oracle_equals_the_recording(gold, runs, case):
    want, got = bc.golden_case(gold, case), runs[case["name"]]
    bc.assert_equals_recording(got, want, case["name"])
    for i, (g, w) in enumerate(zip(got["states"], want["states"])):
        assert g["sum"] == w["sum"], (case["name"], i)              # the same additions in the same order


def test_both_resamplers_fire_on_the_same_samples(runs):
    """m_interpolator and m_interpolatorStereo: the same create, the same distance arithmetic from the same start -- what lets the
    bank run both FIRs from one schedule"""
    assert all(r["probe"]["sched_mismatch"] == 0 for r in runs.values())


def test_case_set_goes_through_every_branch_of_the_step(runs):
    tot = {k: sum(r["probe"][k] for r in runs.values()) for k in bc.PROBE}
    print(tot)
    for k in ("ratio", "plus", "minus", "clamp_lo", "clamp_hi", "wrap", "lock_up", "lock_reset"):
        assert tot[k] > 0, (k, tot)


def test_what_the_named_cases_are_there_for(gold, runs):
    by = {c["name"]: c for c in bc.CASES}
    st = lambda name: bc.golden_case(gold, by[name])["states"]
    assert [s["locked"] for s in st("lock_96k")][-1] == 1 and st("lock_96k")[0]["locked"] == 0
    assert runs["pilot_stops"]["probe"]["lock_reset"] > 0 and st("pilot_stops")[-1]["lock_cnt"] == 0
    assert runs["pilot_19k045_48k"]["probe"]["clamp_hi"] > 0 and runs["pilot_18k8"]["probe"]["minus"] > 0
    assert runs["noise_no_pilot"]["probe"]["plus"] > 0 and runs["noise_no_pilot"]["probe"]["minus"] > 0
    a = np.concatenate(bc.golden_case(gold, by["volume_clips"])["audio"]).astype(np.int64)
    d = np.abs(np.diff(a[:, 0]))
    assert d.max() > 40000, "the qint16 conversion never wrapped"
    # the squelch: closed through the first three feeds, open at the end of some later ones, closed again after one
    sq = st("squelch_bursts")
    open_after = [s["sq_state"] > 625 for s in sq]
    assert open_after[:3] == [False] * 3 and any(open_after) and not all(open_after[3:]), open_after
    assert sum(bc.golden_case(gold, by["show_pilot_mono"])["sink_counts"]) == 0
    assert sum(bc.golden_case(gold, by["show_pilot_stereo"])["sink_counts"]) == (by["show_pilot_stereo"]["n"] // 512) * 512
    mono = np.concatenate(bc.golden_case(gold, by["mono_250k"])["audio"])
    assert np.array_equal(mono[:, 0], mono[:, 1]) and np.any(mono)
    stereo = np.concatenate(bc.golden_case(gold, by["stereo_240k"])["audio"])
    assert np.any(stereo[:, 0] != stereo[:, 1])
    assert [s for s in by["stereo_240k"]["splits"][:5]] == [0, 1, 511, 512, 513]


def test_fixture_size(gold):
    import os
    assert os.path.getsize(bc.GOLDEN) <= 547302


# ---------------------------------------------------------------- the random draw
RCASES = bc.random_cases()
RIDS = [c["name"] for c in RCASES]


@pytest.fixture(scope="module")
def rgold():
    return bc.load_random_golden()


@pytest.fixture(scope="module")
def rruns(oracle):
    """every random case through the oracle with its own cuts, once"""
    return [bc.run_oracle(oracle, c) for c in RCASES]


def test_the_random_recording_has_every_case(rgold):
    assert [k for k in rgold if k != "host"] == RIDS
    assert rgold["host"].startswith("glibc 2.") and rgold["host"].endswith("fma=1")
    assert os.path.getsize(bc.RANDOM_GOLDEN) < 547302


@pytest.mark.parametrize("i", range(len(RCASES)), ids=RIDS)
def test_oracle_equals_the_random_recording(rruns, rgold, i):
    """lengths and digests of audio and sink stream and every state word after every feed, m_magsqSum to the bit: the oracle's
    results packed the way the recorder's were"""
    case, want = RCASES[i], rgold[RCASES[i]["name"]]
    mine = bc.pack_digests([case], [rruns[i]])
    for key in bc.PER_CASE + bc.PER_FEED:
        assert mine[key].shape == want[key].shape and np.array_equal(mine[key], want[key]), (case["name"], key, case)


def test_the_random_draw_keeps_its_shares(rruns):
    s = bc.assert_random_shares(RCASES, rruns)
    print(s)
    short = [c for c in RCASES if c["n"] <= bc.WIDE_N]
    assert len(short) >= 40 and {(bc.is_dyadic(c), c["cfg"]["stereo"]) for c in short} == {(False, 0), (False, 1), (True, 0), (True, 1)}
    assert {(c["cfg"]["in_rate"], c["cfg"]["audio_rate"]) for c in RCASES} == set(bc.RANDOM_RATES)
    assert {c["sig"]["kind"] for c in RCASES} == {"mpx", "noise_full", "zero"}
    assert {c["cfg"][k] for c in RCASES for k in ("af",)} == {3000.0, 15000.0, 20000.0} and {c["cfg"]["vol"] for c in RCASES} == {0.5, 2.0, 10.0, 400.0}
    assert any(c["sig"].get("amp", 0) > 32767 for c in RCASES) and sum("runs" in c["sig"] for c in RCASES) >= 20
    assert sum("p_on" in c["sig"] for c in RCASES) >= 15


@pytest.mark.ref
@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "sdrbase", "dsp")), reason="no reference tree here")
def test_oracle_equals_the_rebuilt_recorder_on_the_random_draw(rruns):
    """what proves tests/bfm_oracle.c at audio rates other than 48000: every l, r pair, every Sample of the sink stream and the state
    after every feed of every random case against the reference's own classes"""
    sys.path.insert(0, os.path.join(bc.ROOT, "tests", "golden"))
    import make_golden_bfm as mg
    if not mg.available(REF):
        pytest.skip("Qt headers not available")
    exe = mg.build_recorder(REF)
    for case, got in zip(RCASES, rruns):
        want = mg.record_case(exe, case, bc.inputs(case))
        assert len(got["audio"]) == len(want["audio"]) == len(case["splits"]), case
        for i in range(len(case["splits"])):
            assert np.array_equal(got["audio"][i], want["audio"][i]), (case, "audio of feed", i)
            assert np.array_equal(got["sink"][i], want["sink"][i]), (case, "sink stream of feed", i)
            g, w = got["states"][i], want["states"][i]
            assert all(g[k] == w[k] for k in ("sum", "peak", "count", "sq_state", "locked", "lock_cnt")), (case, "feed", i, g, w)
            assert np.array_equal(g["bits"], w["bits"]), (case, "feed", i, g["bits"], w["bits"])
