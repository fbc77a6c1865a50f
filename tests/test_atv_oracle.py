"""CPU: tests/atv_oracle.cpp, the scalar restatement of ATVDemod::feed that the GPU tests of tests/test_atv_gpu.py compare the bank
with.

Without the reference: the oracle equals the recording tests/golden/atv_golden.npz (made by tests/golden/make_golden_atv.py from
the reference's own ATVDemod class) for every case and every feed -- the design integers, the render events, the stored frames,
the screens, the scope stream and the state's 28 words, frames, screens and scope as bytes for the short cases and as sha256 for
the long ones; fed whole it equals itself fed by a case's cuts; and the cases reach every branch of the issue's list, asserted on
the oracle's counters.

With the reference (`ref`): the recorder is built and run on every case, and the oracle equals it feed by feed."""
import os
import sys

import numpy as np
import pytest

from tests import atv_cases as ac

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_golden_atv as mk  # noqa: E402

REF = "/root/reference"


@pytest.fixture(scope="module")
def oracle():
    return ac.build_oracle()


@pytest.fixture(scope="module")
def gold():
    g = np.load(ac.GOLDEN)
    return {k: g[k] for k in g.files}


@pytest.fixture(scope="module")
def runs(oracle):
    """every case through the oracle with its own cuts, once"""
    return {c["name"]: ac.run_oracle(oracle, c) for c in ac.CASES}


@pytest.mark.parametrize("case", ac.CASES, ids=[c["name"] for c in ac.CASES])
def test_oracle_equals_the_recording(runs, gold, case):
    name = case["name"]
    assert ac.sha(ac.inputs(case)) == str(gold[name + "/in_sha256"])
    got = runs[name]
    assert got["design"] == gold[name + "/design"].tolist()
    feeds = got["feeds"]
    assert [f["events"].size for f in feeds] == gold[name + "/event_counts"].tolist()
    assert np.array_equal(np.concatenate([f["events"] for f in feeds]), gold[name + "/events"])
    assert [len(f["frames"]) for f in feeds] == gold[name + "/frame_counts"].tolist()
    assert [f["scope"].size for f in feeds] == gold[name + "/scope_counts"].tolist()
    for i, f in enumerate(feeds):
        assert f["state"] == gold[name + "/state"][i].tolist(), (name, "feed", i)
    frames = [fr for f in feeds for fr in f["frames"]]
    if case["n"] <= mk.FULL:
        assert np.array_equal(np.array(frames, np.uint8).reshape(gold[name + "/frames"].shape), gold[name + "/frames"])
        assert np.array_equal(np.array([f["screen"] for f in feeds]), gold[name + "/screens"])
        assert np.array_equal(np.concatenate([f["scope"] for f in feeds]), gold[name + "/scope"])
    else:
        assert ([ac.sha(fr) for fr in frames] or [""]) == gold[name + "/frames_sha256"].tolist()
        assert [ac.sha(f["screen"]) for f in feeds] == gold[name + "/screens_sha256"].tolist()
        assert [ac.sha(f["scope"]) for f in feeds] == gold[name + "/scope_sha256"].tolist()
        assert np.array_equal(feeds[-1]["screen"], gold[name + "/last_screen"])


def test_the_recording_has_every_case(gold):
    assert {k.split("/")[0] for k in gold} == {c["name"] for c in ac.CASES}


@pytest.mark.parametrize("case", ac.CASES, ids=[c["name"] for c in ac.CASES])
def test_fed_whole_equals_fed_by_the_cuts(oracle, runs, case):
    whole = ac.run_oracle(oracle, case, splits=[case["n"]])["feeds"][0]
    m = ac.merged(runs[case["name"]]["feeds"], case["splits"])
    assert np.array_equal(m["events"], whole["events"]) and np.array_equal(m["scope"], whole["scope"])
    assert np.array_equal(m["screen"], whole["screen"]) and m["state"] == whole["state"]


def test_the_cases_reach_every_branch(runs):
    total = ac.assert_coverage([r["hits"] for r in runs.values()])
    print(total)
    # more renders in one feed than a frames_cap of 1, and renders twice within one line
    r = runs["rearmed_vsync"]
    assert ac.BY_NAME["rearmed_vsync"]["cfg"]["frames_cap"] == 1 and max(f["events"].size for f in r["feeds"]) > 1
    assert r["hits"]["max_renders_in_line"] >= 2
    # what the list of cases is meant to hold
    mods = {(c["cfg"]["modulation"], c["cfg"]["standard"] == ac.HSKIP) for c in ac.CASES}
    assert mods >= {(m, h) for m in (ac.FM1, ac.FM2, ac.FM3, ac.AM) for h in (False, True)}
    assert {c["cfg"]["standard"] for c in ac.CASES} == set(range(6))
    assert {(c["cfg"]["hsync"], c["cfg"]["vsync"]) for c in ac.CASES} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert {c["cfg"]["fm_deviation"] for c in ac.CASES} >= {0.5, 1.0, 2.0}
    assert any(c["cfg"]["invert_video"] for c in ac.CASES) and any(c["cfg"]["nco_freq"] for c in ac.CASES) and any(c["cfg"]["n_lines"] == 625 for c in ac.CASES)
    assert {c["sig"]["kind"] for c in ac.CASES} == {"video", "noise", "const", "zero"}


def test_nan_reaches_the_state_as_the_x86_default_nan(runs):
    """all-zero input under FM1: the normalised sample is 0 / 0, the buffers and the line average hold 0xffc00000, the grey is 0"""
    last = runs["zeros_fm1"]["feeds"][-1]
    words = dict(zip(ac.STATE_INTS + ac.STATE_BITS, last["state"]))
    assert words["amp_line_average"] == 0xFFC00000 and last["state"][16] == last["state"][22] == 0xFFC00000
    assert not last["screen"].any() and not last["scope"].any()


def test_refusals(oracle):
    import ctypes as C
    for kw in (dict(modulation=ac.USB), dict(modulation=ac.LSB), dict(level_black=1.0), dict(n_lines=1, frames_per_s=0.5), dict(n_lines=4),
               dict(line_duration=0.0), dict(in_rate=0), dict(frames_cap=0)):
        s = ac.as_struct(ac.cfg(**kw))
        assert not oracle.ato_create(C.byref(s)), kw


# ---------------------------------------------------------------- against the reference
ref = pytest.mark.skipif(not mk.available(REF), reason="reference tree, moc or Qt not present")


@pytest.fixture(scope="module")
def recorder():
    return mk.build_recorder(REF)


@ref
@pytest.mark.ref
def test_oracle_equals_the_recorder_on_every_case(runs, recorder):
    for case in ac.CASES:
        r = mk.record(recorder, case, ac.inputs(case))
        got = runs[case["name"]]
        assert got["design"] == r["design"], case["name"]
        for i, (g, w) in enumerate(zip(got["feeds"], r["feeds"])):
            what = (case["name"], "feed", i)
            assert np.array_equal(g["events"], w["events"]), what
            assert len(g["frames"]) == len(w["frames"]) and all(np.array_equal(a, b) for a, b in zip(g["frames"], w["frames"])), what
            assert np.array_equal(g["screen"], w["screen"]) and np.array_equal(g["scope"], w["scope"]), what
            assert g["state"] == w["state"], what
