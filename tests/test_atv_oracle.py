"""CPU: tests/atv_oracle.cpp, the scalar restatement of ATVDemod::feed that the GPU tests of tests/test_atv_gpu.py compare the bank
with.

Without the reference: the oracle equals the recording tests/golden/atv_golden.npz (made by tests/golden/make_golden_atv.py from
the reference's own ATVDemod class) for every case and every feed -- the design integers, the render events, the stored frames,
the screens, the scope stream and the state's 28 words, frames, screens and scope as bytes for the short cases and as sha256 for
the long ones; fed whole it equals itself fed by a case's cuts; and the cases reach every branch of the issue's list, asserted on
the oracle's counters.

The same for the stretch walk's cases (atv_cases.SHAPE_CASES, CUT_STREAMS fed whole, random_cases()) against the digests of
tests/golden/atv_random_golden.npz (make_golden_atv.py --random); the geometry counters (ato_geo) reach GEO_COVERAGE over the FM
classic shape cases and every named case its own counter; the draw keeps its shares of FM classic cases and of tops of 64 samples
or more; every cut 0 .. 130 of the four cut streams, merged, is the stream fed whole.

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


# ---------------------------------------------------------------- the stretch walk's shapes, the cut streams, the random draw
RCASES = ac.golden_random_cases()
RIDS = [c["name"] for c in RCASES]


@pytest.fixture(scope="module")
def rgold():
    return ac.load_random_golden()


@pytest.fixture(scope="module")
def rruns(oracle):
    """every shape case, cut stream and random case through the oracle with its own cuts, once"""
    return {c["name"]: ac.run_oracle(oracle, c) for c in RCASES}


def test_the_random_recording_has_every_case(rgold):
    assert list(rgold) == RIDS


@pytest.mark.parametrize("case", RCASES, ids=RIDS)
def test_oracle_equals_the_random_recording(rruns, rgold, case):
    """the design integers (the line and the top as the case means them), and per feed the events, the state's words and the
    digests of frames, screen and scope: the oracle packed as the recorder's results were"""
    got, want = rruns[case["name"]], rgold[case["name"]]
    k = case["cfg"]
    assert got["design"][:2] == [round(k["line_duration"] * k["in_rate"] - 0.25), round(k["top_duration"] * k["in_rate"] - 0.25)]
    mine = mk.pack_digests([(case, got["feeds"], got["design"], ac.inputs(case))])
    assert np.array_equal(mine["in_sha256"][0], want["in_sha256"]) and np.array_equal(mine["design"][0], want["design"])
    for key in ("event_counts", "events", "frame_counts", "state", "frames_sha256", "screens_sha256", "scope_sha256"):
        assert mine[key].shape == want[key].shape and np.array_equal(mine[key], want[key]), (case["name"], key)


@pytest.mark.parametrize("case", RCASES, ids=RIDS)
def test_shapes_fed_whole_equal_fed_by_the_cuts(oracle, rruns, case):
    whole = ac.run_oracle(oracle, case, splits=[case["n"]])["feeds"][0]
    m = ac.merged(rruns[case["name"]]["feeds"], case["splits"])
    assert np.array_equal(m["events"], whole["events"]) and np.array_equal(m["scope"], whole["scope"])
    assert np.array_equal(m["screen"], whole["screen"]) and m["state"] == whole["state"]


def test_the_shape_cases_reach_the_geometry(rruns):
    """GEO_COVERAGE over the FM classic shape cases, and each named case what it is named for"""
    fm = [c for c in ac.SHAPE_CASES if ac.is_fm_classic(c["cfg"])]
    total = ac.assert_geo_coverage([rruns[c["name"]]["geo"] for c in fm])
    print(total)
    geo = lambda name: rruns[name]["geo"]
    # the tie: at 31 per top the sum equals the level and the vsync fires; one sample either way it does not tie, and with 30 it does not fire
    assert geo("shape_tie_86_31")["vsync_tie"] >= 1 and geo("shape_tie_86_30")["vsync_tie"] == 0 and geo("shape_tie_86_32")["vsync_tie"] == 0
    assert geo("shape_tie_86_30")["vsync_first_col"] == 0 and geo("shape_tie_86_32")["vsync_first_col"] >= 1
    ev = lambda name: np.concatenate([f["events"] + sum(ac.SHAPE_BY_NAME[name]["splits"][:i]) for i, f in enumerate(rruns[name]["feeds"])])
    assert not np.array_equal(ev("shape_tie_86_30"), ev("shape_tie_86_31"))
    for name, key in (("shape_lost_past_line_65", "col_past_line"), ("shape_lost_past_line_129", "col_past_line"), ("shape_lost_vsync_100", "col_past_line"),
                      ("shape_minus150_100", "col_negative"), ("shape_minus150_192", "col_negative"), ("shape_nan_100", "nan_at_check"),
                      ("shape_nan_640", "nan_at_check"), ("shape_nan_129_fm2", "nan_at_check"), ("shape_noise_100_1", "detect_twice_near"),
                      ("shape_noise_100_2", "detect_twice_near"), ("shape_exact_pulse_100", "detect_held"), ("shape_exact_pulse_129", "detect_held"),
                      ("shape_exact_pulse_129", "points_from_far"), ("shape_192_70_fm3", "points_from_far"), ("shape_1000_130_fm2", "points_from_far"),
                      ("shape_no_broad_65", "line_past_frame"), ("shape_no_broad_i_129", "row_stays"), ("shape_pal625_10ms", "points_from_far")):
        assert geo(name)[key] >= 1, (name, key)
    # what the list is meant to hold
    have = {(rruns[c["name"]]["design"][0], rruns[c["name"]]["design"][1]) for c in fm}
    assert have >= set(ac.SHAPES)
    assert {c["cfg"]["modulation"] for c in fm} == {ac.FM1, ac.FM2, ac.FM3} and {c["cfg"]["standard"] for c in fm} == {0, 1, 2, 3, 4}
    assert {(c["cfg"]["hsync"], c["cfg"]["vsync"]) for c in fm} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert all(c["n"] < 50000 for c in ac.SHAPE_CASES if c["name"] != "shape_pal625_10ms")
    pal = ac.SHAPE_BY_NAME["shape_pal625_10ms"]
    assert rruns[pal["name"]]["design"][:2] == [640, 47] and pal["cfg"]["n_lines"] == 625 and pal["n"] >= 700 * 640
    assert sum(f["events"].size for f in rruns[pal["name"]]["feeds"]) >= 2


def test_the_random_draw_stays_with_the_stretch():
    cases = ac.random_cases()
    fm, far = ac.assert_random_shares(cases)
    print(fm, "FM classic,", far, "with a top of 64 samples or more")
    assert all(c["n"] <= 20000 and 3 <= len(c["splits"]) <= 7 and 0 in c["splits"] for c in cases)
    assert {c["cfg"]["modulation"] for c in cases} == {0, 1, 2, 3} and {c["cfg"]["standard"] for c in cases} == set(range(6))
    assert {c["sig"]["kind"] for c in cases} == {"video", "noise", "const", "zero"}
    assert any("lost" in c["sig"] for c in cases) and any(c["sig"].get("amp", 0) > 32768 for c in cases)
    assert sum(c["cfg"]["decimator_enable"] for c in cases) >= 10 and sum(c["cfg"]["fft_filtering"] for c in cases) >= 10
    assert any(abs(c["cfg"]["nco_freq"]) >= c["cfg"]["in_rate"] // 2 - 1 for c in cases)


@pytest.mark.parametrize("case", ac.CUT_STREAMS, ids=[c["name"] for c in ac.CUT_STREAMS])
def test_every_cut_of_the_cut_streams_equals_the_stream_fed_whole(oracle, case):
    """the oracle itself: channel i's feeds (i samples, the rest, the tail's pieces) merged are the stream in one feed"""
    x = ac.inputs(case)
    whole = ac.run_oracle(oracle, case, splits=[case["n"]])
    assert whole["feeds"][0]["events"].size >= 1
    if "tie" in case["name"]:
        assert whole["geo"]["vsync_tie"] >= 1
    for i in range(ac.CUT_CHANNELS):
        spans = ac.cut_spans(case, i)
        m = ac.merged(ac.run_spans(oracle, case["cfg"], ac.cut(x, spans))["feeds"], spans)
        w = whole["feeds"][0]
        assert np.array_equal(m["events"], w["events"]) and np.array_equal(m["scope"], w["scope"]), (case["name"], i)
        assert np.array_equal(m["screen"], w["screen"]) and m["state"] == w["state"], (case["name"], i)


@ref
@pytest.mark.ref
def test_oracle_equals_the_recorder_on_every_shape_and_random_case(rruns, recorder):
    for case in RCASES:
        r = mk.record(recorder, case, ac.inputs(case))
        got = rruns[case["name"]]
        assert got["design"] == r["design"], case["name"]
        assert len(got["feeds"]) == len(r["feeds"])
        for i, (g, w) in enumerate(zip(got["feeds"], r["feeds"])):
            what = (case["name"], "feed", i)
            assert np.array_equal(g["events"], w["events"]), what
            assert len(g["frames"]) == len(w["frames"]) and all(np.array_equal(a, b) for a, b in zip(g["frames"], w["frames"])), what
            assert np.array_equal(g["screen"], w["screen"]) and np.array_equal(g["scope"], w["scope"]), what
            assert g["state"] == w["state"], what
