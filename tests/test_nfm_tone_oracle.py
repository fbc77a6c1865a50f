"""The C restatement of NFMDemod::feed with m_ctcssOn (tests/nfm_tone_oracle.c, the checker of sdrx_nfm_create_ex) against the
reference's own NCO, Interpolator, PhaseDiscriminators, MovingAverageUtil, DoubleBufferFIFO, Bandpass, Lowpass and
CTCSSDetector: every case of tests/nfm_tone_cases.py recorded by tests/golden/make_golden_nfm_tone.py into
tests/golden/nfm_tone_golden.npz (audio counts of every feed, audio bit for bit or its sha256, levels, squelch state, every
change of m_ctcssIndex, the detector's final state, powers and design).  The probe counters of the oracle show that each case
reaches the branch it is named after.  Where the reference tree and Qt are present, a `ref` test rebuilds the recorder and
compares 100 random configurations sample for sample."""
import hashlib
import os

import numpy as np
import pytest

from tests import nfm_cases as nc
from tests import nfm_tone_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "nfm_tone_golden.npz")
REF = "/root/reference"
BY = {c["name"]: c for c in tc.CASES}


@pytest.fixture(scope="module")
def oracle():
    return tc.build_oracle()


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def runs(oracle):
    """every case through the oracle once, shared by the tests below"""
    return {c["name"]: tc.run_oracle(oracle, c) for c in tc.CASES}


def test_golden_covers_every_case(golden):
    assert {k.split("/")[0] for k in golden.files} == {c["name"] for c in tc.CASES}


@pytest.mark.parametrize("case", tc.CASES, ids=[c["name"] for c in tc.CASES])
def test_oracle_matches_reference_recording(runs, golden, oracle, case):
    name = case["name"]
    r = runs[name]
    assert [f.size for f in r["feeds"]] == golden[f"{name}/counts"].tolist()
    audio = np.concatenate(r["feeds"])
    if f"{name}/audio" in golden.files:
        assert np.array_equal(audio, golden[f"{name}/audio"])
    else:
        assert hashlib.sha256(audio.tobytes()).hexdigest() == str(golden[f"{name}/sha256"])
    m, s, p = golden[f"{name}/levels"].tolist()
    cnt, op, st = golden[f"{name}/state"].tolist()
    assert (r["magsq"], r["sum"], r["peak"], r["count"], int(r["open"]), r["state"]) == (m, s, p, cnt, op, st)
    assert tc.all_events(r) == [tuple(e) for e in golden[f"{name}/events"].tolist()]
    index, changes, blocks, det, mi, N, rate = golden[f"{name}/tone"].tolist()
    assert (r["index"], r["changes"], r["blocks"], int(r["detected"]), r["max_index"]) == (index, changes, blocks, det, mi)
    assert np.array_equal(r["power"].view(np.uint32), golden[f"{name}/power"].view(np.uint32))
    o = tc.OracleNfmTone(oracle, case["cfg"])
    gN, grate, coef, _lp = o.design()
    assert (gN, grate) == (N, rate) == (case["cfg"][2] // 16, case["cfg"][2] // 8)
    assert np.array_equal(coef.view(np.uint32), golden[f"{name}/coef"].view(np.uint32))
    # the AFSquelch as the constructor configures it, bit for bit; never called without m_deltaSquelch: closed, counter 0
    an, tones, acoef, th = o.af_design()
    want = golden[f"{name}/af"]
    assert np.array_equal(np.array([an, *tones, *acoef, th]).view(np.uint64), want[:6].view(np.uint64)), (an, tones, acoef, th, want)
    assert an == case["cfg"][2] // 2000 and tones[0] == 1000.0 and tones[1] == min(6000.0, 0.4 * case["cfg"][2])
    # the AFSquelch's state: isOpen and counter, m_afSquelchOpen, the two sums as bit patterns (all zero without m_deltaSquelch)
    assert want[6] == 1000.0 * (r["af_count"] >= 200) + r["af_count"] and bool(want[7]) == r["af_open"], (want, r["af_open"], r["af_count"])
    assert np.array_equal(r["af_sums"].view(np.uint64), want[8:10].view(np.uint64)), (r["af_sums"], want)
    if not case["cfg"][12]:
        assert th == 0.0 and not want[6:].any()
    else:
        assert np.float32(th) == np.float32(-case["cfg"][7] / 1000.0) == np.float32(o.level())


def test_every_case_reaches_its_branch(runs):
    p = {name: r["probe"] for name, r in runs.items()}
    ev = {name: tc.all_events(r) for name, r in runs.items()}
    audio = {name: np.concatenate(r["feeds"]) for name, r in runs.items()}
    # selected and present: silent up to the first block end, audible after it
    a, (at, idx) = audio["tone_selected"], ev["tone_selected"][0]
    assert idx == 12 and not a[: at + 1].any() and np.count_nonzero(a[at + 1:]) > 10000 and p["tone_selected"]["mismatch"] > 3000
    assert len(ev["tone_selected"]) == 1 and p["tone_selected"]["detections"] == p["tone_selected"]["blocks"] == 4
    # another one selected: silent throughout, the index is reported all the same
    assert not audio["tone_other_selected"].any() and ev["tone_other_selected"] == ev["tone_selected"] and runs["tone_other_selected"]["index"] == 12
    assert p["tone_other_selected"]["mismatch"] == p["tone_other_selected"]["open"] > 15000
    assert p["tone_any"]["mismatch"] == 0 and runs["tone_any"]["index"] == 12 and np.count_nonzero(audio["tone_any"]) > 15000
    # no tone: blocks end below the threshold
    assert p["no_tone"]["blocks"] == 4 and p["no_tone"]["detections"] == 0 and not ev["no_tone"] and not audio["no_tone"].any()
    assert [i for _, i in ev["tone_removed"]] == [12, 0] and p["tone_removed"]["chg_block"] == 2 and 0 < p["tone_removed"]["detections"] < p["tone_removed"]["blocks"]
    g = p["carrier_gap"]
    assert g["chg_close"] == 1 and g["transitions"] == 3 and [i for _, i in ev["carrier_gap"]] == [12, 0, 12], (g, ev["carrier_gap"])
    # the gap falls inside a block: the detector's samples before it count towards the block that ends after it
    close_at, back_at = ev["carrier_gap"][1][0], ev["carrier_gap"][2][0]
    assert (close_at - ev["carrier_gap"][0][0]) % 4000 != 0 and back_at - close_at < 4000
    assert [i for _, i in ev["neighbour_tones"]] == [12, 13] and runs["neighbour_tones"]["max_index"] == 12
    first = int(np.flatnonzero(audio["neighbour_tones"])[0])
    assert first > ev["neighbour_tones"][1][0] and p["neighbour_tones"]["mismatch"] > 15000
    m = p["tone_muted"]
    assert m["blocks"] == m["det_samples"] == m["open"] == 0 and runs["tone_muted"]["open"] and not audio["tone_muted"].any()
    assert runs["rate48k_tone32"]["index"] == 32 and runs["rate48k_tone32"]["blocks"] == 2 and np.count_nonzero(audio["rate48k_tone32"]) > 20000
    assert runs["rate48k_tone1_other"]["index"] == 1 and not audio["rate48k_tone1_other"].any()


def test_every_af_case_reaches_its_branch(runs):
    """8000 Hz: AF block 5 samples, warm-up 600 blocks = 3000 samples, two evaluates per block from then on, Z = 800"""
    p = {name: r["probe"] for name, r in runs.items() if name.startswith("af_")}
    audio = {name: np.concatenate(runs[name]["feeds"]) for name in p}
    assert len(p) == 9
    for name, q in p.items():
        n = runs[name]["count"]
        assert q["af_block_ends"] == n // 5 and q["af_second_eval"] == n // 5 - 600, (name, q)
    for name in (n for n in runs if not n.startswith("af_")):
        assert runs[name]["probe"]["af_block_ends"] == 0 and not runs[name]["af_sums"].any()        # never called without the option
    o = p["af_1k_opens"]
    first = int(np.flatnonzero(audio["af_1k_opens"])[0])
    # 1 kHz opens after the attack of 200 evaluates (one per block, all inside the warm-up) plus the squelch gate; nothing is zeroed
    assert runs["af_1k_opens"]["af_open"] and runs["af_1k_opens"]["af_count"] == 200 and o["af_zero_events"] == 0 and 3000 <= first < 3300, (o, first)
    c = p["af_noise_closed"]
    assert c["af_zero_events"] == c["af_second_eval"] > 3000 and not audio["af_noise_closed"].any() and not runs["af_noise_closed"]["af_open"]
    lt, gt = p["af_sig_noise_sig_gate_lt_z"], p["af_sig_noise_sig_gate_gt_z"]
    assert tc.nc.gate_samples(BY["af_sig_noise_sig_gate_lt_z"]["cfg"]) == 80 < 800 < tc.nc.gate_samples(BY["af_sig_noise_sig_gate_gt_z"]["cfg"]) == 960
    assert 0 < lt["af_zeroed_reads"] < 80 and gt["af_zeroed_reads"] == 799 and lt["transitions"] >= 3 and gt["transitions"] >= 3, (lt, gt)
    lap = p["af_lap"]
    assert runs["af_lap"]["count"] > 24000 and lap["af_zeroed_reads"] > 0 and lap["af_other_copy"] > 0, lap
    g = p["af_gate_24000"]
    assert tc.nc.gate_samples(BY["af_gate_24000"]["cfg"]) == 24000 and g["open"] > 5000 and np.count_nonzero(audio["af_gate_24000"]) > 5000, g
    z = p["af_all_zero"]
    assert z["af_max_zero"] == z["af_block_ends"] + z["af_second_eval"] and runs["af_all_zero"]["af_count"] == 0 and not runs["af_all_zero"]["af_sums"].any()
    s = p["af_threshold_straddled"]
    assert 200 < s["af_zero_events"] < s["af_second_eval"] - 200, s                     # both outcomes, many times each
    b = p["af_and_ctcss"]
    assert b["af_zero_events"] > 0 and b["blocks"] >= 2 and runs["af_and_ctcss"]["index"] == 12 and b["mismatch"] > 0 and b["chg_close"] >= 1, b
    assert np.count_nonzero(audio["af_and_ctcss"]) > 5000


def test_cuts_fall_where_the_case_says(oracle):
    """cuts_block_ends: the detector's blocks end at CUT_ENDS; one inside a feed, one on a feed's last sample, one on the first
    sample of a one-sample feed, one after eleven feeds with feeds of 0, 1 and 5 samples among them"""
    case = BY["cuts_block_ends"]
    o = tc.OracleNfmTone(oracle, case["cfg"])
    ends, pos, feeds_of_block = [], 0, {}
    blocks = 0
    for x in tc.cut(tc.inputs(case), case["splits"]):
        # sample by sample: where does the block count go up
        for k in range(x.size // 2):
            o.feed(x[2 * k: 2 * k + 2])
            b = o.powers()[3]
            if b != blocks:
                ends.append(pos + k); blocks = b
        feeds_of_block[blocks] = feeds_of_block.get(blocks, 0) + 1
        pos += x.size // 2
    assert tuple(ends) == tc.CUT_ENDS
    cum = np.cumsum(case["splits"]).tolist()
    assert not any(c - 1 == tc.CUT_ENDS[0] or c == tc.CUT_ENDS[0] for c in cum)            # inside a feed
    assert tc.CUT_ENDS[1] + 1 in cum                                                        # a feed's last sample
    k = cum.index(tc.CUT_ENDS[2])                                                           # the first sample of the next feed ...
    assert case["splits"][k + 1] == 1                                                       # ... which has that sample alone
    assert feeds_of_block[3] >= 11 and {0, 1, 5} <= set(case["splits"][k + 2: k + 14])      # block 4 is spread over these


def test_splits_do_not_change_the_stream(runs):
    a, b = runs["cuts_block_ends"], runs["cuts_one_feed"]
    assert np.array_equal(np.concatenate(a["feeds"]), np.concatenate(b["feeds"]))
    assert tc.all_events(a) == tc.all_events(b) and (a["index"], a["changes"], a["blocks"]) == (b["index"], b["changes"], b["blocks"])
    assert np.array_equal(a["power"].view(np.uint32), b["power"].view(np.uint32))


def test_ctcss_off_and_any_tone_equal_the_plain_oracle(oracle):
    """independent of the extension: with m_ctcssOn off, and with it on and no tone selected, the audio is tests/nfm_oracle.c's"""
    plain = nc.build_oracle()
    for name in ("tone_any", "carrier_gap", "rate48k_tone32"):
        case = BY[name]
        want = np.concatenate([f for f in _plain_feeds(plain, case)])
        for on, index in ((0, 0), (0, 7), (1, 0)):
            c = dict(case, cfg=case["cfg"][:10] + (on, index))
            got = tc.run_oracle(oracle, c)
            assert np.array_equal(np.concatenate(got["feeds"]), want), (name, on, index)
            assert got["blocks"] == 0 if not on else got["blocks"] > 0


def _plain_feeds(plain, case):
    o = nc.OracleNfm(plain, case["cfg"][:10])
    return [o.feed(x) for x in tc.cut(tc.inputs(case), case["splits"])]


def test_random_cases_cover_the_branches(oracle):
    probes = [tc.run_oracle(oracle, case)["probe"] for case in tc.random_cases()]
    count = {k: sum(p[k] > 0 for p in probes) for k in ("open", "blocks", "detections", "chg_block", "chg_close", "mismatch")}
    print(count)
    assert count["blocks"] >= 50 and count["detections"] >= 40 and count["chg_close"] >= 8 and count["mismatch"] >= 30, count
    af = {k: sum(p[k] > 0 for p in probes) for k in tc.AF_PROBES}
    print(af)
    assert af["af_block_ends"] >= 25 and af["af_zero_events"] >= 15 and af["af_zeroed_reads"] >= 5, af


@pytest.mark.ref
@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "sdrbase", "dsp")), reason="no reference tree here")
def test_oracle_vs_rebuilt_recorder_random(oracle):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_golden_nfm_tone as mg
    if not mg.available(REF):
        pytest.skip("Qt headers not available")
    exe = mg.build_recorder(REF)
    cases = tc.random_cases()
    assert len(cases) == 100
    for case in cases:
        want = mg.record(exe, case["cfg"], tc.inputs(case), case["splits"])
        got = tc.run_oracle(oracle, case)
        assert [f.size for f in got["feeds"]] == [f.size for f in want["feeds"]], case
        for g, w in zip(got["feeds"], want["feeds"]):
            assert np.array_equal(g, w), case
        assert (got["magsq"], got["sum"], got["peak"], got["count"], got["open"], got["state"]) == \
               (want["magsq"], want["sum"], want["peak"], want["count"], want["open"], want["state"]), case
        assert tc.all_events(got) == want["events"], case
        assert (got["index"], got["changes"], got["blocks"], got["detected"], got["max_index"]) == \
               (want["index"], want["changes"], want["blocks"], want["detected"], want["max_index"]), case
        assert np.array_equal(got["power"].view(np.uint32), want["power"].view(np.uint32)), case
        assert np.array_equal(got["af_sums"].view(np.uint64), want["af"][8:10].view(np.uint64)) and bool(want["af"][7]) == got["af_open"], case
        assert want["af"][6] == 1000.0 * (got["af_count"] >= 200) + got["af_count"], case
