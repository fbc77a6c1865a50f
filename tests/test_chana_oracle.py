"""The C restatement of ChannelAnalyzer::feed (tests/chana_oracle.c, the checker of the GPU analyzer bank) against the reference's
own NCOF, Interpolator, fftfilt and fftcorr: every case of tests/chana_cases.py recorded by tests/golden/make_golden_chana.py
into tests/golden/chana_golden.npz (the Sample count of every feed, the Sample stream bit for bit or its sha256, m_magsq and
m_undersampleCount).  Where the reference tree and Qt are present, a `ref` test rebuilds the recorder and compares three cases
cut differently sample for sample."""
import hashlib
import os

import numpy as np
import pytest

from tests import chana_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "chana_golden.npz")
REF = "/root/reference"
BY = {c["name"]: c for c in cc.CASES}


@pytest.fixture(scope="module")
def oracle():
    return cc.build_oracle()


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def runs(oracle):
    """every case through the oracle once, shared by the tests below"""
    return {c["name"]: cc.run_oracle(oracle, c) for c in cc.CASES}


def _cat(parts):
    return np.concatenate(parts) if parts else np.zeros((0, 2), np.int16)


def test_golden_covers_every_case(golden):
    assert {k.split("/")[0] for k in golden.files} == {c["name"] for c in cc.CASES}


@pytest.mark.parametrize("case", cc.CASES, ids=[c["name"] for c in cc.CASES])
def test_oracle_matches_reference_recording(runs, golden, case):
    name = case["name"]
    r = runs[name]
    assert [a.shape[0] for a in r["out"]] == golden[f"{name}/counts"].tolist()
    full = _cat(r["out"])
    if f"{name}/out" in golden.files:
        want = golden[f"{name}/out"]
        assert full.shape == want.shape and np.array_equal(full, want), (name, int(np.count_nonzero(full != want)))
    else:
        assert hashlib.sha256(np.ascontiguousarray(full).tobytes()).hexdigest() == str(golden[f"{name}/out_sha256"]), name
    assert r["magsq"] == golden[f"{name}/magsq"][0], name
    assert r["state"][0] == int(golden[f"{name}/usc"][0]), name


def test_cases_reach_what_they_are_named_after(runs):
    # the first Sample is a group of one; later groups are full
    for name, per in (("span1", 2), ("span3", 8), ("span8", 256)):
        n_filtered = runs[name]["state"][3]
        assert sum(a.shape[0] for a in runs[name]["out"]) == (n_filtered + per - 1) // per, name
    # a group stays open across feeds that emit nothing, and across feeds that emit blocks
    assert [a.shape[0] for a in runs["span8"]["out"]].count(0) >= 3
    # the swap: LSB through a negative bandwidth differs from the same configuration without the swap only in the order
    assert np.array_equal(_cat(runs["dsb_default"]["out"]), _cat(runs["dsb_negative_bandwidth"]["out"]))
    assert not np.array_equal(_cat(runs["dsb_default"]["out"]), _cat(runs["down_step1"]["out"]))       # bypass beside the Interpolator at step 1
    assert _cat(runs["band_clamp"]["out"]).any() and _cat(runs["band_reject"]["out"]).any()
    # applySettings' own root raised cosine on a negative bandwidth passes nothing
    assert not _cat(runs["down_rrc_negative"]["out"]).any()
    # NCOF's increment: a fraction, so the float phase rounds on the way
    assert runs["nco_fractional"]["design"][3] != int(runs["nco_fractional"]["design"][3])
    assert len({_cat(runs[f"rrc_{a}"]["out"]).tobytes() for a in (0, 35, 100)}) == 3


@pytest.mark.parametrize("name", [c["name"] for c in cc.CASES if c["cfg"]["input_type"] == cc.AUTOCORR])
def test_autocorrelation_regimes(runs, name):
    full = _cat(runs[name]["out"]).astype(np.int64)
    per = 1 << BY[name]["cfg"]["span_log2"]
    assert runs[name]["state"][2] == 2 and 0 < runs[name]["state"][1] < 4096, runs[name]["state"]      # two blocks done, the third is open
    assert full.shape[0] > 2 * 4096 and not full[:4095].any()              # P_0 = 0: the first 4095 calls return zeros
    assert full[4095:].any()
    assert full.shape[0] == (runs[name]["state"][3] + per - 1) // per
    if "quiet" in name:
        # in range: nothing saturates, nothing wraps (lag 0 is the largest magnitude of a block)
        assert 0 < np.abs(full).max() < 32767 and np.count_nonzero(full[4095:]) > 1000, name
    if "loud" in name:
        # out of range: (qint16) of a float beyond int32 is 0x8000 0000's low half, 0; beyond int16 it wraps
        assert np.abs(full).max() >= 32767, name


@pytest.mark.parametrize("name", ["usb", "down_96k_37k", "corr_lsb_loud"])
def test_one_feed_equals_the_case_splits(oracle, runs, name):
    one = cc.run_oracle(oracle, BY[name], splits=[BY[name]["n"]])
    assert np.array_equal(_cat(one["out"]), _cat(runs[name]["out"])) and one["magsq"] == runs[name]["magsq"]


def test_seek_moves_the_counters_only(oracle):
    """past 2^31 filtered samples: the mask sees the counter's low bits, fftcorr's call counter follows the groups"""
    case = BY["corr_span2"]
    o = cc.OracleChana(oracle, case["cfg"])
    pos = (1 << 31) + 4 * 4000 + 2                   # the open group holds two samples, 4001 calls into a block (rounded up: 4001)
    o.seek(pos)
    assert o.state()[:2] == (pos & 0xFFFFFFFF, 4001)
    out = o.feed(cc.inputs(case)[: 2 * 2048])        # 2048 filtered samples: groups close at samples 2, 6, ...
    assert out.shape[0] == 512 and o.state()[1] == (4001 + 512) % 4096 and o.state()[2] == 1


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "sdrbase", "dsp")), reason="reference tree not present")
def test_ref_recorder_on_other_splits(oracle):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_golden_chana as mg
    if not mg.available(REF):
        pytest.skip("Qt headers not present")
    exe = mg.build_recorder(REF)
    for name, splits in (("nco_negative", [4396]), ("down_96k_37k", [7, 4000, 3993]), ("corr_dsb_loud", [5000, 4316])):
        case = BY[name]
        assert sum(splits) == case["n"]
        want = mg.record(exe, case["cfg"], cc.inputs(case), splits)
        got = cc.run_oracle(oracle, case, splits=splits)
        assert all(np.array_equal(g, w) for g, w in zip(got["out"], want["out"])) and got["magsq"] == want["magsq"], name
