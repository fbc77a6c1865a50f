"""The C restatement of UDPSrc::feed for the SSB formats 4 .. 7 (tests/udpsrc_ssb_oracle.c, the checker of the GPU bank, with its
own 512-point g_fft network: bitrevR2, the radix-4 stage bfR4, two radix-8 stages) against the reference's own fftfilt, g_fft,
MagAGC, MovingAverage, NCO and Interpolator: every case of tests/udpsrc_ssb_cases.py recorded by
tests/golden/make_golden_udpsrc_ssb.py into tests/golden/udpsrc_ssb_golden.npz -- counts of every feed, payload bytes and
spectrum Samples bit for bit or their sha256, m_inMagsq, the squelch state with gate and release, fftfilt's inptr and the filter
design.  The probe counters show that each case reaches what it is named after.  Where the reference tree and Qt are present, a
`ref` test rebuilds the recorder and compares 50 random configurations element for element."""
import hashlib
import os

import numpy as np
import pytest

from tests import udpsrc_ssb_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "udpsrc_ssb_golden.npz")
REF = "/root/reference"


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


def test_golden_covers_every_case_and_format(golden):
    assert {k.split("/")[0] for k in golden.files} - {"filter"} == {c["name"] for c in sc.CASES}
    assert {(c["cfg"][3], c["cfg"][10]) for c in sc.CASES} == {(f, a) for f in sc.FORMATS for a in (0, 1)}


@pytest.mark.parametrize("case", sc.CASES, ids=[c["name"] for c in sc.CASES])
def test_oracle_matches_reference_recording(runs, golden, case):
    name, fmt = case["name"], case["cfg"][3]
    r = runs[name]
    assert [[s.shape[0], f.shape[0]] for s, f in zip(r["specs"], r["feeds"])] == golden[f"{name}/counts"].tolist()
    for key, got in (("payload", np.concatenate(r["feeds"])), ("spectrum", np.concatenate(r["specs"]))):
        if f"{name}/{key}" in golden.files:
            want = golden[f"{name}/{key}"]
            assert got.dtype == want.dtype and np.array_equal(got, want), key
        else:
            assert hashlib.sha256(np.ascontiguousarray(got).tobytes()).hexdigest() == str(golden[f"{name}/{key}_sha256"]), key
    assert r["in_magsq"] == float(golden[f"{name}/in_magsq"][0])
    assert [int(r["open"]), r["open_count"], r["close_count"], r["design"]["gate"], r["design"]["release"], r["pending"]] == golden[f"{name}/state"].tolist()
    assert r["total"] == int(golden[f"{name}/counts"][:, 1].sum()) and r["resampled"] == int(golden[f"{name}/counts"][:, 0].sum())
    # the design the reference built from its default settings, whatever this case's bandwidth and rate are (item 1)
    assert np.array_equal(r["filter"].view(np.uint32), golden["filter"].view(np.uint32))


def test_the_filter_is_a_low_pass_at_6250_of_48000(runs):
    h = runs["lsb_burst"]["filter"].view(np.complex64)
    mag = np.abs(h)
    assert mag[:256].max() == pytest.approx(1.0, abs=1e-6) and mag[:60].min() > 0.9 and mag[80:256].max() < 1e-3      # 6250 / 48000 * 512 = 66.7


def test_payload_counts_follow_the_schedule(runs):
    """format 4: one raw element per resampled sample plus 256 per block; formats 5 .. 7: the blocks only"""
    for name, r in runs.items():
        fmt, pend = sc.BY[name]["cfg"][3], 0
        for s, f, st in zip(r["specs"], r["feeds"], r["states"]):
            k = s.shape[0]
            nb = (pend + k) // 256
            assert f.shape[0] == (k if fmt == sc.LSB else 0) + 256 * nb, name
            pend = (pend + k) % 256
            assert st["pending"] == pend, name
        assert r["blocks"] == r["resampled"] // 256, name


def test_cases_cover_what_they_claim(runs):
    p = {name: r["probe"] for name, r in runs.items()}
    for name in ("lsb_burst", "usb_burst", "lsbmono_burst_gate0", "usbmono_burst"):        # item 8: flips inside blocks, both ways
        m = np.concatenate(runs[name]["masks"])
        flips = np.flatnonzero(np.diff(m.astype(np.int8)))
        ups, downs = [i + 1 for i in flips if m[i + 1]], [i + 1 for i in flips if not m[i + 1]]
        assert ups and downs and all(i % 256 for i in ups + downs), (name, ups, downs)
        assert 0 < p[name]["blocks_open"] < p[name]["blocks"] and p[name]["flips_in_block"] >= 2, (name, p[name])
    assert runs["lsbmono_burst_gate0"]["design"] == {"gate": 400, "release": 0}                  # item 7
    assert runs["usbmono_burst"]["design"] == {"gate": 400, "release": 160}
    assert runs["usbmono_agc_float_rate"]["design"] == {"gate": 551, "release": 551}
    assert runs["usb_wild_settings"]["design"]["gate"] == 2400
    for name in ("lsb_gain_wraps", "usbmono_gain_wraps"):
        assert p[name]["wraps"] > 100 and p[name]["past_int32"] == 0, (name, p[name])
    for name in ("usb_gain_past_int32", "lsbmono_gain_past_int32"):
        assert p[name]["past_int32"] > 100, (name, p[name])
    # item 11: the factor is inf while MagAGC holds and ramps (1360 samples and more here) and 0.0 afterwards: all five blocks are NaN,
    # four of them with the squelch open, and the payload is 0 throughout
    for name in ("usb_agc_silence", "lsb_agc_silence"):
        assert p[name]["nan_blocks"] == p[name]["blocks"] == 5 and p[name]["blocks_open"] == 4 and not np.concatenate(runs[name]["feeds"]).any(), (name, p[name])
    assert p["lsbmono_silence"]["nan_blocks"] == 0
    for name in ("lsb_feed_yields", "usbmono_feed_yields"):
        assert [s.shape[0] for s in runs[name]["specs"]][: len(sc.YIELDS)] == sc.YIELDS, name
    # item 9: feed boundaries of the interleave case fall mid-block, once exactly on a block's last sample
    pend = [st["pending"] for st in runs["lsb_interleave"]["states"]]
    assert pend[:5] == [100, 144, 44, 45, 44] and 0 in [st["pending"] for st in runs["lsb_feed_yields"]["states"]][3:]
    # the AGC moves the payload: same case with the flag off differs (item 6), and AGC cases are not silent
    for name in ("lsb_agc_cross", "usb_agc_squelched", "lsbmono_agc", "usbmono_agc_float_rate"):
        assert np.concatenate(runs[name]["feeds"]).any(), name


def test_format_4_is_blocks_interleaved_with_raw_iq(oracle):
    """item 9: format 4's stream is format 5's LSB twin cut into blocks, each right in front of the raw element of the sample that
    completed it, and the raw elements are format 0's samples"""
    from tests import udpsrc_cases as uc
    case = sc.BY["lsb_interleave"]
    x = sc.inputs(case)
    got = np.concatenate(sc.run_oracle(oracle, case)["feeds"])
    raw = uc.OracleUdp(uc.build_oracle(), case["cfg"][:3] + (0,) + case["cfg"][4:]).feed(x)[0]
    k = raw.shape[0]
    pos = np.arange(k) + 256 * ((np.arange(k) + 1) // 256)
    # (the disabled squelch opens behind a gate of 400 samples here and of 80 in format 0)
    assert got.shape[0] == k + 256 * (k // 256) and np.array_equal(got[pos][401:], raw[401:]) and raw[401:].any() and not got[pos][:400].any()
    mono = sc.run_oracle(oracle, dict(case, cfg=case["cfg"][:3] + (sc.LSB_MONO,) + case["cfg"][4:]))
    blocks = np.delete(got, pos, axis=0)
    assert blocks.shape[0] == 256 * (k // 256) == np.concatenate(mono["feeds"]).shape[0] and blocks.any()


def test_agc_flag_reaches_the_filter(oracle):
    case = sc.BY["lsb_agc_cross"]
    off = dict(case, cfg=case["cfg"][:10] + (0,))
    a, b = sc.run_oracle(oracle, case), sc.run_oracle(oracle, off)
    assert not np.array_equal(np.concatenate(a["feeds"]), np.concatenate(b["feeds"]))
    assert all(np.array_equal(x, y) for x, y in zip(a["specs"], b["specs"])) and a["in_magsq"] == b["in_magsq"]     # the unscaled ci


def test_splits_do_not_change_the_stream(oracle, runs):
    for name in ("lsb_interleave", "usbmono_burst"):
        one = sc.run_oracle(oracle, sc.BY[name], splits=[sc.BY[name]["n"]])
        assert np.array_equal(np.concatenate(runs[name]["feeds"]), one["feeds"][0]), name
        assert (runs[name]["pending"], runs[name]["blocks"], runs[name]["in_magsq"]) == (one["pending"], one["blocks"], one["in_magsq"])


def test_random_cases_cover_the_branches(oracle):
    cases = sc.random_cases()
    assert len(cases) == 50 and {c["cfg"][3] for c in cases} == set(sc.FORMATS)
    probes = [sc.run_oracle(oracle, c)["probe"] for c in cases]
    print({k: sum(p[k] > 0 for p in probes) for k in sc.PROBES})
    assert sum(p["blocks_open"] > 0 for p in probes) >= 15 and sum(p["flips_in_block"] > 0 for p in probes) >= 3


@pytest.mark.ref
@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "sdrbase", "dsp")), reason="no reference tree here")
def test_oracle_vs_rebuilt_recorder_random(oracle):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_golden_udpsrc_ssb as mg
    if not mg.available(REF):
        pytest.skip("Qt headers not available")
    exe = mg.build_recorder(REF)
    for case in sc.random_cases():
        want = mg.record(exe, case["cfg"], sc.inputs(case), case["splits"])
        got = sc.run_oracle(oracle, case)
        for g, w, gs, ws in zip(got["feeds"], want["feeds"], got["specs"], want["specs"]):
            assert np.array_equal(g, w) and np.array_equal(gs, ws), case
        assert (got["in_magsq"], got["open"], got["open_count"], got["close_count"], got["pending"], got["design"]["gate"], got["design"]["release"]) == \
               (want["in_magsq"], want["open"], want["open_count"], want["close_count"], want["pending"], want["gate"], want["release"]), case
        assert np.array_equal(got["filter"].view(np.uint32), want["filter"].view(np.uint32)), case
