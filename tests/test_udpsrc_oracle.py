"""The C restatement of UDPSrc::feed (tests/udpsrc_oracle.c, the checker of the GPU bank) against the reference's own NCO,
Interpolator, MagAGC, MovingAverage, PhaseDiscriminators and Bandpass: every case of tests/udpsrc_cases.py recorded by
tests/golden/make_golden_udpsrc.py into tests/golden/udpsrc_golden.npz (sample counts of every feed, payload bytes and spectrum
Samples bit for bit or their sha256, m_inMagsq, final squelch state), all seven formats, the AM formats with the AGC off and on.  The probe counters of the oracle show
that each case reaches the branch it is named after.  Where the reference tree and Qt are present, a `ref` test rebuilds the
recorder and compares 100 random configurations sample for sample."""
import hashlib
import os

import numpy as np
import pytest

from tests import udpsrc_cases as uc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "udpsrc_golden.npz")
REF = "/root/reference"
BY = {c["name"]: c for c in uc.CASES}


@pytest.fixture(scope="module")
def oracle():
    return uc.build_oracle()


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def runs(oracle):
    """every case through the oracle once, shared by the tests below"""
    return {c["name"]: uc.run_oracle(oracle, c) for c in uc.CASES}


def _joined(parts, empty):
    return np.concatenate(parts) if parts else empty


def test_golden_covers_every_case_and_format(golden):
    names = {k.split("/")[0] for k in golden.files}
    assert names == {c["name"] for c in uc.CASES}
    assert {c["cfg"][3] for c in uc.CASES} == set(uc.FORMATS)


@pytest.mark.parametrize("case", uc.CASES, ids=[c["name"] for c in uc.CASES])
def test_oracle_matches_reference_recording(runs, golden, case):
    name, fmt = case["name"], case["cfg"][3]
    r = runs[name]
    assert [f.shape[0] for f in r["feeds"]] == golden[f"{name}/counts"].tolist()
    for key, got in (("payload", _joined(r["feeds"], uc.as_samples(fmt, b""))), ("spectrum", _joined(r["specs"], np.zeros((0, 2), np.int16)))):
        if f"{name}/{key}" in golden.files:
            want = golden[f"{name}/{key}"]
            assert got.dtype == want.dtype and np.array_equal(got, want), key
        else:
            assert hashlib.sha256(np.ascontiguousarray(got).tobytes()).hexdigest() == str(golden[f"{name}/{key}_sha256"]), key
    assert r["in_magsq"] == float(golden[f"{name}/in_magsq"][0])
    assert [int(r["open"]), r["open_count"], r["close_count"]] == golden[f"{name}/state"].tolist()
    assert r["total"] == int(golden[f"{name}/counts"].sum())


def test_cases_cover_what_they_claim():
    for name in ("iq16_burst_gate5", "iq16_burst_gate1", "amnodc_burst", "ambpf_burst", "nfm_burst"):
        for s in (0, 1, 31, 32, 33):
            assert s in BY[name]["splits"], (name, s)
    assert BY["one_long_feed"]["splits"] == [BY["one_long_feed"]["n"]]
    assert [uc.gate_samples(BY[n]["cfg"]) for n in ("iq16_burst_gate5", "iq16_burst_gate1", "iq16_burst_gate0")] == [400, 80, 0]
    # bursts: output-rate runs on both sides of the gate
    for name, runs_in in (("iq16_burst_gate5", uc.BURST_RUNS_5), ("iq16_burst_gate1", uc.BURST_RUNS_1)):
        g = uc.gate_samples(BY[name]["cfg"])
        out_runs = [r // 6 for r in runs_in]
        assert min(out_runs) < g < max(out_runs), name
    # format 2 / 3 cases keep fm_scaling * gain below 8 except the overflowing one at 9.6
    for c in uc.CASES:
        if c["cfg"][3] in (uc.NFM, uc.NFM_MONO):
            v = c["cfg"][2] / (2.0 * c["cfg"][5]) * c["cfg"][6]
            assert (abs(v - 9.6) < 1e-6) if c["name"] == "nfm_overflow_9p6" else v < 8, c["name"]
    # 62500 / 48000 is not dyadic: the resampler schedule of that case is the serial one
    step = np.float32(62500) / np.float32(48000)
    assert all(float(step * np.float32(1 << q)) != np.floor(float(step * np.float32(1 << q))) for q in range(11))


def test_first_output_comes_one_step_in(oracle):
    """m_sampleDistanceRemain starts at in_rate / output_sample_rate: 6 inputs per output from the very first one"""
    o = uc.OracleUdp(oracle, BY["iq16_burst_gate5"]["cfg"])
    assert o.feed(np.zeros(2 * 5, np.int16))[0].shape[0] == 0
    assert o.feed(np.zeros(2, np.int16))[0].shape[0] == 1
    assert o.feed(np.zeros(2 * 5999, np.int16))[0].shape[0] == 999
    o = uc.OracleUdp(oracle, BY["iq16_step1_48k"]["cfg"])
    assert o.feed(np.zeros(2, np.int16))[0].shape[0] == 1


def test_splits_do_not_change_the_stream(runs):
    a, b = runs["splits_edges"], runs["one_long_feed"]
    assert np.array_equal(np.concatenate(a["feeds"]), np.concatenate(b["feeds"]))
    assert np.array_equal(np.concatenate(a["specs"]), np.concatenate(b["specs"]))
    assert (a["in_magsq"], a["open"], a["open_count"], a["close_count"], a["total"]) == (b["in_magsq"], b["open"], b["open_count"], b["close_count"], b["total"])


def test_every_case_reaches_its_branch(runs):
    p = {name: r["probe"] for name, r in runs.items()}
    for name in ("iq16_burst_gate5", "iq16_burst_gate1", "iq24_burst", "nfm_burst", "nfmmono_burst_gate5", "am_burst", "amnodc_burst", "ambpf_burst"):
        assert p[name]["transitions"] >= 4 and p[name]["release_hits"] >= 2, (name, p[name])       # opens and closes twice at least
        assert p[name]["closed_above"] > 0 and p[name]["gate_hits"] > 0 and p[name]["open"] > 1000, (name, p[name])
    assert p["iq16_burst_gate0"]["transitions"] >= 4 and p["iq16_burst_gate0"]["gate_hits"] == 0
    s = p["iq16_short_burst"]
    assert s["open"] == 0 and s["transitions"] == 0 and 200 < s["closed_above"] < 400, s        # above for less than the gate: never opens
    assert p["iq16_squelch_off"]["above_changes"] == 0 and p["iq16_squelch_off"]["open"] > 900
    for name in ("iq16_overflow_gain", "iq24_overflow_gain", "am_overflow_gain", "nfm_overflow_9p6"):
        assert p[name]["conv_wraps"] > 40, (name, p[name])
    for name in ("nfmmono_zero_input", "amnodc_zero_open"):
        assert p[name]["zero_ci"] == runs[name]["total"] == p[name]["open"], (name, p[name])
    for name, r in runs.items():                            # closed samples are zeros in every format
        for f, m in zip(r["feeds"], r["masks"]):
            assert m.size == f.shape[0] and not f[~m].any(), name
    # AGC on: the raw power crosses the AGC threshold in both directions (the mode bit flips at least twice each way), both ramps
    # run, the factor is cut to 0 for a stretch, and the channel stays open across it where the squelch is disabled
    for name in ("am_agc_cross", "ambpf_agc_cross"):
        assert p[name]["agc_mode_changes"] >= 4 and p[name]["agc_up_ramp"] > 800 and p[name]["agc_down_ramp"] > 400 and p[name]["agc_cut"] > 100, (name, p[name])
        assert p[name]["open"] > 3000 and p[name]["transitions"] == 1, (name, p[name])
    assert p["amnodc_agc_cross"]["agc_mode_changes"] >= 2 and p["amnodc_agc_cross"]["agc_cut"] > 100, p["amnodc_agc_cross"]
    assert p["am_agc_squelched"]["transitions"] >= 4 and p["am_agc_squelched"]["agc_mode_changes"] >= 2, p["am_agc_squelched"]
    assert p["am_agc_nondyadic_62500"]["agc_mode_changes"] >= 2 and p["am_agc_nondyadic_62500"]["agc_up_ramp"] == 4800, p["am_agc_nondyadic_62500"]
    z = p["amnodc_agc_zero_input"]                        # m_u0 = inf, NaN amplitudes: (qint16) gives 0
    assert z["zero_ci"] == z["open"] == 1000 and z["agc_cut"] > 0 and not np.concatenate(runs["amnodc_agc_zero_input"]["feeds"]).any(), z
    for name, r in runs.items():                            # with the AGC off no AGC probe moves
        if not BY[name]["cfg"][10]:
            assert p[name]["agc_up_ramp"] == p[name]["agc_down_ramp"] == p[name]["agc_cut"] == 0, name
    assert {(c["cfg"][3], c["cfg"][10]) for c in uc.CASES} >= {(8, 0), (8, 1), (9, 0), (9, 1), (10, 0), (10, 1)}
    assert p["ambpf_all_zero"]["open"] == 0 and not np.concatenate(runs["ambpf_all_zero"]["feeds"]).any()
    for name in ("amnodc_small_feeds", "ambpf_small_feeds"):
        per_feed = [f.shape[0] for f in runs[name]["feeds"]]
        assert max(per_feed[:50]) <= 10 and per_feed[-1] > 600 and np.concatenate(runs[name]["feeds"]).any(), name


def test_release_runs_out_at_a_feed_boundary(runs):
    r = runs["iq16_release_boundary"]
    # after the third feed the squelch is still open with the release used up; the six inputs of the fourth bring the closing sample
    assert r["opens"] == [False, False, True, False, False]
    o_case = BY["iq16_release_boundary"]
    assert sum(o_case["splits"][:3]) == uc.RELEASE_BOUNDARY_SPLIT and o_case["splits"][3] == 6
    assert r["feeds"][3].shape[0] == 1 and not r["feeds"][3].any() and r["feeds"][2][-1].any()


def test_release_count_is_zero_at_that_boundary(oracle):
    case = BY["iq16_release_boundary"]
    o = uc.OracleUdp(oracle, case["cfg"])
    x = uc.inputs(case)
    o.feed(x[: 2 * uc.RELEASE_BOUNDARY_SPLIT])
    s = o.state()
    assert s["open"] and s["close_count"] == 0 and s["open_count"] == 400
    o.close()


def test_discriminator_runs_on_open_samples_only(oracle):
    """m_m1Sample is the last OPEN sample: with the squelch forced open the first sample after a gap differs"""
    case = BY["nfm_burst"]
    x = uc.inputs(case)
    gated = uc.OracleUdp(oracle, case["cfg"]).feed(x)[0]
    cfg = list(case["cfg"]); cfg[9] = 0
    free = uc.OracleUdp(oracle, tuple(cfg)).feed(x)[0]
    opened = np.flatnonzero(gated[:, 0])
    starts = opened[np.flatnonzero(np.diff(opened, prepend=-10) > 5)]
    assert starts.size >= 2
    assert any(gated[s, 0] != free[s, 0] for s in starts[1:])
    inside = opened[np.flatnonzero(np.diff(opened, prepend=-10) == 1)]
    assert np.array_equal(gated[inside], free[inside])


def test_random_cases_cover_the_branches(oracle):
    """the 100 random cases (the GPU banks of tests/test_demod_random_gpu.py run them too) through the oracle: floors on how
    many open the squelch and how many flip the AGC's mode, and every format.  With the generator and seed of
    tests/udpsrc_cases.py 77 open, 10 change the AGC mode, 5 use up the release, 44 wrap a conversion"""
    cases = uc.random_cases()
    probes = [uc.run_oracle(oracle, case)["probe"] for case in cases]
    opened = sum(p["open"] > 0 for p in probes)
    agc_moved = sum(p["agc_mode_changes"] > 0 for p in probes)
    formats = {case["cfg"][3] for case in cases}
    print("open", opened, "agc_mode_changes", agc_moved, {k: sum(p[k] > 0 for p in probes) for k in ("release_hits", "conv_wraps")})
    assert opened >= 30 and formats == set(uc.FORMATS) and agc_moved >= 8, (opened, formats, agc_moved)


@pytest.mark.ref
@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "sdrbase", "dsp")), reason="no reference tree here")
def test_oracle_vs_rebuilt_recorder_random(oracle):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_golden_udpsrc as mg
    if not mg.available(REF):
        pytest.skip("Qt headers not available")
    exe = mg.build_recorder(REF)
    cases = uc.random_cases()
    assert len(cases) == 100
    for case in cases:
        want = mg.record(exe, case["cfg"], uc.inputs(case), case["splits"])
        got = uc.run_oracle(oracle, case)
        assert [f.shape[0] for f in got["feeds"]] == [f.shape[0] for f in want["feeds"]], case
        for g, w, gs, ws in zip(got["feeds"], want["feeds"], got["specs"], want["specs"]):
            assert np.array_equal(g, w) and np.array_equal(gs, ws), case
        assert (got["in_magsq"], got["open"], got["open_count"], got["close_count"]) == \
               (want["in_magsq"], want["open"], want["open_count"], want["close_count"]), case
