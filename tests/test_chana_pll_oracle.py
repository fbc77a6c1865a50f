"""The C restatement of ChannelAnalyzer::feed with the PLL, the FLL and InputPLL (tests/chana_pll_oracle.c, the checker of
sdrx_chanapll_*; its cosf, sinf and atan2f are its own) against the reference's own PhaseLockComplex, FreqLockComplex, NCOF,
Interpolator, fftfilt and fftcorr: every case of tests/chana_pll_cases.py recorded by tests/golden/make_golden_chana_pll.py into
tests/golden/chana_pll_golden.npz (the Samples, m_magsq, isPllLocked and the bits of the three floats after every feed), all bit
for bit: the loops feed back, so nothing less means anything.  Probe counters show that a case reaches what it is named for.
Where the reference tree and Qt are present, a `ref` test rebuilds the recorder and compares 100 random configurations.

The 100 random cases (random_cases(): a signal made for every channel, n sized in closed groups) are what the GPU runs in wide banks
(tests/test_chana_random_gpu.py).  Here their shares are asserted on the oracle's probes, the oracle's runs are compared with the
recorder's digests (tests/golden/chana_random_golden.npz: counts, a SHA-256 of every feed's Samples, m_magsq, isPllLocked and the
state bits), and a second `ref` test compares every Sample with the live recorder."""
import os

import numpy as np
import pytest

from tests import chana_pll_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "chana_pll_golden.npz")
REF = "/root/reference"
BY = {c["name"]: c for c in pc.CASES}


@pytest.fixture(scope="module")
def oracle():
    return pc.build_oracle()


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def runs(oracle, golden):
    """every case through the oracle once, on the fixture's inputs, shared by the tests below"""
    return {c["name"]: pc.run_oracle(oracle, c["cfg"], pc.cut(golden[f"{c['name']}/in"], c["splits"])) for c in pc.CASES}


@pytest.fixture(scope="module")
def random_runs(oracle):
    """the 100 random cases through the oracle once"""
    cases = pc.random_cases()
    return cases, [pc.run_case(oracle, c) for c in cases]


def _maker():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_golden_chana_pll as mg
    return mg


def _cat(parts):
    return np.concatenate(parts) if parts else np.zeros((0, 2), np.int16)


def test_golden_covers_every_case_and_notes_its_host(golden):
    assert {k.split("/")[0] for k in golden.files} - {"host"} == {c["name"] for c in pc.CASES}
    host = str(golden["host"])
    assert "glibc" in host and "fma=1" in host, host
    for c in pc.CASES:
        assert np.array_equal(golden[f"{c['name']}/in"], pc.inputs(c)), c["name"]


@pytest.mark.parametrize("case", pc.CASES, ids=[c["name"] for c in pc.CASES])
def test_oracle_matches_reference_recording(runs, golden, case):
    name = case["name"]
    r = runs[name]
    assert [a.shape[0] for a in r["out"]] == golden[f"{name}/counts"].tolist()
    full, want = _cat(r["out"]), golden[f"{name}/out"]
    assert full.shape == want.shape and np.array_equal(full, want), (name, int(np.count_nonzero(full != want)))
    assert [s[0] for s in r["states"]] == golden[f"{name}/locked"].tolist(), name
    assert np.array_equal(np.array([s[1:4] for s in r["states"]], np.uint32).reshape(-1, 3), golden[f"{name}/state_bits"]), name
    assert [s[4] for s in r["states"]] == golden[f"{name}/magsq"].tolist(), name


def test_cases_reach_what_they_are_named_after(runs, golden):
    p = {n: r["probe"] for n, r in runs.items()}
    locked = {n: [s[0] for s in r["states"]] for n, r in runs.items()}
    # lock acquired, then lost after the frequency step
    seq = locked["pll_lock_lost_dsb"]
    assert 1 in seq and seq[-1] == 0 and seq.index(1) < len(seq) - 1 - seq[::-1].index(1) < len(seq) - 1, seq
    assert p["pll_lock_lost_dsb"]["lock_up"] > 478 and p["pll_lock_lost_dsb"]["lock_down"] > 0
    # both saturation branches
    assert p["pll_above_usb"]["sat_hi"] > 1 and p["pll_above_usb"]["sat_lo"] == 0
    assert p["pll_below_lsb"]["sat_lo"] > 1 and p["pll_below_lsb"]["sat_hi"] == 0
    # a normalizeAngle loop taken more than once
    assert p["psk4_noisy"]["turns_many"] > 100 and p["psk16_lsb"]["turns_many"] > 1000
    assert all(p[n]["turns_many"] == 0 for n in p if BY[n]["cfg"]["psk_order"] < 4)
    # the PSK lock counter up and down, and a lock through it
    assert p["psk4_noisy"]["lock_up"] > 1 and p["psk4_noisy"]["lock_down"] > 0
    assert p["psk2_span3"]["lock_up"] == 20 and locked["psk2_span3"][-1] == 1
    # m_lockTime 1: locked() is true from the start
    assert locked["pll_span8"] == [1] * 9 and p["pll_span8"]["steps"] == 12
    # the FLL's phase past 120: the large reduction
    for n in ("fll_pll", "fll_pll_in1_lsb", "minus_32768_fll"):
        assert p[n]["big_arg"] > 1000, n
    assert all(p[n]["big_arg"] == 0 for n in p if not BY[n]["cfg"]["fll"])
    # silence: arg(0) at every step
    for n in ("silence_pll", "silence_fll"):
        assert p[n]["arg_zero"] == p[n]["steps"] > 3000 and not golden[f"{n}/in"].any(), n
    assert golden["minus_32768/in"].min() == golden["minus_32768/in"].max() == -32768
    # no loop runs with pll clear; the Sample of the unfed oscillator is (1, 0) * 32768 as x86-64 converts it
    for n in ("in1_unfed", "in1_fll_only_lsb", "fll_only"):
        assert p[n]["steps"] == 0, n
    assert (golden["in1_unfed/out"] == np.array([-32768, 0], np.int16)).all() and (golden["in1_fll_only_lsb/out"] == np.array([0, -32768], np.int16)).all()
    # InputPLL with a loop: the oscillator turns
    assert len(np.unique(golden["in1_pll/out"], axis=0)) > 100 and len(np.unique(golden["fll_pll_in1_lsb/out"], axis=0)) > 100
    # the autocorrelation behind the PLL: two blocks completed
    assert golden["corr_pll/out"].shape[0] > 2 * 4096 and golden["corr_pll/out"][4095:].any() and not golden["corr_pll/out"][:4095].any()


@pytest.mark.parametrize("name", ["pll_lock_lost_dsb", "psk16_lsb", "fll_pll", "corr_pll", "pll_down_96k_37k"])
def test_one_feed_equals_the_case_splits(oracle, runs, golden, name):
    one = pc.run_oracle(oracle, BY[name]["cfg"], [golden[f"{name}/in"]])
    assert np.array_equal(_cat(one["out"]), _cat(runs[name]["out"])) and one["states"][-1] == runs[name]["states"][-1]


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "sdrbase", "dsp")), reason="reference tree not present")
def test_ref_recorder_on_random_configurations(oracle):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_golden_chana_pll as mg
    if not mg.available(REF):
        pytest.skip("Qt headers not present")
    if "glibc" not in mg.host_note() or "fma=1" not in mg.host_note():
        pytest.skip("the recorder would call a libm other than the fused glibc build the oracle restates")
    exe = mg.build_recorder(REF)
    rng = np.random.default_rng(20261020)
    kinds = set()
    for i in range(100):
        cfg = pc.random_cfg(rng)
        n = 2500 if cfg["input_type"] != pc.AUTOCORR else 5200
        x = pc.random_signal(rng, n)
        splits = [int(rng.integers(0, n // 2))]
        splits.append(n - splits[0])
        want = mg.record(exe, cfg, x, splits)
        got = pc.run_oracle(oracle, cfg, pc.cut(x, splits))
        assert all(np.array_equal(g, w) for g, w in zip(got["out"], want["out"])), (i, cfg)
        assert got["states"] == want["states"], (i, cfg, got["states"], want["states"])
        kinds.add((cfg["pll"], cfg["fll"], cfg["input_type"]))
    assert len(kinds) >= 10, kinds


def test_random_cases_cover_the_branches(random_runs):
    cases, results = random_runs
    assert len(cases) == 100 and len({c["name"] for c in cases}) == 100
    assert cases == pc.random_cases()                         # drawn in order from one generator with a fixed seed
    pc.assert_random_shares(cases, results)


def test_random_cases_match_the_reference_digests(random_runs):
    """ties the oracle to the reference where the reference does not exist: the recorder's digests of every feed of every case"""
    cases, results = random_runs
    want = np.load(os.path.join(ROOT, "tests", "golden", "chana_random_golden.npz"))
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "chana_random_golden.npz")) < os.path.getsize(GOLDEN)
    host = str(want["host"])
    assert "glibc" in host and "fma=1" in host, host
    got = _maker().digest(cases, results)
    assert set(got) | {"host"} == set(want.files)
    assert got["names"].tolist() == want["names"].tolist() and got["feeds"].tolist() == want["feeds"].tolist()
    ends = np.cumsum(got["feeds"])
    for k in ("counts", "sha", "locked", "state_bits", "magsq"):
        bad = np.flatnonzero((got[k] != want[k]).reshape(len(got[k]), -1).any(axis=1))
        assert got[k].shape == want[k].shape and not bad.size, (k, [cases[int(np.searchsorted(ends, b, side="right"))]["name"] for b in bad[:5]])
    assert want["counts"].sum() > 400000 and want["locked"].sum() > 60


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "sdrbase", "dsp")), reason="reference tree not present")
def test_ref_recorder_on_random_cases(random_runs):
    """all 100 through the live recorder: every Sample of every feed, m_magsq, locked and the three state floats as bits"""
    mg = _maker()
    if not mg.available(REF):
        pytest.skip("Qt headers not present")
    if "glibc" not in mg.host_note() or "fma=1" not in mg.host_note():
        pytest.skip("the recorder would call a libm other than the fused glibc build the oracle restates")
    exe = mg.build_recorder(REF)
    cases, results = random_runs
    for c, got in zip(cases, results):
        want = mg.record(exe, c["cfg"], pc.inputs(c), c["splits"])
        assert [g.shape for g in got["out"]] == [w.shape for w in want["out"]], c
        assert all(np.array_equal(g, w) for g, w in zip(got["out"], want["out"])), c
        assert got["states"] == want["states"], (c, got["states"], want["states"])
