"""GPU: the wideband-FM demodulator bank (sdrx_wfm_*) against the oracle (tests/wfm_oracle.c), every audio sample of every
channel: the named cases of tests/wfm_cases.py, random splits, 16 mixed channels in one handle, reset, the device hand-over
from the channelizer bank, and the full-size load."""
import numpy as np
import pytest

import sdrangel_amd as sa
from tests import oracle_py as orc
from tests import synth
from tests import wfm_cases as wc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def oracle():
    return wc.build_oracle()


def gcfg(cfg) -> sa.WfmCfg:
    return sa.WfmCfg(in_rate=int(cfg[0]), nco_freq=int(cfg[1]), audio_rate=int(cfg[2]), rf_bandwidth=float(cfg[3]), af_bandwidth=float(cfg[4]),
                     volume=float(cfg[5]), squelch_db=float(cfg[6]), audio_mute=int(cfg[7]))


def check_levels(bank, ch, want, what):
    s, p, n = bank.levels(ch)
    print(f"{what}: sum {s!r} (oracle {want['sum']!r}), peak {p!r}, count {n}, open {bank.squelch_open(ch)}")
    assert n == want["count"], what
    assert p == want["peak"], what
    assert bank.squelch_open(ch) == want["open"], what
    # reordering n non-negative double terms moves the sum by at most n * 2^-53 relative, on either side
    assert abs(s - want["sum"]) <= 2 * max(n, 1) * 2.0 ** -53 * want["sum"], (what, s, want["sum"])


def run_gpu(case, splits=None, bank=None):
    bank = bank or sa.WfmDemodBank([gcfg(case["cfg"])])
    feeds = []
    for x in wc.cut(wc.inputs(case), splits or case["splits"]):
        bank.feed([x])
        feeds.append(bank.read(0))
    return bank, feeds


def assert_feeds_equal(got, want, what):
    assert [g.size for g in got] == [w.size for w in want], what
    for i, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), (what, i, int(np.count_nonzero(g != w)))


@pytest.mark.parametrize("case", wc.CASES, ids=[c["name"] for c in wc.CASES])
def test_case_bit_exact(oracle, case):
    want = wc.run_oracle(oracle, case)
    bank, got = run_gpu(case)
    assert_feeds_equal(got, want["feeds"], case["name"])
    check_levels(bank, 0, want, case["name"])


@pytest.mark.parametrize("case", wc.DYADIC_CASES, ids=[c["name"] for c in wc.DYADIC_CASES])
def test_case_bit_exact_on_the_forced_serial_schedule(oracle, case, monkeypatch):
    """SDRX_WFM_SERIAL_SCHEDULE=1 (read by sdrx_wfm_create): wfm_sched_walk_kernel on the steps that wfm_prep_kernel and
    wfm_sched_fill_kernel otherwise take in closed form -- walk and closed form against the same oracle on the same channel"""
    monkeypatch.setenv("SDRX_WFM_SERIAL_SCHEDULE", "1")
    want = wc.run_oracle(oracle, case)
    bank, got = run_gpu(case)
    assert_feeds_equal(got, want["feeds"], case["name"] + " serial")
    check_levels(bank, 0, want, case["name"] + " serial")


def test_design_products_equal_the_oracle(oracle):
    for case in wc.CASES[:6]:
        o = wc.OracleWfm(oracle, case["cfg"])
        nt, taps, filt, inc, lvl = o.design()
        g = sa.WfmDemodBank([gcfg(case["cfg"])]).design(0)
        assert g[0] == nt == 72 and g[3] == inc, case["name"]
        assert np.array_equal(g[1].view(np.uint32), taps.view(np.uint32)), case["name"]
        assert np.array_equal(g[2].view(np.uint32), filt.view(np.uint32)), case["name"]
        assert np.float32(g[4]) == np.float32(lvl)


@pytest.mark.parametrize("name", ["default_240k", "nondyadic_250k", "burst_48k", "burst_240k_fraccap"])
def test_random_splits_equal_one_feed(oracle, name):
    case = {c["name"]: c for c in wc.CASES}[name]
    want = wc.run_oracle(oracle, case, splits=[case["n"]])
    one = np.concatenate(want["feeds"])
    rng = np.random.default_rng(len(name))
    for trial in range(3):
        splits, left = [], case["n"]
        while left > 0:
            m = min(left, int(rng.choice([0, 1, 2, 511, 512, 513, int(rng.integers(1, 2000)), int(rng.integers(1, 40000))])))
            splits.append(m); left -= m
        bank, got = run_gpu(case, splits)
        got = np.concatenate(got)
        assert got.size == one.size and np.array_equal(got, one), (name, trial)
        check_levels(bank, 0, want, f"{name} trial {trial}")


def _mixed16():
    cases = list(wc.CASES)
    for k, name in enumerate(["default_120k", "burst_48k"]):
        c = dict({c["name"]: c for c in wc.CASES}[name])
        c["name"] += "_again"; c["seed"] = 100 + k; c["splits"] = wc._ragged(c["n"], 100 + k)
        cases.append(c)
    assert len(cases) == 16
    return cases


def test_sixteen_mixed_channels_in_one_handle(oracle):
    cases = _mixed16()
    want = [wc.run_oracle(oracle, c) for c in cases]
    singles = [run_gpu(c)[1] for c in cases]
    bank = sa.WfmDemodBank([gcfg(c["cfg"]) for c in cases])
    cuts = [wc.cut(wc.inputs(c), c["splits"]) for c in cases]
    rounds = max(len(x) for x in cuts)
    empty = np.zeros(0, np.int16)
    got = [[] for _ in cases]
    for r in range(rounds):
        bank.feed([x[r] if r < len(x) else empty for x in cuts])
        for c, x in enumerate(cuts):
            a = bank.read(c)
            if r < len(x):
                got[c].append(a)
            else:
                assert a.size == 0, (c, r)                  # an empty feed: no audio, state untouched
    for c, case in enumerate(cases):
        assert_feeds_equal(got[c], want[c]["feeds"], case["name"])
        assert_feeds_equal(got[c], singles[c], case["name"] + " vs single-channel handle")
        check_levels(bank, c, want[c], case["name"])


def test_reset_restores_a_fresh_handle(oracle):
    for name in ("burst_240k_fraccap", "nondyadic_250k"):
        case = {c["name"]: c for c in wc.CASES}[name]
        want = wc.run_oracle(oracle, case)
        bank, first = run_gpu(case)
        assert_feeds_equal(first, want["feeds"], name)
        bank.feed([wc.inputs(case)[: 2 * 777]])            # leave pending samples and a half-way state behind
        bank.reset()
        assert bank.levels(0) == (0.0, 0.0, 0) and not bank.squelch_open(0)
        _, again = run_gpu(case, bank=bank)
        assert_feeds_equal(again, want["feeds"], name + " after reset")
        check_levels(bank, 0, want, name + " after reset")


def test_levels_reset_flag_and_empty_feed():
    case = wc.CASES[0]
    bank, _ = run_gpu(case)
    s, p, n = bank.levels(0, reset=True)
    assert n == (case["n"] // 512) * 512 and s > 0 and p > 0
    assert bank.levels(0) == (0.0, 0.0, 0)
    bank.feed([np.zeros(0, np.int16)])
    assert bank.read(0).size == 0 and bank.last_dev(0)[1] == 0


def test_feed_dev_and_last_dev_match_feed(oracle):
    import torch
    case = {c["name"]: c for c in wc.CASES}["r384k_to_44k1"]
    want = wc.run_oracle(oracle, case)
    bank = sa.WfmDemodBank([gcfg(case["cfg"])])
    for x, w in zip(wc.cut(wc.inputs(case), case["splits"]), want["feeds"]):
        t = torch.from_numpy(x.copy()).cuda() if x.size else torch.zeros(2, dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        bank.feed_dev([t.data_ptr()], [x.size // 2])
        ptr, n = bank.last_dev(0)
        assert n == w.size
        assert np.array_equal(bank.read(0), w)
        bank.sync()


def test_last_launch_names_the_new_kernels():
    case = wc.CASES[0]
    bank = sa.WfmDemodBank([gcfg(case["cfg"])] * 3)
    x = wc.inputs(case)[: 2 * 5000]
    bank.feed([x, x, x])
    ll = bank.last_launch()
    assert ll["kernel"] == "wfm_fft_kernel" and ll["block"] == 128 and ll["grid"] == 3 * (5000 // 512) and ll["lds_bytes"] > 16384, ll
    bank.set_timing(True)
    bank.feed([x, x, x])
    ms, n = bank.get_timing()
    assert n == 1 and ms > 0
    assert bank.get_stream() != 0


def test_feed_bank_device_handover(oracle):
    """61.44 MS/s stream, 8 channels at req_rate = requiredBW(80000): the audio of feed_bank equals feed() of what bank.read
    returned and the oracle on the bank oracle's output; a second bank.feed queued right behind does not disturb it"""
    fs, n_ch = 61_440_000, 8
    req = wc.required_bw(80000)
    fcs = [int(-24_000_000 + c * 6_500_000 + 1371 * c) for c in range(n_ch)]
    bank_dev = sa.ChannelizerBank(fs, [req] * n_ch, fcs)
    bank_host = sa.ChannelizerBank(fs, [req] * n_ch, fcs)
    cfgs, oras, chains = [], [], []
    for c in range(n_ch):
        modes, out_rate, ofs = bank_dev.info(c)
        cfg = (out_rate, -ofs, 48000, 80000.0, 15000.0, 2.0, -60.0, 0)
        cfgs.append(gcfg(cfg)); oras.append(wc.OracleWfm(oracle, cfg)); chains.append(orc.Chain(modes))
    wfm = sa.WfmDemodBank(cfgs)
    wfm_host = sa.WfmDemodBank(cfgs)
    x = synth.mix(3_000_000, 78, 3000, 1500, 1)
    cuts = ((0, 1_000_001), (1_000_001, 2_100_000), (2_100_000, 3_000_000))
    segs = [x[2 * a: 2 * b] for a, b in cuts]

    def check(seg):
        bank_host.feed(seg)
        chans = [bank_host.read(c) for c in range(n_ch)]
        wfm_host.feed(chans)
        for c in range(n_ch):
            ch_want = chains[c].feed(seg)
            assert np.array_equal(chans[c], ch_want), c
            want = oras[c].feed(ch_want)
            got = wfm.read(c)
            assert got.size == want.size and got.size > 0, (c, got.size, want.size)
            assert np.array_equal(got, want), c
            assert np.array_equal(got, wfm_host.read(c)), c

    for i, seg in enumerate(segs):
        bank_dev.feed(seg)                   # from the second round on this overwrites the queues the demodulators were handed
        if i:
            check(segs[i - 1])               # ... before their results for the previous feed are looked at
        wfm.feed_bank(bank_dev)
        for c in range(n_ch):
            bank_dev.skip(c)
    check(segs[-1])


def test_fullsize_32_channels_one_second(oracle):
    """32 channels x 1 s at the bank's output rate for requiredBW(80000) on a 61.44 MS/s stream, one feed"""
    modes, in_rate, _ofs = sa.chan_plan(61_440_000, wc.required_bw(80000), 1_000_000)
    assert in_rate >= 120000
    cases = []
    for c in range(32):
        f0 = float(-20000 + 1300 * c)
        cfg = (in_rate, -int(f0), 48000, 80000.0, 15000.0, 2.0, -60.0 if c % 4 else -30.0, 0)
        sig = {"kind": "fm" if c % 4 else "burst", "f0": f0, "dev": 50000.0, "fa": 400.0 + 100.0 * c, "amp": 6000.0, "hi": 12000.0, "lo": 60.0,
               "noise": 10.0, "runs": [3000 + 100 * c, 1000, 5000, 700, 20000, 30000]}
        cases.append({"name": f"full{c}", "cfg": cfg, "sig": sig, "n": in_rate, "seed": 500 + c, "splits": [in_rate]})
    bank = sa.WfmDemodBank([gcfg(c["cfg"]) for c in cases])
    bank.feed([wc.inputs(c) for c in cases])
    for c, case in enumerate(cases):
        want = wc.run_oracle(oracle, case)
        got = bank.read(c)
        assert got.size == want["feeds"][0].size and got.size > 40000, (c, got.size)
        assert np.array_equal(got, want["feeds"][0]), c
        check_levels(bank, c, want, case["name"])
