"""GPU: the AM demodulator bank (sdrx_am_*) against the oracle (tests/am_oracle.c), every audio sample of every channel, m_magsq,
peak, count and squelch state bit for bit: the named cases of tests/am_cases.py, random splits, 16 mixed channels in one
handle, reset, the device hand-over from the channelizer bank, and the 64-channel load."""
import numpy as np
import pytest

import sdrangel_amd as sa
from tests import am_cases as ac
from tests import oracle_py as orc
from tests import synth

pytestmark = pytest.mark.gpu
BY = {c["name"]: c for c in ac.CASES}


@pytest.fixture(scope="module")
def oracle():
    return ac.build_oracle()


@pytest.fixture(scope="module")
def wants(oracle):
    """every named case through the oracle once, shared (and left unchanged) by the tests below"""
    return {c["name"]: ac.run_oracle(oracle, c) for c in ac.CASES}


def gcfg(cfg) -> sa.AmCfg:
    return sa.AmCfg(in_rate=int(cfg[0]), nco_freq=int(cfg[1]), audio_rate=int(cfg[2]), rf_bandwidth=float(cfg[3]), volume=float(cfg[4]),
                    squelch_db=float(cfg[5]), audio_mute=int(cfg[6]), bandpass_enable=int(cfg[7]))


def check_levels(bank, ch, want, what):
    m, s, p, n = bank.levels(ch)
    print(f"{what}: magsq {m!r} (oracle {want['magsq']!r}), sum {s!r} (oracle {want['sum']!r}), peak {p!r}, count {n}, open {bank.squelch_open(ch)}")
    assert n == want["count"], what
    assert m == want["magsq"], (what, m, want["magsq"])
    assert p == want["peak"], what
    assert bank.squelch_open(ch) == want["open"], what
    # reordering n non-negative double terms moves the sum by at most n * 2^-53 relative, on either side
    assert abs(s - want["sum"]) <= 2 * max(n, 1) * 2.0 ** -53 * want["sum"], (what, s, want["sum"])


def run_gpu(case, splits=None, bank=None):
    bank = bank or sa.AmDemodBank([gcfg(case["cfg"])])
    feeds = []
    for x in ac.cut(ac.inputs(case), splits or case["splits"]):
        bank.feed([x])
        feeds.append(bank.read(0))
    return bank, feeds


def assert_feeds_equal(got, want, what):
    assert [g.size for g in got] == [w.size for w in want], what
    for i, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), (what, i, int(np.count_nonzero(g != w)), int(np.flatnonzero(g != w)[0]))


@pytest.mark.parametrize("case", ac.CASES, ids=[c["name"] for c in ac.CASES])
def test_case_bit_exact(wants, case):
    want = wants[case["name"]]
    bank, got = run_gpu(case)
    assert_feeds_equal(got, want["feeds"], case["name"])
    check_levels(bank, 0, want, case["name"])


def test_design_products_equal_the_oracle(oracle):
    for name in ("default_airband", "nondyadic_62500", "step1_48k", "r96k_to_44k1", "rf8330", "level_edge"):
        case = BY[name]
        o = ac.OracleAm(oracle, case["cfg"])
        nt, taps, bp, inc, lvl = o.design()
        g = sa.AmDemodBank([gcfg(case["cfg"])]).design(0)
        assert g[0] == nt == 72 and g[3] == inc, name
        assert np.array_equal(g[1].view(np.uint32), taps.view(np.uint32)), name
        assert np.array_equal(g[2].view(np.uint32), bp.view(np.uint32)), name
        assert np.float32(g[4]) == np.float32(lvl)


@pytest.mark.parametrize("name", ["burst", "burst_bandpass", "nondyadic_62500", "zero_gap"])
def test_random_splits_equal_one_feed(oracle, name):
    case = BY[name]
    want = ac.run_oracle(oracle, case, splits=[case["n"]])
    one = np.concatenate(want["feeds"])
    rng = np.random.default_rng(len(name))
    for trial in range(2):
        splits, left = [], case["n"]
        while left > 0:
            m = min(left, int(rng.choice([0, 1, 2, 15, 16, 17, int(rng.integers(1, 2000)), int(rng.integers(1, 40000)), int(rng.integers(1, 40000))])))
            splits.append(m); left -= m
        bank, got = run_gpu(case, splits)
        got = np.concatenate(got)
        assert got.size == one.size and np.array_equal(got, one), (name, trial)
        check_levels(bank, 0, want, f"{name} trial {trial}")


def test_sixteen_mixed_channels_in_one_handle(wants):
    cases = list(ac.CASES)
    assert len(cases) == 16
    singles = [run_gpu(c)[1] for c in cases]
    bank = sa.AmDemodBank([gcfg(c["cfg"]) for c in cases])
    cuts = [ac.cut(ac.inputs(c), c["splits"]) for c in cases]
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
        want = wants[case["name"]]
        assert_feeds_equal(got[c], want["feeds"], case["name"])
        assert_feeds_equal(got[c], singles[c], case["name"] + " vs single-channel handle")
        check_levels(bank, c, want, case["name"])


def test_reset_restores_a_fresh_handle(wants):
    for name in ("burst_bandpass", "nondyadic_62500"):
        case = BY[name]
        want = wants[name]
        bank, first = run_gpu(case)
        assert_feeds_equal(first, want["feeds"], name)
        # leave the squelch open and the histories half full: 5000 more inputs of a strong carrier (AGC history 4800, delay 2400)
        bank.feed([ac.inputs(BY["default_airband"])[: 2 * 5000]])
        bank.feed([ac.inputs(case)[: 2 * 777]])
        bank.reset()
        assert bank.levels(0) == (0.0, 0.0, 0.0, 0) and not bank.squelch_open(0)
        _, again = run_gpu(case, bank=bank)
        assert_feeds_equal(again, want["feeds"], name + " after reset")
        check_levels(bank, 0, want, name + " after reset")


def test_levels_reset_flag_and_empty_feed(wants):
    case = ac.CASES[0]
    bank, _ = run_gpu(case)
    m, s, p, n = bank.levels(0, reset=True)
    assert n == wants[case["name"]]["count"] and s > 0 and p > 0 and m > 0
    assert bank.levels(0) == (m, 0.0, 0.0, 0)              # getMagSqLevels zeroes sum, peak and count; m_magsq stays
    bank.feed([np.zeros(0, np.int16)])
    assert bank.read(0).size == 0 and bank.last_dev(0)[1] == 0
    assert bank.levels(0) == (m, 0.0, 0.0, 0) and bank.squelch_open(0)


def test_feed_dev_and_last_dev_match_feed(wants):
    import torch
    case = BY["r96k_to_44k1"]
    want = wants[case["name"]]
    bank = sa.AmDemodBank([gcfg(case["cfg"])])
    for x, w in zip(ac.cut(ac.inputs(case), case["splits"]), want["feeds"]):
        t = torch.from_numpy(x.copy()).cuda() if x.size else torch.zeros(2, dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        bank.feed_dev([t.data_ptr()], [x.size // 2])
        ptr, n = bank.last_dev(0)
        assert n == w.size
        assert np.array_equal(bank.read(0), w)
        assert (ptr != 0) or n == 0
        bank.sync()
    check_levels(bank, 0, want, case["name"])


def test_last_launch_timing_and_stream_accessors():
    import torch
    case = ac.CASES[0]
    bank = sa.AmDemodBank([gcfg(case["cfg"])] * 3)
    x = ac.inputs(case)[: 2 * 5000]
    bank.feed([x, x, x])
    ll = bank.last_launch()
    # 5000 inputs at 60000 -> 48000: at most 5000 / 1 + 4 audio samples per channel, 256 per workgroup
    assert ll["kernel"] == "am_out_kernel" and ll["block"] == 256 and ll["grid"] == 3 * ((5000 + 255) // 256) and ll["lds_bytes"] == 151 * 4, ll
    bank.set_timing(True)
    bank.feed([x, x, x])
    ms, n = bank.get_timing()
    assert n == 1 and ms > 0
    own = bank.get_stream()
    assert own != 0
    first = bank.read(1)
    s = torch.cuda.Stream()
    bank.set_stream(s.cuda_stream)
    assert bank.get_stream() == s.cuda_stream
    bank.reset()
    bank.feed([x, x, x])
    bank.feed([x, x, x])
    assert np.array_equal(bank.read(1), first)             # the same two feeds on the caller's stream
    bank.set_stream(None)
    assert bank.get_stream() == own


def test_feed_bank_device_handover(oracle):
    """61.44 MS/s stream, 4 channels at req_rate 48000, 6 000 000 samples in three uneven feeds: the audio of feed_bank equals
    feed() of what bank.read returned and the oracle on the bank oracle's output, and the squelch opens in every channel; the
    next bank.feed queued right behind does not disturb it"""
    fs, n_ch = 61_440_000, 4
    fcs = [int(-24_000_000 + c * 13_000_000 + 1371 * c) for c in range(n_ch)]
    bank_dev = sa.ChannelizerBank(fs, [48000] * n_ch, fcs)
    bank_host = sa.ChannelizerBank(fs, [48000] * n_ch, fcs)
    cfgs, oras, chains = [], [], []
    for c in range(n_ch):
        modes, out_rate, ofs = bank_dev.info(c)
        assert out_rate >= 48000
        cfg = (out_rate, -ofs, 48000, 5000.0, 2.0, -90.0, 0, c % 2)
        cfgs.append(gcfg(cfg)); oras.append(ac.OracleAm(oracle, cfg)); chains.append(orc.Chain(modes))
    am = sa.AmDemodBank(cfgs)
    am_host = sa.AmDemodBank(cfgs)
    x = synth.mix(6_000_000, 78, 3000, 1500, 1)
    cuts = ((0, 2_000_001), (2_000_001, 4_300_000), (4_300_000, 6_000_000))
    segs = [x[2 * a: 2 * b] for a, b in cuts]
    heard = [False] * n_ch

    def check(seg):
        bank_host.feed(seg)
        chans = [bank_host.read(c) for c in range(n_ch)]
        am_host.feed(chans)
        for c in range(n_ch):
            ch_want = chains[c].feed(seg)
            assert np.array_equal(chans[c], ch_want), c
            want = oras[c].feed(ch_want)
            got = am.read(c)
            assert got.size == want.size and got.size > 0, (c, got.size, want.size)
            assert np.array_equal(got, want), c
            assert np.array_equal(got, am_host.read(c)), c
            heard[c] = heard[c] or bool(got.any())

    for i, seg in enumerate(segs):
        bank_dev.feed(seg)                   # from the second round on this overwrites the queues the demodulators were handed
        if i:
            check(segs[i - 1])               # ... before their results for the previous feed are looked at
        am.feed_bank(bank_dev)
        for c in range(n_ch):
            bank_dev.skip(c)
    check(segs[-1])
    for c in range(n_ch):
        m, s, p, n = oras[c].levels()
        assert oras[c].squelch_open() and am.squelch_open(c) and heard[c], c
        assert am.levels(c)[0] == m and am.levels(c)[2] == p and am.levels(c)[3] == n, c


def test_sixtyfour_channels_one_second(oracle):
    """64 channels x 1 s at 60 kS/s in one feed, every fourth a burst, half with the Bandpass"""
    cases = []
    for c in range(64):
        f0 = float(-6000 + 190 * c)
        cfg = (60000, -int(f0), 48000, 5000.0 if c % 3 else 8330.0, 2.0, -40.0, 0, c % 2)
        sig = {"kind": "am", "f0": f0, "depth": 0.3 + 0.01 * c, "fa": 400.0 + 30.0 * c, "amp": 6000.0, "noise": 10.0}
        if c % 4 == 0:
            sig.update(runs=[9000 + 100 * c, 2000, 14000, 7000, 4000, 3500], amps=[8000.0, 30.0])
        cases.append({"name": f"full{c}", "cfg": cfg, "sig": sig, "n": 60000, "seed": 500 + c, "splits": [60000]})
    bank = sa.AmDemodBank([gcfg(c["cfg"]) for c in cases])
    bank.feed([ac.inputs(c) for c in cases])
    for c, case in enumerate(cases):
        want = ac.run_oracle(oracle, case)
        got = bank.read(c)
        assert got.size == want["feeds"][0].size == 48001, (c, got.size)
        assert np.array_equal(got, want["feeds"][0]), (c, int(np.count_nonzero(got != want["feeds"][0])))
        assert want["probe"]["open"] > 20000, c
        check_levels(bank, c, want, case["name"])
