"""GPU: the ChannelAnalyzer bank (sdrx_chana_*) against the oracle (tests/chana_oracle.c), every Sample of every feed of every
channel and m_magsq bit for bit, no tolerance anywhere: the named cases of tests/chana_cases.py, random splits, banks of 1, 3,
17 and 65 mixed channels, reset, the device paths, the design products, a stream position past 2^31 and the accessors."""
import numpy as np
import pytest

import sdrangel_amd as sa
from tests import chana_cases as cc
from tests import oracle_py as orc
from tests import synth
from tests.demod_mixed import feed_rounds

pytestmark = pytest.mark.gpu
BY = {c["name"]: c for c in cc.CASES}


@pytest.fixture(scope="module")
def oracle():
    return cc.build_oracle()


@pytest.fixture(scope="module")
def wants(oracle):
    """every named case through the oracle once, shared (and left unchanged) by the tests below"""
    return {c["name"]: cc.run_oracle(oracle, c) for c in cc.CASES}


def gcfg(cfg) -> sa.ChanaCfg:
    return sa.ChanaCfg(pll=0, fll=0, **{k: int(v) for k, v in cfg.items()})


def run_gpu(case, splits=None, bank=None):
    bank = bank or sa.ChannelAnalyzerBank([gcfg(case["cfg"])])
    out = []
    for x in cc.cut(cc.inputs(case), splits or case["splits"]):
        bank.feed([x])
        out.append(bank.read(0))
    return bank, out


def assert_feeds_equal(got, want, what):
    assert [g.shape[0] for g in got] == [w.shape[0] for w in want], what
    for i, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), (what, i, int(np.count_nonzero(g != w)), np.argwhere(g != w)[0].tolist())


def cat(parts):
    return np.concatenate(parts) if parts else np.zeros((0, 2), np.int16)


@pytest.mark.parametrize("case", cc.CASES, ids=[c["name"] for c in cc.CASES])
def test_case_bit_exact(wants, case):
    want = wants[case["name"]]
    bank, out = run_gpu(case)
    m = bank.magsq(0)
    print(f"{case['name']}: {sum(o.shape[0] for o in out)} Samples, magsq {m!r} (oracle {want['magsq']!r})")
    assert_feeds_equal(out, want["out"], case["name"])
    assert m == want["magsq"], (case["name"], m, want["magsq"])
    assert bank.positive_only(0) == bool(case["cfg"]["ssb"])


def test_bypass_and_step_one_resampler_differ(wants):
    """the same rate and filter with and without the Interpolator: each equals its oracle (above) and they are not the same stream"""
    a, b = run_gpu(BY["dsb_default"])[1], run_gpu(BY["down_step1"])[1]
    assert cat(a).shape == cat(b).shape and not np.array_equal(cat(a), cat(b))


def test_design_products_equal_the_oracle(wants):
    for name in ("dsb_default", "lsb_swap", "band_reject", "band_clamp", "rrc_0", "rrc_35", "rrc_100", "down_96k_37k", "down_rrc_negative", "nco_fractional"):
        case = BY[name]
        nt, taps, filt, inc = wants[name]["design"]
        g = sa.ChannelAnalyzerBank([gcfg(case["cfg"])]).design(0)
        assert g[0] == nt == 72, name
        assert np.array_equal(g[1].view(np.uint32), taps.view(np.uint32)), name
        used = 2048 if case["cfg"]["ssb"] else 4096
        assert np.array_equal(g[2][:used].view(np.uint32), filt[:used].view(np.uint32)), name
        assert filt[:used].any() or name == "down_rrc_negative", name
        assert np.float32(g[3]) == np.float32(inc), name


SPLIT_SIZES = [0, 1, 2, 511, 512, 513, 1023, 1024, 4095, 4096, 4097]


@pytest.mark.parametrize("name", ["usb", "rrc_35", "span8", "down_96k_37k", "corr_dsb_quiet", "corr_lsb_loud", "corr_span2"])
def test_random_splits_equal_one_feed(oracle, name):
    case = BY[name]
    want = cc.run_oracle(oracle, case, splits=[case["n"]])
    rng = np.random.default_rng(len(name))
    splits, left = [], case["n"]
    while left > 0:
        m = min(left, int(rng.choice(SPLIT_SIZES + [int(rng.integers(1, 6000))])))
        splits.append(m); left -= m
    bank, out = run_gpu(case, splits)
    assert np.array_equal(cat(out), cat(want["out"])), name
    assert bank.magsq(0) == want["magsq"], name


def _mixed(names, wants):
    cases = [BY[n] for n in names]
    bank = sa.ChannelAnalyzerBank([gcfg(c["cfg"]) for c in cases])
    got = feed_rounds(bank, [cc.cut(cc.inputs(c), c["splits"]) for c in cases], lambda b, c: b.read(c))
    for c, case in enumerate(cases):
        assert_feeds_equal(got[c], wants[case["name"]]["out"], case["name"])
        assert bank.magsq(c) == wants[case["name"]]["magsq"], case["name"]
    return bank


def test_three_mixed_channels_in_one_handle(wants):
    _mixed(["rrc_35", "corr_lsb_loud", "down_96k_37k"], wants)


def test_seventeen_mixed_channels_in_one_handle(wants):
    """mixed filters, rates and input types; the last round's feeds complete blocks of several autocorrelation channels at once"""
    names = ["dsb_default", "usb", "lsb_swap", "band_reject", "band_clamp", "nco_fractional", "nco_negative", "rrc_0", "rrc_100", "span3", "span8",
             "down_48k_12k", "down_96k_37k", "down_rrc_negative", "corr_dsb_quiet", "corr_usb_quiet", "corr_span2"]
    assert len(names) == 17
    _mixed(names, wants)


def test_sixty_five_channels_cross_the_oscillator_walk_workgroup(oracle):
    """be_ncof_kernel walks 64 channels per workgroup: the 65th is the second workgroup's first lane.  Every channel has its own
    fractional increment, every third runs behind the Interpolator; two feeds of 1100 and 700 inputs"""
    cfgs = [cc._cfg(50000, nco_freq=-101 * c - 7, ssb=1, span_log2=c % 3, down_sample=int(c % 3 == 2), down_sample_rate=25000 if c % 3 == 2 else 0)
            for c in range(65)]
    bank = sa.ChannelAnalyzerBank([gcfg(k) for k in cfgs])
    oras = [cc.OracleChana(oracle, k) for k in cfgs]
    xs = [synth.mix(1800, 300 + c, 300, 8000, 1) for c in range(65)]
    total = 0
    for a, b in ((0, 1100), (1100, 1800)):
        bank.feed([x[2 * a: 2 * b] for x in xs])
        for c in range(65):
            w = oras[c].feed(xs[c][2 * a: 2 * b])
            g = bank.read(c)
            assert g.shape == w.shape and np.array_equal(g, w), (c, g.shape, w.shape)
            total += g.shape[0]
    assert total > 65 * 200 and all(bank.magsq(c) == oras[c].magsq() for c in range(65))


def test_corr_kernel_gets_more_than_one_workgroup_in_both_dimensions(wants):
    """three autocorrelation channels, one feed of 8804 inputs each: at most 8804 + 1024 filtered samples are 39 workgroups of
    256 groups, which can complete (4095 + 39 * 256) // 4096 = 3 blocks on top of an open one: a grid of 3 blocks by 3 channels,
    of which 2 by 3 have a block to transform"""
    names = ["corr_dsb_quiet", "corr_dsb_loud", "corr_usb_quiet"]
    cases = [BY[n] for n in names]
    bank = sa.ChannelAnalyzerBank([gcfg(c["cfg"]) for c in cases])
    n = 2 * 4096 + 100 + 512
    bank.feed([cc.inputs(c)[: 2 * n] for c in cases])
    ll = bank.last_launch()
    assert ll["kernel"] == "chana_corr_kernel" and ll["block"] == 1024 and ll["lds_bytes"] == 2 * 8192 * 8 + 2049 * 4, ll
    assert ll["grid"] == 3 * 3, ll
    for c, case in enumerate(cases):
        want = cat(wants[case["name"]]["out"])
        got = bank.read(c)
        assert got.shape[0] >= 2 * 4096 and np.array_equal(got, want[: got.shape[0]]), case["name"]


def test_reset_restores_a_fresh_handle(wants):
    for name in ("span8", "corr_dsb_quiet", "down_96k_37k"):
        case = BY[name]
        want = wants[name]
        bank, first = run_gpu(case)
        assert_feeds_equal(first, want["out"], name)
        # leave the counters, an open group and an open block half way
        bank.feed([cc.inputs(BY["dsb_default"])[: 2 * 3000]])
        bank.feed([cc.inputs(case)[: 2 * 777]])
        bank.reset()
        assert bank.magsq(0) == 0.0
        _, again = run_gpu(case, bank=bank)
        assert_feeds_equal(again, want["out"], name + " after reset")
        assert bank.magsq(0) == want["magsq"], name


def test_feed_dev_and_last_dev_match_feed(wants):
    import torch
    for name in ("down_96k_37k", "corr_lsb_quiet"):
        case = BY[name]
        want = wants[name]
        bank = sa.ChannelAnalyzerBank([gcfg(case["cfg"])])
        for x, w in zip(cc.cut(cc.inputs(case), case["splits"]), want["out"]):
            t = torch.from_numpy(x.copy()).cuda() if x.size else torch.zeros(2, dtype=torch.int16, device="cuda")
            torch.cuda.synchronize()
            bank.feed_dev([t.data_ptr()], [x.size // 2])
            ptr, n = bank.last_dev(0)
            assert n == w.shape[0] and np.array_equal(bank.read(0), w)
            assert (ptr != 0) or n == 0
            bank.sync()
        assert bank.magsq(0) == want["magsq"], name


def test_past_two_to_the_31_filtered_samples(oracle):
    """the carried counters preset through sdrx_chana_seek and the oracle's chao_seek: m_undersampleCount's low bits pick the
    groups, fftcorr's call counter follows them; a signal channel and an autocorrelation channel"""
    for name, pos in (("span3", (1 << 31) + 5), ("corr_span2", (1 << 32) + (1 << 31) + 4 * 4000 + 2), ("span8", (1 << 33) + 255)):
        case = BY[name]
        o = cc.OracleChana(oracle, case["cfg"])
        o.seek(pos)
        bank = sa.ChannelAnalyzerBank([gcfg(case["cfg"])])
        bank.seek(0, pos)
        total = 0
        for x in cc.cut(cc.inputs(case), case["splits"]):
            w = o.feed(x)
            bank.feed([x])
            g = bank.read(0)
            assert g.shape == w.shape and np.array_equal(g, w), (name, g.shape, w.shape)
            total += g.shape[0]
        assert total > 0 and bank.magsq(0) == o.magsq(), name
        bank.reset()                                     # and reset goes back to position 0
        assert_feeds_equal(run_gpu(case, bank=bank)[1], cc.run_oracle(oracle, case)["out"], name + " after reset")


def test_accessors():
    """the accessor set of tests/test_handle_accessors_gpu.py, on this family"""
    import torch
    case = BY["usb"]
    h = sa.ChannelAnalyzerBank([gcfg(case["cfg"])] * 3)
    x = cc.inputs(case)[: 2 * 3000]

    def feed():
        h.feed([x, x, x])
        return h.read(1)

    h.reset()
    own_out = feed()
    assert own_out.shape[0] == 2560 and own_out.any()        # 3000 inputs, no Interpolator: five blocks of 512
    assert h.get_timing()[1] == 0                           # timing off: a feed is not counted
    ll = h.last_launch()
    # at most 3000 filter inputs per channel plus one held-back block of up to 1024, 256 groups per workgroup; no LDS
    assert ll["kernel"] == "chana_group_kernel" and ll["block"] == 256 and ll["grid"] == 3 * ((3000 + 1024 + 255) // 256), ll
    assert ll["lds_bytes"] == 0, ll
    h.set_timing(True)
    feed()
    ms, n = h.get_timing(reset=False)
    assert n == 1 and ms > 0, (ms, n)
    assert h.get_timing(reset=True) == (ms, n)
    assert h.get_timing() == (0.0, 0)
    h.set_timing(False)
    own = h.get_stream()
    assert own != 0
    s = torch.cuda.Stream()
    h.set_stream(s.cuda_stream)
    assert h.get_stream() == s.cuda_stream
    h.reset()
    got = feed()
    assert got.dtype == own_out.dtype and np.array_equal(got, own_out)     # the same feed from a fresh state on the caller's stream
    h.sync()
    h.set_stream(None)
    assert h.get_stream() == own
    h.feed([np.zeros(0, np.int16)] * 3)
    assert h.read(0).shape[0] == 0 and h.last_dev(0)[1] == 0
    h.close()


def test_feed_bank_device_handover(oracle):
    """61.44 MS/s stream, 4 channels at req_rate 48000, 3 000 000 samples in three uneven feeds: the Samples of feed_bank equal the
    oracle on the bank oracle's output; the next bank.feed queued right behind does not disturb them"""
    fs, n_ch = 61_440_000, 4
    fcs = [int(-24_000_000 + c * 13_000_000 + 1371 * c) for c in range(n_ch)]
    bank_dev = sa.ChannelizerBank(fs, [48000] * n_ch, fcs)
    cfgs, oras, chains = [], [], []
    for c in range(n_ch):
        modes, out_rate, ofs = bank_dev.info(c)
        assert out_rate >= 48000
        cfg = cc._cfg(out_rate, nco_freq=-ofs, ssb=int(c == 1), bandwidth=-5000 if c == 1 else 5000, rrc=int(c == 2), span_log2=c,
                      down_sample=int(c == 3), down_sample_rate=48000 if c == 3 else 0, input_type=cc.AUTOCORR if c == 0 else cc.SIGNAL)
        cfgs.append(gcfg(cfg)); oras.append(cc.OracleChana(oracle, cfg)); chains.append(orc.Chain(modes))
    ana = sa.ChannelAnalyzerBank(cfgs)
    x = synth.mix(3_000_000, 78, 3000, 1500, 1)
    cuts = ((0, 1_000_001), (1_000_001, 2_150_000), (2_150_000, 3_000_000))
    segs = [x[2 * a: 2 * b] for a, b in cuts]
    total = [0] * n_ch

    def check(seg):
        for c in range(n_ch):
            w = oras[c].feed(chains[c].feed(seg))
            g = ana.read(c)
            assert g.shape == w.shape and np.array_equal(g, w), (c, g.shape, w.shape)
            total[c] += g.shape[0]

    for i, seg in enumerate(segs):
        bank_dev.feed(seg)                   # from the second round on this overwrites the queues the analyzers were handed
        if i:
            check(segs[i - 1])               # ... before their results for the previous feed are looked at
        ana.feed_bank(bank_dev)
        for c in range(n_ch):
            bank_dev.skip(c)
    check(segs[-1])
    for c in range(n_ch):
        assert total[c] > 0 and ana.magsq(c) == oras[c].magsq(), (c, total)
