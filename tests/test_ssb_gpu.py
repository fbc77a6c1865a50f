"""GPU: the SSB / DSB demodulator bank (sdrx_ssb_*) against the oracle (tests/ssb_oracle.c), every audio pair and every spectrum
Sample of every channel, m_audioActive, m_magsq, peak and count bit for bit: the named cases of tests/ssb_cases.py, random
splits, banks of 1, 3 and 17 mixed channels, reset, the device paths, the accessors, and -- independent of that oracle -- the
composition of older handles, sdrx_backend_* (filt_mode 2) feeding sdrx_audiotail_* kind 1."""
import numpy as np
import pytest

import sdrangel_amd as sa
from tests import oracle_py as orc
from tests import ssb_cases as sc
from tests import synth
from tests.demod_mixed import feed_rounds

pytestmark = pytest.mark.gpu
BY = {c["name"]: c for c in sc.CASES}


@pytest.fixture(scope="module")
def oracle():
    return sc.build_oracle()


@pytest.fixture(scope="module")
def wants(oracle):
    """every named case through the oracle once, shared (and left unchanged) by the tests below"""
    return {c["name"]: sc.run_oracle(oracle, c) for c in sc.CASES}


def gcfg(cfg) -> sa.SsbCfg:
    return sa.SsbCfg(**{k: (float(v) if k in ("rf_bandwidth", "low_cutoff", "volume") else int(v)) for k, v in cfg.items()})


def check_levels(bank, ch, want, what):
    m, s, p, n = bank.levels(ch)
    print(f"{what}: magsq {m!r} (oracle {want['magsq']!r}), sum {s!r} (oracle {want['sum']!r}), peak {p!r}, count {n}, active {bank.audio_active(ch)}")
    assert n == want["count"], what
    assert m == want["magsq"], (what, m, want["magsq"])
    assert p == want["peak"], what
    assert bank.audio_active(ch) == want["active"], what
    # reordering n non-negative double terms moves the sum by at most n * 2^-53 relative, on either side
    assert abs(s - want["sum"]) <= 2 * max(n, 1) * 2.0 ** -53 * want["sum"], (what, s, want["sum"])


def run_gpu(case, splits=None, bank=None):
    bank = bank or sa.SsbDemodBank([gcfg(case["cfg"])])
    audio, spec = [], []
    for x in sc.cut(sc.inputs(case), splits or case["splits"]):
        bank.feed([x])
        audio.append(bank.read(0)); spec.append(bank.read_spectrum(0))
    return bank, audio, spec


def assert_feeds_equal(got, want, what):
    assert [g.shape[0] for g in got] == [w.shape[0] for w in want], what
    for i, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), (what, i, int(np.count_nonzero(g != w)), np.argwhere(g != w)[0].tolist())


def cat(parts):
    return np.concatenate(parts) if parts else np.zeros((0, 2), np.int16)


@pytest.mark.parametrize("case", sc.CASES, ids=[c["name"] for c in sc.CASES])
def test_case_bit_exact(wants, case):
    want = wants[case["name"]]
    bank, audio, spec = run_gpu(case)
    assert_feeds_equal(audio, want["audio"], case["name"] + " audio")
    assert_feeds_equal(spec, want["spec"], case["name"] + " spectrum")
    check_levels(bank, 0, want, case["name"])


def test_silence_with_the_agc_off_and_with_the_threshold_disabled(wants):
    """the reference's behaviour (include/sdrx.h): getStepValue() stays smootherstep(0) = 0, the delay line runs on"""
    for name in ("agc_off", "threshold_disabled"):
        bank, audio, spec = run_gpu(BY[name])
        assert sum(a.shape[0] for a in audio) > 20000 and not cat(audio).any(), name
        assert bank.audio_active(0) and cat(spec).any(), name


def test_design_products_equal_the_oracle(wants):
    for name in ("default_usb", "lsb", "dsb", "short_history", "long_history", "resample_96k_8k", "threshold_disabled", "gate"):
        case = BY[name]
        nt, taps, filt, inc, hn, gate, thr, vol = wants[name]["design"]
        g = sa.SsbDemodBank([gcfg(case["cfg"])]).design(0)
        assert g[0] == nt and g[3] == inc, name
        assert np.array_equal(g[1].view(np.uint32), taps.view(np.uint32)), name
        used = 4096 if case["cfg"]["dsb"] else 2048
        assert np.array_equal(g[2][:used].view(np.uint32), filt[:used].view(np.uint32)) and filt[:used].any(), name
        assert (g[4], g[5]) == (hn, gate) == (sc.hn_of(case["cfg"]), sc.gate_of(case["cfg"])), name
        assert g[6] == thr and np.float32(g[7]) == np.float32(vol), name


@pytest.mark.parametrize("name", ["gate", "step_down_and_back", "short_history", "dsb", "span8"])
def test_random_splits_equal_one_feed(oracle, name):
    case = BY[name]
    want = sc.run_oracle(oracle, case, splits=[case["n"]])
    one_a, one_s = cat(want["audio"]), cat(want["spec"])
    rng = np.random.default_rng(len(name))
    splits, left = [], case["n"]
    while left > 0:
        m = min(left, int(rng.choice([0, 1, 2, 511, 512, 513, int(rng.integers(1, 2000)), int(rng.integers(1, 40000)), int(rng.integers(1, 40000))])))
        splits.append(m); left -= m
    bank, audio, spec = run_gpu(case, splits)
    assert np.array_equal(cat(audio), one_a) and np.array_equal(cat(spec), one_s), name
    check_levels(bank, 0, want, name)


def read_both(bank, ch):
    return bank.read(ch), bank.read_spectrum(ch)


def _mixed(names, wants):
    cases = [BY[n] for n in names]
    bank = sa.SsbDemodBank([gcfg(c["cfg"]) for c in cases])
    got = feed_rounds(bank, [sc.cut(sc.inputs(c), c["splits"]) for c in cases], read_both)
    for c, case in enumerate(cases):
        want = wants[case["name"]]
        assert_feeds_equal([g[0] for g in got[c]], want["audio"], case["name"] + " audio")
        assert_feeds_equal([g[1] for g in got[c]], want["spec"], case["name"] + " spectrum")
        check_levels(bank, c, want, case["name"])


def test_three_mixed_channels_in_one_handle(wants):
    _mixed(["dsb", "short_history", "agc_off"], wants)


def test_seventeen_mixed_channels_in_one_handle(wants):
    """17 rows cross the 16-rows-per-wave tile of psum_rows; configurations and lengths differ per channel"""
    names = [c["name"] for c in sc.CASES if c["name"] not in ("long_history", "first_block_only", "splits_edges")]
    assert len(names) == 17
    _mixed(names, wants)


def test_reset_restores_a_fresh_handle(wants):
    for name in ("gate", "short_history"):
        case = BY[name]
        want = wants[name]
        bank, first, _ = run_gpu(case)
        assert_feeds_equal(first, want["audio"], name)
        # leave the counters, the histories and a spectrum group half way: 5000 more inputs of a strong tone, then 777
        bank.feed([sc.inputs(BY["default_usb"])[: 2 * 5000]])
        bank.feed([sc.inputs(case)[: 2 * 777]])
        bank.reset()
        assert bank.levels(0) == (0.0, 0.0, 0.0, 0) and not bank.audio_active(0)
        _, again, spec = run_gpu(case, bank=bank)
        assert_feeds_equal(again, want["audio"], name + " after reset")
        assert_feeds_equal(spec, want["spec"], name + " spectrum after reset")
        check_levels(bank, 0, want, name + " after reset")


def test_levels_reset_flag_and_empty_feed(wants):
    case = sc.CASES[0]
    bank, _, _ = run_gpu(case)
    m, s, p, n = bank.levels(0, reset=True)
    assert n == wants[case["name"]]["count"] and s > 0 and p > 0 and m > 0
    assert bank.levels(0) == (m, 0.0, 0.0, 0)              # getMagSqLevels zeroes sum, peak and count; m_magsq stays
    bank.feed([np.zeros(0, np.int16)])
    assert bank.read(0).shape[0] == 0 and bank.last_dev(0)[1] == 0 and bank.spectrum_last_dev(0)[1] == 0
    assert bank.levels(0) == (m, 0.0, 0.0, 0) and bank.audio_active(0)


def test_feed_dev_and_last_dev_match_feed(wants):
    import torch
    case = BY["resample_96k_8k"]
    want = wants[case["name"]]
    bank = sa.SsbDemodBank([gcfg(case["cfg"])])
    for x, w, ws in zip(sc.cut(sc.inputs(case), case["splits"]), want["audio"], want["spec"]):
        t = torch.from_numpy(x.copy()).cuda() if x.size else torch.zeros(2, dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        bank.feed_dev([t.data_ptr()], [x.size // 2])
        ptr, n = bank.last_dev(0)
        sptr, ns = bank.spectrum_last_dev(0)
        assert n == w.shape[0] and ns == ws.shape[0]
        assert np.array_equal(bank.read(0), w) and np.array_equal(bank.read_spectrum(0), ws)
        assert (ptr != 0) or n == 0
        assert n == 0 or (sptr != 0 and sptr != ptr)
        bank.sync()
    check_levels(bank, 0, want, case["name"])


def test_accessors():
    """the accessor set of tests/test_handle_accessors_gpu.py, on this family"""
    import torch
    case = sc.CASES[0]
    h = sa.SsbDemodBank([gcfg(dict(case["cfg"], agc_time_log2=2))] * 3)     # hn = 192: the delay line hands out audio within the feed
    x = sc.inputs(case)[: 2 * 5000]

    def feed():
        h.feed([x, x, x])
        return h.read(1)

    h.reset()
    own_out = feed()
    assert own_out.shape[0] == 3584 and own_out.any()       # 5000 inputs at 60000 -> 48000: 4000 resampled, seven blocks of 512
    assert h.get_timing()[1] == 0                           # timing off: a feed is not counted
    ll = h.last_launch()
    # at most 5000 / 1 + 4 resampler outputs per channel plus one held-back block of up to 1024, 256 per workgroup; no LDS
    assert ll["kernel"] == "ssb_out_kernel" and ll["block"] == 256 and ll["grid"] == 3 * ((5000 + 1024 + 255) // 256), ll
    assert ll["lds_bytes"] == 0, ll
    h.set_timing(True)
    feed()
    ms, n = h.get_timing(reset=False)
    assert n == 1 and ms > 0, (ms, n)
    assert h.get_timing(reset=False) == (ms, n)
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
    h.close()


def tail_cfgs(cfg):
    """the parent's route to this audio: sdrx_backend_* with the SSB filter, then sdrx_audiotail_* kind 1, same derived parameters"""
    rate = np.float32(cfg["audio_rate"])
    band, low, usb = np.float32(cfg["rf_bandwidth"]), np.float32(cfg["low_cutoff"]), True
    if band < 0:
        band, low, usb = -band, -low, False
    if band < 100:
        band, low = np.float32(100.0), np.float32(0.0)
    be = sa.BackendCfg(in_rate=cfg["in_rate"], nco_freq=cfg["nco_freq"], out_rate=cfg["audio_rate"], interp_cutoff=float(band * np.float32(1.5)),
                       taps_per_phase=2.0, filt_mode=4 if cfg["dsb"] else (2 if usb else 3), f1=float(low / rate),
                       f2=float((np.float32(2.0) * band) / rate if cfg["dsb"] else band / rate), discri=0, fm_scaling=1.0)
    at = sa.AudioTailCfg(kind=1, audio_rate=cfg["audio_rate"], volume=float(np.float32(cfg["volume"] / 4.0)), agc_active=cfg["agc"],
                         agc_nb_samples=sc.hn_of(cfg), agc_threshold_enable=int(cfg["agc_power_threshold"] != 100), agc_gate=sc.gate_of(cfg),
                         agc_clamping=cfg["agc_clamping"], agc_threshold=10.0 ** (cfg["agc_power_threshold"] / 10.0) * (32768.0 * 32768.0))
    return be, at


MONO = [c["name"] for c in sc.CASES if not (c["cfg"]["audio_binaural"] or c["cfg"]["audio_mute"])]


@pytest.mark.parametrize("name", MONO)
def test_left_channel_equals_backend_plus_audiotail(name):
    """independent of tests/ssb_oracle.c: BackendBank -> AudioTail (kind 1) give the left (= right) channel, feed by feed"""
    case = BY[name]
    bcfg, tcfg = tail_cfgs(case["cfg"])
    be, tail = sa.BackendBank([bcfg]), sa.AudioTail([tcfg])
    bank = sa.SsbDemodBank([gcfg(case["cfg"])])
    total = 0
    for x in sc.cut(sc.inputs(case), case["splits"]):
        bank.feed([x])
        got = bank.read(0)
        be.feed([x])
        sb = be.read(0)
        want = tail.feed([sb])[0] if sb.size else np.zeros(0, np.int16)
        assert got.shape[0] == want.size and np.array_equal(got[:, 0], want) and np.array_equal(got[:, 1], want), (name, got.shape, want.size)
        total += got.shape[0]
    assert total >= 512, total


def test_feed_bank_device_handover(oracle):
    """61.44 MS/s stream, 4 channels at req_rate 48000, 3 000 000 samples in three uneven feeds: audio and spectrum of feed_bank
    equal the oracle on the bank oracle's output; the next bank.feed queued right behind does not disturb them"""
    fs, n_ch = 61_440_000, 4
    fcs = [int(-24_000_000 + c * 13_000_000 + 1371 * c) for c in range(n_ch)]
    bank_dev = sa.ChannelizerBank(fs, [48000] * n_ch, fcs)
    cfgs, oras, chains = [], [], []
    for c in range(n_ch):
        modes, out_rate, ofs = bank_dev.info(c)
        assert out_rate >= 48000
        cfg = sc._cfg(out_rate, 48000, nco_freq=-ofs, agc=1, agc_time_log2=3 + c, dsb=int(c == 3), span_log2=1 + 2 * c,
                      rf_bandwidth=-3000.0 if c == 1 else 3000.0, low_cutoff=-300.0 if c == 1 else 300.0, audio_binaural=int(c == 2))
        cfgs.append(gcfg(cfg)); oras.append(sc.OracleSsb(oracle, cfg)); chains.append(orc.Chain(modes))
    ssb = sa.SsbDemodBank(cfgs)
    x = synth.mix(3_000_000, 78, 3000, 1500, 1)
    cuts = ((0, 1_000_001), (1_000_001, 2_150_000), (2_150_000, 3_000_000))
    segs = [x[2 * a: 2 * b] for a, b in cuts]
    total = [0] * n_ch

    def check(seg):
        for c in range(n_ch):
            wa, ws = oras[c].feed(chains[c].feed(seg))
            ga, gs = ssb.read(c), ssb.read_spectrum(c)
            assert ga.shape == wa.shape and gs.shape == ws.shape, (c, ga.shape, wa.shape)
            assert np.array_equal(ga, wa) and np.array_equal(gs, ws), c
            total[c] += ga.shape[0]

    for i, seg in enumerate(segs):
        bank_dev.feed(seg)                   # from the second round on this overwrites the queues the demodulators were handed
        if i:
            check(segs[i - 1])               # ... before their results for the previous feed are looked at
        ssb.feed_bank(bank_dev)
        for c in range(n_ch):
            bank_dev.skip(c)
    check(segs[-1])
    for c in range(n_ch):
        m, s, p, n = oras[c].levels()
        assert total[c] >= 1024, (c, total)
        assert ssb.levels(c)[0] == m and ssb.levels(c)[2] == p and ssb.levels(c)[3] == n and ssb.audio_active(c) == oras[c].audio_active(), c
