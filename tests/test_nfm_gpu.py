"""GPU: the NFM demodulator bank (sdrx_nfm_*) against the oracle (tests/nfm_oracle.c), every audio sample of every channel, the
moving average, peak, count and squelch state bit for bit: the named cases of tests/nfm_cases.py, random splits, 16 mixed
channels in one handle, reset, the device hand-over from the channelizer bank, the accessors, and -- independent of that
oracle -- the composition of older handles, sdrx_backend_* feeding sdrx_audiotail_* kind 0."""
import numpy as np
import pytest

import sdrangel_amd as sa
from tests import nfm_cases as nc
from tests import oracle_py as orc
from tests import synth

pytestmark = pytest.mark.gpu
BY = {c["name"]: c for c in nc.CASES}


@pytest.fixture(scope="module")
def oracle():
    return nc.build_oracle()


@pytest.fixture(scope="module")
def wants(oracle):
    """every named case through the oracle once, shared (and left unchanged) by the tests below"""
    return {c["name"]: nc.run_oracle(oracle, c) for c in nc.CASES}


def gcfg(cfg) -> sa.NfmCfg:
    return sa.NfmCfg(in_rate=int(cfg[0]), nco_freq=int(cfg[1]), audio_rate=int(cfg[2]), rf_bandwidth=float(cfg[3]), af_bandwidth=float(cfg[4]),
                     fm_deviation=int(cfg[5]), volume=float(cfg[6]), squelch=float(cfg[7]), squelch_gate=int(cfg[8]), audio_mute=int(cfg[9]))


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
    bank = bank or sa.NfmDemodBank([gcfg(case["cfg"])])
    feeds = []
    for x in nc.cut(nc.inputs(case), splits or case["splits"]):
        bank.feed([x])
        feeds.append(bank.read(0))
    return bank, feeds


def assert_feeds_equal(got, want, what):
    assert [g.size for g in got] == [w.size for w in want], what
    for i, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), (what, i, int(np.count_nonzero(g != w)), int(np.flatnonzero(g != w)[0]))


@pytest.mark.parametrize("case", nc.CASES, ids=[c["name"] for c in nc.CASES])
def test_case_bit_exact(wants, case):
    want = wants[case["name"]]
    bank, got = run_gpu(case)
    assert_feeds_equal(got, want["feeds"], case["name"])
    check_levels(bank, 0, want, case["name"])


def test_design_products_equal_the_oracle(oracle):
    for name in ("default_60k", "nondyadic_62500", "step1_48k", "r96k_to_44k1", "gate60_clamped", "wide_25k", "level_edge"):
        case = BY[name]
        o = nc.OracleNfm(oracle, case["cfg"])
        nt, taps, bp, inc, lvl, gate = o.design()
        g = sa.NfmDemodBank([gcfg(case["cfg"])]).design(0)
        assert g[0] == nt == 72 and g[3] == inc, name
        assert np.array_equal(g[1].view(np.uint32), taps.view(np.uint32)), name
        assert np.array_equal(g[2].view(np.uint32), bp.view(np.uint32)), name
        assert np.float32(g[4]) == np.float32(lvl)
        assert g[5] == gate == nc.gate_samples(case["cfg"]), name


@pytest.mark.parametrize("name", ["burst_gate5", "burst_gate1", "nondyadic_62500", "gate60_clamped"])
def test_random_splits_equal_one_feed(oracle, name):
    case = BY[name]
    want = nc.run_oracle(oracle, case, splits=[case["n"]])
    one = np.concatenate(want["feeds"])
    rng = np.random.default_rng(len(name))
    for trial in range(2):
        splits, left = [], case["n"]
        while left > 0:
            m = min(left, int(rng.choice([0, 1, 2, 31, 32, 33, int(rng.integers(1, 2000)), int(rng.integers(1, 40000)), int(rng.integers(1, 40000))])))
            splits.append(m); left -= m
        bank, got = run_gpu(case, splits)
        got = np.concatenate(got)
        assert got.size == one.size and np.array_equal(got, one), (name, trial)
        check_levels(bank, 0, want, f"{name} trial {trial}")


def test_sixteen_mixed_channels_in_one_handle(wants):
    cases = list(nc.CASES)
    assert len(cases) == 16
    bank = sa.NfmDemodBank([gcfg(c["cfg"]) for c in cases])
    cuts = [nc.cut(nc.inputs(c), c["splits"]) for c in cases]
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
        check_levels(bank, c, want, case["name"])


def test_reset_restores_a_fresh_handle(wants):
    for name in ("burst_gate1", "nondyadic_62500"):
        case = BY[name]
        want = wants[name]
        bank, first = run_gpu(case)
        assert_feeds_equal(first, want["feeds"], name)
        # leave the squelch open and the histories half full: 5000 more inputs of a strong carrier (delay 2400 or 480, ring 300)
        bank.feed([nc.inputs(BY["default_60k"])[: 2 * 5000]])
        bank.feed([nc.inputs(case)[: 2 * 777]])
        bank.reset()
        assert bank.levels(0) == (0.0, 0.0, 0.0, 0) and not bank.squelch_open(0)
        _, again = run_gpu(case, bank=bank)
        assert_feeds_equal(again, want["feeds"], name + " after reset")
        check_levels(bank, 0, want, name + " after reset")


def test_levels_reset_flag_and_empty_feed(wants):
    case = nc.CASES[0]
    bank, _ = run_gpu(case)
    m, s, p, n = bank.levels(0, reset=True)
    assert n == wants[case["name"]]["count"] and s > 0 and p > 0 and m > 0
    assert bank.levels(0) == (m, 0.0, 0.0, 0)              # getMagSqLevels zeroes sum, peak and count; the moving average stays
    bank.feed([np.zeros(0, np.int16)])
    assert bank.read(0).size == 0 and bank.last_dev(0)[1] == 0
    assert bank.levels(0) == (m, 0.0, 0.0, 0) and bank.squelch_open(0)


def test_feed_dev_and_last_dev_match_feed(wants):
    import torch
    case = BY["r96k_to_44k1"]
    want = wants[case["name"]]
    bank = sa.NfmDemodBank([gcfg(case["cfg"])])
    for x, w in zip(nc.cut(nc.inputs(case), case["splits"]), want["feeds"]):
        t = torch.from_numpy(x.copy()).cuda() if x.size else torch.zeros(2, dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        bank.feed_dev([t.data_ptr()], [x.size // 2])
        ptr, n = bank.last_dev(0)
        assert n == w.size
        assert np.array_equal(bank.read(0), w)
        assert (ptr != 0) or n == 0
        bank.sync()
    check_levels(bank, 0, want, case["name"])


def test_accessors():
    """the accessor set of tests/test_handle_accessors_gpu.py, on this family"""
    import torch
    case = nc.CASES[0]
    h = sa.NfmDemodBank([gcfg(case["cfg"])] * 3)
    x = nc.inputs(case)[: 2 * 5000]

    def feed():
        h.feed([x, x, x])
        return h.read(1)

    h.reset()
    own_out = feed()
    assert own_out.size > 0
    assert h.get_timing()[1] == 0                           # timing off: a feed is not counted
    ll = h.last_launch()
    # 5000 inputs at 60000 -> 48000: at most 5000 / 1 + 4 audio samples per channel, 256 per workgroup; 151 taps and a window
    # of 256 + 300 Bandpass inputs in LDS
    assert ll["kernel"] == "nfm_out_kernel" and ll["block"] == 256 and ll["grid"] == 3 * ((5000 + 255) // 256), ll
    assert ll["lds_bytes"] == (151 + 556) * 4, ll
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


@pytest.mark.parametrize("name", ["burst_gate5", "burst_gate1", "default_60k"])
def test_audio_equals_backend_plus_audiotail(name):
    """independent of tests/nfm_oracle.c: BackendBank (filt_mode 0, discri 0) -> AudioTail (kind 0) with the same derived
    parameters produce the same audio, feed by feed"""
    case = BY[name]
    cfg = case["cfg"]
    rate = int(cfg[2])
    be = sa.BackendBank([sa.BackendCfg(in_rate=int(cfg[0]), nco_freq=int(cfg[1]), out_rate=rate,
                                       interp_cutoff=float(np.float32(cfg[3]) / np.float32(2.2)), taps_per_phase=4.5, filt_mode=0, f1=0.0, f2=0.0,
                                       discri=0, fm_scaling=1.0)])
    tail = sa.AudioTail([sa.AudioTailCfg(kind=0, audio_rate=rate, volume=float(cfg[6]),
                                         fm_scaling=float(np.float32(8.0) * np.float32(rate) / np.float32(cfg[5])),
                                         squelch_level=float(np.float32(10.0 ** (float(np.float32(cfg[7])) / 100.0))),
                                         squelch_gate=nc.gate_samples(cfg), af_bandwidth=float(cfg[4]))])
    bank = sa.NfmDemodBank([gcfg(cfg)])
    heard = 0
    for x in nc.cut(nc.inputs(case), case["splits"]):
        bank.feed([x])
        got = bank.read(0)
        be.feed([x])
        want = tail.feed([be.read(0)])[0]
        assert got.size == want.size and np.array_equal(got, want), (name, got.size, want.size)
        heard += int(np.count_nonzero(got))
    assert heard > 20000, heard


def test_feed_bank_device_handover(oracle):
    """61.44 MS/s stream, 4 channels at req_rate 48000, 3 000 000 samples in three uneven feeds: the audio of feed_bank equals
    the oracle on the bank oracle's output, and the squelch opens in every channel; the next bank.feed queued right behind does
    not disturb it"""
    fs, n_ch = 61_440_000, 4
    fcs = [int(-24_000_000 + c * 13_000_000 + 1371 * c) for c in range(n_ch)]
    bank_dev = sa.ChannelizerBank(fs, [48000] * n_ch, fcs)
    cfgs, oras, chains = [], [], []
    for c in range(n_ch):
        modes, out_rate, ofs = bank_dev.info(c)
        assert out_rate >= 48000
        cfg = (out_rate, -ofs, 48000, 12500.0, 3000.0, 2000, 2.0, -900.0, 1 + c % 2, 0)
        cfgs.append(gcfg(cfg)); oras.append(nc.OracleNfm(oracle, cfg)); chains.append(orc.Chain(modes))
    nfm = sa.NfmDemodBank(cfgs)
    x = synth.mix(3_000_000, 78, 3000, 1500, 1)
    cuts = ((0, 1_000_001), (1_000_001, 2_150_000), (2_150_000, 3_000_000))
    segs = [x[2 * a: 2 * b] for a, b in cuts]
    heard = [False] * n_ch

    def check(seg):
        for c in range(n_ch):
            want = oras[c].feed(chains[c].feed(seg))
            got = nfm.read(c)
            assert got.size == want.size and got.size > 0, (c, got.size, want.size)
            assert np.array_equal(got, want), c
            heard[c] = heard[c] or bool(got.any())

    for i, seg in enumerate(segs):
        bank_dev.feed(seg)                   # from the second round on this overwrites the queues the demodulators were handed
        if i:
            check(segs[i - 1])               # ... before their results for the previous feed are looked at
        nfm.feed_bank(bank_dev)
        for c in range(n_ch):
            bank_dev.skip(c)
    check(segs[-1])
    for c in range(n_ch):
        m, s, p, n = oras[c].levels()
        assert oras[c].squelch_open() and nfm.squelch_open(c) and heard[c], c
        assert nfm.levels(c)[0] == m and nfm.levels(c)[2] == p and nfm.levels(c)[3] == n, c
