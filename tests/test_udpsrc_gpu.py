"""GPU: the UDPSrc bank (sdrx_udpsrc_*) against the oracle (tests/udpsrc_oracle.c): every payload sample, spectrum Sample,
m_inMagsq, the squelch flag and counters and the running total, bit for bit for formats 0, 1, 8, 9 and 10.  Formats 2 and 3
scale std::arg = atan2f, which the device evaluates as the fdlibm float routines do (udp_atan2f, include/sdrx.h): the same bits
as the oracle's where the host's libm is a glibc up to 2.40, within 2 ulp of any other.  The rule below dates from a device
atan2 that was a few ulp from the host's -- with |d * gain| < 8 the float's ulp is at most 2^-21, four ulp times 32768 is 2^-4
of an LSB, so each int16 equals the oracle's or differs by exactly 1 modulo 2^16 -- and stays as the bound: the tests allow no
difference above 1, at most 1/4 of a case's open samples differing, and demand exact zeros on closed samples.  The named cases of
tests/udpsrc_cases.py (the AM formats with MagAGC off and on, the power crossing its threshold both ways), random splits, banks of
1, 3 and 17 mixed channels, reset, the device hand-over from the channelizer
bank, the design products, the accessors, and -- independent of that oracle -- format 0 against sdrx_backend_*."""
import numpy as np
import pytest

import sdrangel_amd as sa
from tests import oracle_py as orc
from tests import synth
from tests import udpsrc_cases as uc
from tests.demod_mixed import feed_rounds

pytestmark = pytest.mark.gpu
BY = {c["name"]: c for c in uc.CASES}


@pytest.fixture(scope="module")
def oracle():
    return uc.build_oracle()


@pytest.fixture(scope="module")
def wants(oracle):
    """every named case through the oracle once, shared (and left unchanged) by the tests below"""
    return {c["name"]: uc.run_oracle(oracle, c) for c in uc.CASES}


def gcfg(cfg, agc=None) -> sa.UdpSrcCfg:
    return sa.UdpSrcCfg(in_rate=int(cfg[0]), nco_freq=int(cfg[1]), output_sample_rate=float(cfg[2]), sample_format=int(cfg[3]),
                        rf_bandwidth=float(cfg[4]), fm_deviation=int(cfg[5]), gain=float(cfg[6]), squelch_db=int(cfg[7]), squelch_gate=int(cfg[8]),
                        squelch_enabled=int(cfg[9]), agc=int(cfg[10]) if agc is None else agc)


def check_state(bank, ch, want, what):
    got = (bank.in_magsq(ch), bank.squelch_open(ch), *bank.squelch_counts(ch), bank.total(ch))
    print(f"{what}: in_magsq {got[0]!r} (oracle {want['in_magsq']!r}), open {got[1]}, counts {got[2:4]}, total {got[4]}")
    assert got == (want["in_magsq"], want["open"], want["open_count"], want["close_count"], want["total"]), (what, got)


def run_gpu(case, splits=None, bank=None):
    bank = bank or sa.UdpSrcBank([gcfg(case["cfg"])])
    feeds, specs = [], []
    for x in uc.cut(uc.inputs(case), splits or case["splits"]):
        bank.feed([x])
        feeds.append(bank.read(0)); specs.append(bank.read_spectrum(0))
    return bank, feeds, specs


def assert_payload(fmt, got, want, mask, what):
    """the exactness rule of the module docstring on one stream; returns (differing, open) sample counts for formats 2 and 3"""
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if fmt not in (uc.NFM, uc.NFM_MONO):
        assert np.array_equal(got, want), (what, int(np.count_nonzero(got != want)), np.flatnonzero((got != want).reshape(got.shape[0], -1).any(axis=1))[:4])
        return 0, int(mask.sum())
    diff = (got.astype(np.int32) - want.astype(np.int32)).astype(np.int16)          # modulo 2^16
    assert np.abs(diff.astype(np.int32)).max(initial=0) <= 1, (what, int(np.abs(diff.astype(np.int32)).max()))
    assert not got[~mask].any(), what                                               # closed samples are exactly 0
    if fmt == uc.NFM:
        assert np.array_equal(got[:, 0], got[:, 1]), what
    n_diff = int(np.count_nonzero(diff.reshape(diff.shape[0], -1).any(axis=1)))
    n_open = int(mask.sum())
    assert 4 * n_diff <= n_open, (what, n_diff, n_open)
    return n_diff, n_open


def assert_streams(case, got_feeds, got_specs, want, what, per_feed=True):
    fmt = case["cfg"][3]
    if per_feed:
        assert [g.shape[0] for g in got_feeds] == [w.shape[0] for w in want["feeds"]], what
    got, spec = np.concatenate(got_feeds), np.concatenate(got_specs)
    n_diff, n_open = assert_payload(fmt, got, np.concatenate(want["feeds"]), np.concatenate(want["masks"]), what)
    assert np.array_equal(spec, np.concatenate(want["specs"])), what
    if fmt in (uc.NFM, uc.NFM_MONO):
        print(f"{what}: format {fmt}: {n_diff} of {n_open} open samples differ by 1 (share {n_diff / max(n_open, 1):.4f})")


@pytest.mark.parametrize("case", uc.CASES, ids=[c["name"] for c in uc.CASES])
def test_case_against_the_oracle(wants, case):
    want = wants[case["name"]]
    bank, feeds, specs = run_gpu(case)
    assert_streams(case, feeds, specs, want, case["name"])
    check_state(bank, 0, want, case["name"])
    assert bank.sample_bytes(0) == uc.elem_bytes(case["cfg"][3])


def test_design_products_equal_the_oracle(oracle):
    for name in ("iq16_burst_gate5", "iq16_burst_gate0", "am_nondyadic_62500", "iq16_step1_48k", "ambpf_r96k_to_44k1", "nfm_float_rate", "amnodc_burst", "am_agc_cross",
                 "amnodc_agc_cross", "ambpf_agc_cross", "am_agc_nondyadic_62500"):
        case = BY[name]
        o = uc.OracleUdp(oracle, case["cfg"]).design()
        g = sa.UdpSrcBank([gcfg(case["cfg"])]).design(0)
        assert g["ntaps"] == o["ntaps"] == 72 and g["nco_inc"] == o["nco_inc"], name
        assert np.array_equal(g["taps"], o["taps"].astype(np.float64)), name
        assert np.array_equal(g["bandpass"], o["bandpass"].astype(np.float64)), name
        assert g["windows"] == o["windows"] and g["gate"] == o["gate"] == uc.gate_samples(case["cfg"]) and g["release"] == o["release"], name
        assert g["agc"] == o["agc"] and g["agc_threshold"] == o["agc_threshold"] == g["level"] * 2.0 ** 23, name
        assert g["level"] == o["level"] and np.float32(g["fm_scaling"]) == np.float32(o["fm_scaling"]) and np.float32(g["step"]) == np.float32(o["step"]), name
    assert sa.UdpSrcBank([gcfg(BY["iq16_burst_gate5"]["cfg"])]).design(0)["windows"] == [80, 40, 80]
    # history rate / 5, steps rate / 20, step-down delay rate * gate / 100 (gate 0 counts as 1), gate rate * 0.05
    assert sa.UdpSrcBank([gcfg(BY["amnodc_agc_cross"]["cfg"])]).design(0)["agc"] == [1600, 400, 400, 400]
    assert sa.UdpSrcBank([gcfg(BY["ambpf_agc_cross"]["cfg"])]).design(0)["agc"] == [1600, 400, 80, 400]


@pytest.mark.parametrize("name", ["iq16_burst_gate5", "iq24_burst", "nfm_burst", "nfmmono_burst_gate5", "am_burst", "amnodc_burst", "ambpf_burst",
                                  "am_nondyadic_62500", "iq16_burst_gate0", "am_agc_cross", "amnodc_agc_cross", "ambpf_agc_cross",
                                  "am_agc_squelched"])
def test_random_splits_equal_one_feed(oracle, name):
    case = BY[name]
    want = uc.run_oracle(oracle, case, splits=[case["n"]])
    rng = np.random.default_rng(len(name))
    for trial in range(2):
        splits, left = [0, 1, 31, 32, 33], case["n"] - 97
        while left > 0:
            m = min(left, int(rng.choice([0, 1, 2, 31, 32, 33, int(rng.integers(1, 300)), int(rng.integers(1, 3000)), int(rng.integers(1, 8000))])))
            splits.append(m); left -= m
        rng.shuffle(splits)
        bank, feeds, specs = run_gpu(case, splits)
        assert_streams(case, feeds, specs, want, f"{name} trial {trial}", per_feed=False)
        check_state(bank, 0, want, f"{name} trial {trial}")


def read_both(bank, ch):
    return bank.read(ch), bank.read_spectrum(ch)


#: seventeen channels: all seven formats, every gate setting, four rates, the three AM formats with the AGC off and on
MIX17 = ["iq16_burst_gate5", "iq24_burst", "nfm_burst", "nfmmono_burst_gate5", "am_burst", "amnodc_burst", "ambpf_burst", "iq16_burst_gate0",
         "iq16_release_boundary", "amnodc_small_feeds", "ambpf_small_feeds", "nfm_float_rate", "am_nondyadic_62500", "ambpf_r96k_to_44k1",
         "am_agc_cross", "amnodc_agc_cross", "ambpf_agc_cross"]


@pytest.mark.parametrize("names", [["ambpf_agc_default"], ["iq24_burst", "nfm_burst", "amnodc_agc_cross"], MIX17], ids=["1", "3", "17"])
def test_mixed_channels_in_one_handle(wants, names):
    cases = [BY[n] for n in names]
    if len(names) == 17:
        assert {c["cfg"][3] for c in cases} == set(uc.FORMATS)
        assert {(c["cfg"][3], c["cfg"][10]) for c in cases} >= {(8, 0), (8, 1), (9, 0), (9, 1), (10, 0), (10, 1)}
    # formats 0 .. 3 never feed the AGC: the flag is accepted and changes nothing there
    bank = sa.UdpSrcBank([gcfg(c["cfg"], agc=1 if c["cfg"][3] < 8 and i % 2 == 0 else None) for i, c in enumerate(cases)])
    got = feed_rounds(bank, [uc.cut(uc.inputs(c), c["splits"]) for c in cases], read_both, idle=lambda bank, c: bank.last_dev(c)[1])
    for c, case in enumerate(cases):
        want = wants[case["name"]]
        assert_streams(case, [g[0] for g in got[c]], [g[1] for g in got[c]], want, case["name"])
        check_state(bank, c, want, case["name"])


def test_reset_restores_a_fresh_handle(wants):
    for name in ("amnodc_burst", "ambpf_agc_cross", "nfm_burst", "am_agc_nondyadic_62500"):
        case = BY[name]
        want = wants[name]
        bank, feeds, specs = run_gpu(case)
        assert_streams(case, feeds, specs, want, name)
        bank.feed([uc.inputs(case)[: 2 * 777]])             # leave the squelch, the averages and the ring somewhere else
        assert bank.total(0) > want["total"]
        bank.reset()
        assert (bank.in_magsq(0), bank.squelch_open(0), bank.squelch_counts(0), bank.total(0)) == (0.0, False, (0, 0), 0)
        _, feeds, specs = run_gpu(case, bank=bank)
        assert_streams(case, feeds, specs, want, name + " after reset")
        check_state(bank, 0, want, name + " after reset")


def test_payloads_cut_the_running_stream_into_datagrams(wants):
    for name, per in (("iq16_burst_gate1", 128), ("iq24_burst", 64), ("ambpf_burst", 256)):
        case = BY[name]
        bank = sa.UdpSrcBank([gcfg(case["cfg"])])
        grams = []
        for x in uc.cut(uc.inputs(case), case["splits"]):
            bank.feed([x])
            grams += bank.payloads(0)
        stream = np.concatenate(wants[name]["feeds"]).tobytes()
        assert len(grams) == bank.total(0) // per == wants[name]["total"] // per and len(grams) >= 7, name
        assert b"".join(grams) == stream[: len(grams) * 512], name


def test_feed_dev_and_last_dev_match_feed(wants):
    import torch
    case = BY["ambpf_r96k_to_44k1"]
    want = wants[case["name"]]
    bank = sa.UdpSrcBank([gcfg(case["cfg"])])
    for x, w in zip(uc.cut(uc.inputs(case), case["splits"]), want["feeds"]):
        t = torch.from_numpy(x.copy()).cuda() if x.size else torch.zeros(2, dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        bank.feed_dev([t.data_ptr()], [x.size // 2])
        ptr, n = bank.last_dev(0)
        assert n == w.shape[0] == bank.spectrum_last_dev(0)[1]
        assert np.array_equal(bank.read(0), w)
        assert (ptr != 0) or n == 0
        bank.sync()
    check_state(bank, 0, want, case["name"])


def test_accessors():
    """the accessor set of tests/test_handle_accessors_gpu.py, on this family"""
    import torch
    case = BY["ambpf_burst"]
    h = sa.UdpSrcBank([gcfg(case["cfg"])] * 3)
    x = uc.inputs(case)[: 2 * 6000]

    def feed():
        h.feed([x, x, x])
        return h.read(1)

    h.reset()
    own_out = feed()
    assert own_out.size == 1000
    assert h.get_timing()[1] == 0                           # timing off: a feed is not counted
    ll = h.last_launch()
    # 6000 inputs at 48000 -> 8000: at most 6000 / 6 + 4 samples per channel, 256 per workgroup; 151 Real taps and a window of
    # 256 + 300 double Bandpass inputs in LDS
    assert ll["kernel"] == "udp_out_kernel" and ll["block"] == 256 and ll["grid"] == 3 * ((1004 + 255) // 256), ll
    assert ll["lds_bytes"] == 151 * 4 + 556 * 8, ll
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
    h.close()


@pytest.mark.parametrize("rates", [(48000, 8000), (48000, 48000), (96000, 48000)])
def test_format0_equals_the_backend_output(rates):
    """independent of tests/udpsrc_oracle.c: format 0 with the squelch disabled and gain 1 is (qint16) of the resampler output,
    and so are the spectrum Samples.  sdrx_backend_* has no starting distance in its public configuration: it starts at 0, emits
    one output for the very first input and leaves the distance at step - 1.  UDPSrc starts at step, whose first `-= 1.0`
    leaves step - 1 as well, and for these integer steps every later operation is exact -- so the back-end's stream without its
    first output is the stream UDPSrc's front produces.  The comparison is made on that shifted stream.  At step 1 both emit
    for every input from the first one on, at phase 0 (the back-end's negative phase is clamped to 0): no shift there."""
    in_rate, rate = rates
    sig = {"kind": "nfm", "f0": 1000.0, "dev": 2000.0, "fa": 700.0, "amp": 9000.0}
    case = {"cfg": uc._cfg(in_rate, rate, nco_freq=-1000, enabled=0, gate=0, rf=6000.0), "sig": sig, "n": 9000, "seed": 77, "splits": uc._nc._ragged(9000, 77)}
    be = sa.BackendBank([sa.BackendCfg(in_rate=in_rate, nco_freq=-1000, out_rate=rate, interp_cutoff=3000.0, taps_per_phase=4.5, filt_mode=0,
                                       f1=0.0, f2=0.0, discri=0, fm_scaling=1.0)])
    bank = sa.UdpSrcBank([gcfg(case["cfg"])])
    got, spec, ref = [], [], []
    for x in uc.cut(uc.inputs(case), case["splits"]):
        bank.feed([x]); be.feed([x])
        got.append(bank.read(0)); spec.append(bank.read_spectrum(0)); ref.append(be.read(0))
    got, spec, ref = np.concatenate(got), np.concatenate(spec), np.concatenate(ref).reshape(-1, 2)[(0 if in_rate == rate else 1):]
    assert got.shape[0] in (ref.shape[0], ref.shape[0] - 1) and got.shape[0] >= 9000 * rate // in_rate - 1
    want = ref[: got.shape[0]].astype(np.int16)             # |ci| < 32768 here: truncation toward zero, as cvttss2si
    assert np.abs(ref).max() < 32767 and want.any()
    assert np.array_equal(got, want) and np.array_equal(spec, want)


def test_feed_bank_device_handover(oracle):
    """61.44 MS/s stream, 4 channels at req_rate 48000, 1 200 000 samples in two uneven feeds: the payload of feed_bank equals the
    oracle on the bank oracle's output (one format per channel), the squelch opens in every channel; the next bank.feed queued
    right behind does not disturb it"""
    fs, n_ch = 61_440_000, 4
    fcs = [int(-24_000_000 + c * 13_000_000 + 1371 * c) for c in range(n_ch)]
    bank_dev = sa.ChannelizerBank(fs, [48000] * n_ch, fcs)
    fmts = [uc.IQ16, uc.AM_BPF_MONO, uc.AM_NODC_MONO, uc.IQ24]
    cfgs, oras, chains = [], [], []
    for c in range(n_ch):
        modes, out_rate, ofs = bank_dev.info(c)
        assert out_rate >= 48000
        cfg = (out_rate, -ofs, 8000.0, fmts[c], 5000.0, 2500, 1.0, -90, c % 2, 1, c % 2)
        cfgs.append(gcfg(cfg)); oras.append(uc.OracleUdp(oracle, cfg)); chains.append(orc.Chain(modes))
    udp = sa.UdpSrcBank(cfgs)
    x = synth.mix(1_200_000, 78, 3000, 1500, 1)
    cuts = ((0, 500_001), (500_001, 1_200_000))
    segs = [x[2 * a: 2 * b] for a, b in cuts]
    heard, heard_want = [False] * n_ch, [False] * n_ch

    def check(seg):
        for c in range(n_ch):
            want, wspec = oras[c].feed(chains[c].feed(seg))
            got = udp.read(c)
            assert got.shape == want.shape and got.shape[0] > 0, (c, got.shape, want.shape)
            assert np.array_equal(got, want) and np.array_equal(udp.read_spectrum(c), wspec), c
            heard[c] = heard[c] or bool(got.any())
            heard_want[c] = heard_want[c] or bool(want.any())

    for i, seg in enumerate(segs):
        bank_dev.feed(seg)                   # the second round overwrites the queues the channels were handed
        if i:
            check(segs[i - 1])               # ... before their results for the previous feed are looked at
        udp.feed_bank(bank_dev)
        for c in range(n_ch):
            bank_dev.skip(c)
    check(segs[-1])
    for c in range(n_ch):
        st = oras[c].state()
        assert st["open"] and udp.squelch_open(c) and heard[c] == heard_want[c], c
        # the carriers have a constant envelope: behind the 300 Hz high-pass edge of the Bandpass format 10 rounds to 0 in the oracle too
        assert heard[c] or fmts[c] == uc.AM_BPF_MONO, c
        assert (udp.in_magsq(c), udp.total(c)) == (st["in_magsq"], st["total"]), c
