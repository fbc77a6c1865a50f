"""CPU side of the float edge cases (tests/float_edge_cases.py).

First the preconditions, on the oracle alone: the committed seeds, lengths and scales do drive the oracle into the regime
each GPU test of tests/test_float_edges_gpu.py is about (subnormal outputs, a stuck and a recovering I/Q correction,
conversions outside int32, zeros of both signs), so that those tests cannot pass vacuously.

Then, marked `ref` and skipped where oracle/_ref is absent: on the very same inputs the oracle equals the reference's own
classes compiled from its sources (oracle/ref_shim*.cpp), and the committed fixture tests/golden/fdecim_edges_golden.npz is
what that build produces.  The compiled reference, not the oracle, is the arbiter of these inputs."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import float_edge_cases as fe
from tests import oracle_py as orc
from tests.test_audiotail_gpu import IIR_SPECS, NFM, SSB, bursts
from tests.test_backend_gpu import CFGS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "oracle", "_ref", "libsdrref.so")
GOLDEN = os.path.join(ROOT, "tests", "golden", "fdecim_edges_golden.npz")
needs_ref = pytest.mark.skipif(not os.path.exists(REF), reason="oracle/_ref not built (no reference tree here)")

BE_D2 = dict(in_rate=60000, nco_freq=100, out_rate=48000, interp_cutoff=6000.0, taps_per_phase=4.5, filt_mode=0, f1=0.0, f2=0.0, discri=2, fm_scaling=10.0)


def fd_oracle(kind, L, fc, x):
    o = orc.FDecim(kind, L, fc)
    return np.concatenate([o.process(b) for b in fe.fd_blocks(x)])


def audiotail_input(i, k):
    gap = fe.AT_GAP_LONG if k.get("agc_nb_samples") == 12288 else fe.AT_GAP
    return fe.with_gap(bursts(fe.AT_BURST, 400 + i), gap, bursts(fe.AT_BURST, 500 + i)), gap


def backend_oracle(cfg):
    return orc.Backend(cfg["in_rate"], cfg["nco_freq"], cfg["out_rate"], cfg["interp_cutoff"], cfg["taps_per_phase"],
                       cfg["filt_mode"], cfg["f1"], cfg["f2"], cfg["discri"], cfg["fm_scaling"])


def backend_channels():
    """(configuration, data seed) of the back-end channels: CFGS[0], CFGS[2] and the atan2 discriminator with nco_freq of
    both signs, each on two data seeds"""
    return [(CFGS[0], 800), (CFGS[2], 800)] + [(dict(BE_D2, nco_freq=f), s) for f in (100, -100) for s in fe.BE_SEEDS]


# ------------------------------------------------------------------------------------------------ helpers of the module itself
def test_same_bits_and_subnormal_count():
    f = lambda *u: np.array(u, np.uint32).view(np.float32)
    assert fe.same_bits(f(0x7FC00000, 0, 0x80000000, 1), f(0xFFC00000, 0, 0x80000000, 1))          # NaN of either sign
    assert not fe.same_bits(f(0), f(0x80000000))                                                    # the sign of zero counts
    assert not fe.same_bits(f(1), f(0)) and not fe.same_bits(f(0x7F800000), f(0xFF800000))
    assert not fe.same_bits(f(0x7FC00000), f(0x7F800000)) and not fe.same_bits(f(0, 0), f(0))
    assert fe.subnormal_count(f(0, 0x80000000, 1, 0x807FFFFF, 0x00800000, 0x7FC00000)) == 2
    assert list(fe.ulp_diff(f(0, 0x3F800000, 0x7F800000, 1), f(0x80000000, 0x3F800002, 0x7F800000, 0x80000001))) == [0, 2, 0, 2]
    assert fe.ulp_diff(f(0x7FC00000), f(0x7FC00000))[0] > 1 << 30
    assert fe.subnormal_count(fe.fd_subnormal()) > 0.99 * fe.FD_N and float(np.abs(fe.fd_wrap()).max()) < 3.99


# ------------------------------------------------------------------------------------------------ preconditions (oracle alone)
@pytest.mark.parametrize("L,fc", fe.FD_CASES)
def test_ff_subnormal_input_gives_subnormal_outputs(L, fc):
    y = fd_oracle("ff", L, fc, fe.fd_subnormal())
    assert 2 * fe.subnormal_count(y) >= y.size, (L, fc, fe.subnormal_count(y), y.size)


@pytest.mark.parametrize("L,fc", fe.FD_CASES)
def test_fi_overflow_input_converts_to_zero_and_recovers(L, fc):
    x = fe.fd_overflow()
    assert np.all(np.diff(fe.FD_SPECIAL_AT) >= 2 * 300) and fe.FD_SPECIAL_AT[-1] < fe.FD_N // 4
    y = fd_oracle("fi", L, fc, x)
    if L == 0:                                              # decimate1: output k is input k times 32768
        assert np.array_equal(y[fe.FD_SPECIAL_AT], np.zeros(len(fe.FD_SPECIAL_AT), np.int16))
    last = y[-(y.size // 4):]
    assert np.all(last != 0), (L, fc, int((last == 0).sum()))
    lastf = fd_oracle("ff", L, fc, x)[-(y.size // 4):]
    assert np.all(np.isfinite(lastf)) and np.all(lastf != 0)
    if L >= 3:                                              # in front of that the filters did see inf - inf
        assert np.isnan(fd_oracle("ff", L, fc, x)).any()


def test_fi_wrap_input_wraps_inside_int32():
    x = fe.fd_wrap()
    y = fd_oracle("fi", 0, fe.FC_CEN, x)
    p = x[: y.size].astype(np.float64) * 32768.0
    assert np.abs(p).max() < 2.0 ** 31 and np.abs(p).max() > 3.9 * 32768
    assert np.array_equal(y, np.trunc(p).astype(np.int64).astype(np.int16))     # the low 16 bits


def test_ff_signed_zero_input_gives_zeros_of_both_signs():
    for L, fc in ((0, fe.FC_CEN), (1, fe.FC_INF), (1, fe.FC_SUP)):
        u = fd_oracle("ff", L, fc, fe.fd_signed_zero()).view(np.uint32)
        assert (u == 0x80000000).sum() > 100 and (u == 0).sum() > 100, (L, fc)


def test_iir_silence_settles_in_the_subnormal_range():
    deep = 0
    for i, s in enumerate(IIR_SPECS):
        y = orc.Iir(*s).run(fe.iir_input(70 + i))
        silent = y[fe.IIR_PARTS[0]: fe.IIR_PARTS[0] + fe.IIR_PARTS[1]]
        deep += fe.subnormal_count(silent) >= 1000
        if i < 4:                                           # the feeds are cut where these four emit subnormals
            assert fe.subnormal_count(y[fe.IIR_CUT - 100: fe.IIR_CUT + 100]) == 200, i
    assert deep >= 3
    y = orc.Iir(*fe.IIR_UNSTABLE).run(fe.iir_input(99))
    assert np.isinf(y).any() and np.isnan(y[-1000:]).all()


@pytest.mark.parametrize("c", range(len(fe.FIR_SPECS)))
def test_fir_subnormal_scale(c):
    """the committed scale is the first of 1e-38, 1e-38 / 2, 1e-38 / 4, ... at which half of the outputs are subnormal"""
    ulps = 7136238
    while True:
        y = orc.Fir(*fe.FIR_SPECS[c]).run(fe.subnormals(fe.FIR_N, 50 + c, ulps))
        if 2 * fe.subnormal_count(y) >= y.size:
            break
        ulps //= 2
    assert ulps == fe.FIR_SUBNORMAL_ULPS[c]
    y = orc.Fir(*fe.FIR_SPECS[c]).run(fe.fir_huge())
    assert np.isinf(y).any() and np.isnan(y).any()


def test_iqimb_gap_streams_stick_and_recover():
    xs = fe.iq_streams()
    q = {k: orc.IqImb().process(x)[1::2] for k, x in xs.items()}
    assert np.all(q["stuck"][fe.IQ_SETTLED:] == 0) and np.any(q["stuck"][: fe.IQ_GAP[0]] != 0)
    assert np.all(q["recovers"][fe.IQ_SETTLED:] != 0)
    assert np.count_nonzero(q["control"][fe.IQ_SETTLED:]) > 0.99 * (fe.IQ_N - fe.IQ_SETTLED)
    i_const = orc.IqImb().process(xs["constant"])[0::2]
    assert np.all(i_const[1100:] == 0) and np.any(i_const[:1000] != 0)
    assert all(fe.IQ_GAP[0] < c < fe.IQ_GAP[1] for c in fe.IQ_CUTS[4:5]) and fe.IQ_CUTS[1:4] == [63, 127, 192]


def test_audiotail_streams_carry_audio_on_both_sides_of_the_gap():
    both = 0
    for i, k in enumerate(NFM + SSB):
        x, gap = audiotail_input(i, k)
        assert gap > k.get("agc_nb_samples", 0)
        y = orc.AudioTailOracle(**k).feed(x)
        both += bool(np.any(y[: fe.AT_BURST] != 0) and np.any(y[fe.AT_BURST + gap:] != 0))
    assert both >= 4


def test_backend_silence_meets_the_sign_of_zero_outcomes():
    """discri = 2 is atan2(d.i, d.r) of d = cur * conj(prev).  The resampler starts every output from +0.0 and adds, so in
    silence it emits (+0, +0) whatever signs the NCO product gave the zeros, and d = (+0, +0) -> 0.  Zeros of other signs
    reach atan2 at the two samples where silence begins and ends: one of cur, prev is (+0, +0), the other (a, b), and
    d = (+-0, +-0) with the signs of a and b.  That gives +0, -0 and +pi; -pi needs d.r = -0 and d.i = -0, i.e.
    a * 0 = -0 and b * 0 = +0 for d.r but b * 0 = -0 (or a * 0 = +0) for d.i: no (a, b) does that.  So the committed
    channels have to show +0, -0 and +pi * fm_scaling / pi = fm_scaling, and they do."""
    seen = set()
    for cfg, seed in backend_channels():
        if cfg["discri"] != 2:
            continue
        o = backend_oracle(cfg)
        y = np.concatenate([o.feed(f) for f in fe.ragged(fe.be_input(seed), fe.BE_CUTS)])
        u = y.view(np.uint32)
        assert (u == 0).sum() > 4000                      # the silent stretch: 6000 * 48000 / 60000 outputs less the filter's length
        seen |= set(int(v) for v in u[np.isin(u, (0, 0x80000000, 0x41200000, 0xC1200000))])
    assert seen == {0, 0x80000000, 0x41200000}, [hex(v) for v in seen]


# ------------------------------------------------------------------------------------------------ oracle == compiled reference
@pytest.fixture(scope="module")
def ref():
    R = C.CDLL(REF)
    vp = C.c_void_p
    R.ref_fdecim_new.restype = vp; R.ref_fdecim_new.argtypes = [C.c_int] * 3
    R.ref_fdecim_free.argtypes = [vp]
    R.ref_fdecim_process.restype = C.c_int; R.ref_fdecim_process.argtypes = [vp, C.c_int, C.c_int, vp, C.c_int32, vp]
    R.ref_iqimb_new.restype = vp
    R.ref_iqimb_process.argtypes = [vp, vp, C.c_int64, vp]
    R.ref_iqimb_free.argtypes = [vp]
    R.ref_iir_new.restype = vp; R.ref_iir_new.argtypes = [C.c_int32, vp, vp]
    R.ref_iir_run.argtypes = [vp, vp, C.c_int64, vp]
    R.ref_fir_new.restype = vp; R.ref_fir_new.argtypes = [C.c_int, C.c_int, C.c_double, C.c_double, C.c_double]
    R.ref_fir_run.argtypes = [vp, vp, C.c_int64, vp]
    R.ref_nfmtail_new.restype = vp; R.ref_nfmtail_new.argtypes = [C.c_int32, C.c_float, C.c_float, C.c_int32, C.c_float, C.c_float]
    R.ref_nfmtail_process.argtypes = [vp, vp, C.c_int64, vp]
    R.ref_ssbtail_new.restype = vp; R.ref_ssbtail_new.argtypes = [C.c_int32, C.c_int32, C.c_double, C.c_int32, C.c_int32, C.c_int32, C.c_float]
    R.ref_ssbtail_process.argtypes = [vp, vp, C.c_int64, vp]
    return R


def ref_fdecim(R, kind, L, fc, x):
    ik, ok = orc.FDecim.KINDS[kind]
    h = R.ref_fdecim_new(ik, ok, 16)
    outs = []
    for blk in fe.fd_blocks(x):
        blk = np.ascontiguousarray(blk)
        o = np.zeros(blk.size + 8, np.int16 if ok == 0 else np.float32)
        k = R.ref_fdecim_process(h, L, fc, blk.ctypes.data, blk.size, o.ctypes.data)
        outs.append(o[: 2 * k].copy())
    R.ref_fdecim_free(h)
    return np.concatenate(outs)


@pytest.mark.ref
@needs_ref
@pytest.mark.parametrize("L,fc", fe.FD_CASES)
@pytest.mark.parametrize("kind", ("fi", "ff"))
def test_float_decimators_vs_reference_on_edge_inputs(ref, kind, L, fc):
    for name in fe.FD_KIND_INPUTS[kind]:
        x = fe.FD_INPUTS[name]()
        got, want = fd_oracle(kind, L, fc, x), ref_fdecim(ref, kind, L, fc, x)
        if kind == "fi":
            assert np.array_equal(got, want), (name, int((got != want).sum()))
        else:
            assert fe.same_bits(got, want), (name, fe.first_difference(got, want))


@pytest.mark.ref
@needs_ref
def test_golden_file_is_what_the_reference_produces(ref):
    g = np.load(GOLDEN)
    assert sorted(g.files) == sorted(f"fi_{n}_L{L}_fc{fc}" for n in fe.FD_KIND_INPUTS["fi"] for L, fc in fe.FD_GOLDEN_CASES)
    for name in fe.FD_KIND_INPUTS["fi"]:
        for L, fc in fe.FD_GOLDEN_CASES:
            assert np.array_equal(g[f"fi_{name}_L{L}_fc{fc}"], ref_fdecim(ref, "fi", L, fc, fe.FD_INPUTS[name]())), (name, L, fc)


def test_oracle_matches_the_golden_file():
    """runs everywhere: the reference's recorded word on the conversions against the oracle"""
    g = np.load(GOLDEN)
    for name in fe.FD_KIND_INPUTS["fi"]:
        for L, fc in fe.FD_GOLDEN_CASES:
            assert np.array_equal(g[f"fi_{name}_L{L}_fc{fc}"], fd_oracle("fi", L, fc, fe.FD_INPUTS[name]())), (name, L, fc)


@pytest.mark.ref
@needs_ref
def test_iq_imbalance_vs_reference_on_gap_streams(ref):
    for name, x in fe.iq_streams().items():
        h = ref.ref_iqimb_new(); o = orc.IqImb()
        for seg in fe.iq_feeds(x):
            seg = np.ascontiguousarray(seg); want = np.zeros(seg.size + 2, np.int16)
            ref.ref_iqimb_process(h, seg.ctypes.data, seg.size // 2, want.ctypes.data)
            assert np.array_equal(o.process(seg), want[: seg.size]), name
        ref.ref_iqimb_free(h)


@pytest.mark.ref
@needs_ref
def test_iir_vs_reference_through_subnormals_and_overflow(ref):
    for i, (o, a, b) in enumerate(IIR_SPECS + [fe.IIR_UNSTABLE]):
        a32 = np.ascontiguousarray(a, np.float32); b32 = np.ascontiguousarray(b, np.float32)
        h = ref.ref_iir_new(o, a32.ctypes.data, b32.ctypes.data); f = orc.Iir(o, a, b)
        x = fe.iir_input(70 + i if i < len(IIR_SPECS) else 99)
        for seg in (x[: fe.IIR_CUT], x[fe.IIR_CUT:]):
            seg = np.ascontiguousarray(seg); want = np.zeros(seg.size, np.float32)
            ref.ref_iir_run(h, seg.ctypes.data, seg.size, want.ctypes.data)
            assert fe.same_bits(f.run(seg), want), i


@pytest.mark.ref
@needs_ref
def test_audio_firs_vs_reference_on_edge_inputs(ref):
    for c, s in enumerate(fe.FIR_SPECS):
        for x in (fe.fir_subnormal(c), fe.fir_huge(), fe.fir_signed_zero()):
            h = ref.ref_fir_new(*s); o = orc.Fir(*s)
            for a, b in zip(fe.FIR_FEEDS[:-1], fe.FIR_FEEDS[1:]):
                seg = np.ascontiguousarray(x[a:b]); want = np.zeros(seg.size + 1, np.float32)
                ref.ref_fir_run(h, seg.ctypes.data, seg.size, want.ctypes.data)
                assert fe.same_bits(o.run(seg), want[: seg.size]), (c, a, b)


@pytest.mark.ref
@needs_ref
def test_audio_tails_vs_reference_across_a_gap(ref):
    for i, k in enumerate(NFM + SSB):
        x, gap = audiotail_input(i, k)
        o = orc.AudioTailOracle(**k)
        if k["kind"] == 0:
            h = ref.ref_nfmtail_new(k["audio_rate"], k["fm_scaling"], k["squelch_level"], k["squelch_gate"], k["volume"], k["af_bandwidth"]); run = ref.ref_nfmtail_process
        else:
            h = ref.ref_ssbtail_new(k["agc_active"], k["agc_nb_samples"], k["agc_threshold"], k["agc_threshold_enable"], k["agc_gate"], k["agc_clamping"], k["volume"]); run = ref.ref_ssbtail_process
        for seg in fe.ragged(x, (fe.AT_BURST + 1234,)):
            seg = np.ascontiguousarray(seg); want = np.zeros(seg.size // 2, np.int16)
            run(h, seg.ctypes.data, seg.size // 2, want.ctypes.data)
            assert np.array_equal(o.feed(seg), want), i
