"""CPU, build container only: the oracle against the compiled reference (oracle/_ref/libsdrref.so) at the limits of what
sdrx_backend_create, sdrx_audiotail_create and sdrx_firbank_create accept -- the configurations of tests/float_limit_cases.py,
which tests/test_float_limits_gpu.py then runs on the GPU against the oracle.  Skipped where the reference build did not happen."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import float_limit_cases as flc
from tests import oracle_py as orc
from tests import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "oracle", "_ref", "libsdrref.so")
pytestmark = [pytest.mark.ref, pytest.mark.skipif(not os.path.exists(REF), reason="oracle/_ref not built (no /root/reference here)")]


@pytest.fixture(scope="module")
def ref():
    L = C.CDLL(REF)
    vp, i32, i64, f32, f64 = C.c_void_p, C.c_int32, C.c_int64, C.c_float, C.c_double
    L.ref_backend_new.restype = vp; L.ref_backend_new.argtypes = [f32, f32, f32, C.c_int, f32, f32]
    L.ref_backend_free.argtypes = [vp]
    L.ref_backend_feed.restype = i64; L.ref_backend_feed.argtypes = [vp, vp, i64, vp]
    L.ref_nfmtail_new.restype = vp; L.ref_nfmtail_new.argtypes = [i32, f32, f32, i32, f32, f32]
    L.ref_nfmtail_process.argtypes = [vp, vp, i64, vp]
    L.ref_ssbtail_new.restype = vp; L.ref_ssbtail_new.argtypes = [i32, i32, f64, i32, i32, i32, f32]
    L.ref_ssbtail_process.argtypes = [vp, vp, i64, vp]
    L.ref_fir_new.restype = vp; L.ref_fir_new.argtypes = [C.c_int, C.c_int, f64, f64, f64]
    L.ref_fir_run.argtypes = [vp, vp, i64, vp]
    return L


@pytest.mark.parametrize("i", range(len(flc.BACKEND)))
def test_backend_corner_vs_reference(ref, i):
    """NCO + Interpolator at 2..256 taps per phase, NCO increments beyond the table, ratios from 1.00002 to 2930:
    one feed of noise, oracle == reference bit for bit; the tap count and the NCO increment are the ones the case is named for"""
    k = flc.BACKEND[i]
    nf, ir, orr, cut, tpp = float(k["nco_freq"]), float(k["in_rate"]), float(k["out_rate"]), k["interp_cutoff"], k["taps_per_phase"]
    n = flc.be_ref_len(k)
    x = synth.noise_iq(n, 55 + i, 30000)
    hr = ref.ref_backend_new(nf, ir, orr, 16, cut, tpp); o = orc.Backend(ir, nf, orr, cut, tpp)
    assert o.taps()[0] == k["ntaps"]
    if k["nco_inc"] is not None:
        assert orc.lib().sdro_nco_inc(nf, ir) == k["nco_inc"]
    A = np.zeros(2 * n + 8, np.float32)
    m = ref.ref_backend_feed(hr, x.ctypes.data, n, A.ctypes.data)
    got = o.feed(x)
    ref.ref_backend_free(hr)
    assert m > 10 and got.size == 2 * m and np.array_equal(A[: 2 * m].view(np.uint32), got.view(np.uint32))


@pytest.mark.parametrize("i", range(len(flc.NFM_TAILS) + len(flc.SSB_TAILS)))
def test_audio_tail_corner_vs_reference(ref, i):
    """squelch gates 1, NFM_DL and NFM_DL + 1, audio rates other than 48000 (the `comp` factor, the band pass at that rate), AGC
    lengths 2 and 3 (step length 1) and at / past the SSB delay line (the delay clamp): qint16 audio identical over ragged
    calls, and not all zero -- the squelch opened, the AGC stepped up"""
    k = flc.tail_cfgs()[i]
    if k["kind"] == 0:
        h = ref.ref_nfmtail_new(k["audio_rate"], k["fm_scaling"], k["squelch_level"], k["squelch_gate"], k["volume"], k["af_bandwidth"]); run = ref.ref_nfmtail_process
    else:
        h = ref.ref_ssbtail_new(k["agc_active"], k["agc_nb_samples"], k["agc_threshold"], k["agc_threshold_enable"], k["agc_gate"], k["agc_clamping"], k["volume"]); run = ref.ref_ssbtail_process
    x = flc.tail_input(i)
    nonzero = 0
    for (a, b), have in zip(flc.TAIL_CALLS, flc.tail_expected(i)):
        seg = np.ascontiguousarray(x[2 * a: 2 * b]); want = np.zeros(b - a, np.int16)
        run(h, seg.ctypes.data, b - a, want.ctypes.data)
        assert np.array_equal(have, want), (i, a, b, int((have != want).sum()))
        nonzero += int((want != 0).sum())
    print("tail", i, "non-zero samples", nonzero)
    assert nonzero > 0


@pytest.mark.parametrize("kind,nt,rate,f1,f2", flc.FIR_SPECS)
def test_audio_fir_corner_vs_reference(ref, kind, nt, rate, f1, f2):
    """Lowpass / Bandpass at the shortest and longest tap counts (an even count is made odd): calls shorter than, equal to and
    longer than the ring"""
    hr = ref.ref_fir_new(kind, nt, rate, f1, f2); o = orc.Fir(kind, nt, rate, f1, f2)
    assert o.taps().size == (nt | 1) // 2 + 1
    rng = np.random.default_rng(nt)
    for n in flc.fir_calls(nt):
        x = rng.standard_normal(n).astype(np.float32); A = np.zeros(n + 1, np.float32)
        ref.ref_fir_run(hr, x.ctypes.data, n, A.ctypes.data)
        assert np.array_equal(A[:n].view(np.uint32), o.run(x).view(np.uint32)), (kind, nt, n)


def test_case_tables_reach_what_they_are_for():
    """properties of the tables that the GPU tests rely on, from arithmetic alone"""
    steps = [flc.be_step(k) for k in flc.BACKEND]
    assert min(steps) < 1.00003 and max(steps) > 2929
    assert sorted(k["ntaps"] for k in flc.BE_TAPS) == [2, 6, 70, 80, 96, 256]
    for k in flc.BACKEND:
        if k["q10"]:
            assert flc.be_step(k) == 1 + 1 / 1024
            L = np.cumsum(flc.be_feed_lengths(k, 1))
            assert {700, 1024, 1025} <= set(int(v) for v in L)
    k = flc.BACKEND[flc.WINDOW_CASE]
    assert flc.fir_windows(k, [4000])[:5] == [383, 384, 385, 384, 385]
