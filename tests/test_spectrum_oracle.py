"""CPU checks of the spectrum sink: the C restatement of SpectrumVis (tests/spectrum_oracle.c) against an independent numpy
model of its buffer quirk, the configurations sdrx_spectrum_* rejects (validated before any device call), and frame counts."""
import ctypes as C

import numpy as np
import pytest

import sdrangel_amd as sa
from tests import spectrum_cases as sc


@pytest.fixture(scope="module")
def oracle():
    return sc.build_oracle()


def _np_frames(iq, n_fft, pct, window, scalef=32768.0):
    """numpy model of a fresh object fed once: frame k transforms zeros except the S fresh samples at [ov, N - ov)"""
    ov = n_fft * pct // 100
    s = n_fft - 2 * ov
    x = iq[0::2].astype(np.float32) / np.float32(scalef) + 1j * (iq[1::2].astype(np.float32) / np.float32(scalef))
    out = []
    for k in range(x.size // s):
        b = np.zeros(n_fft, complex)
        b[ov:ov + s] = x[k * s:(k + 1) * s]
        p = np.abs(np.fft.fft(b * window)) ** 2 / n_fft ** 2
        out.append(np.fft.fftshift(p))
    return np.array(out)


@pytest.mark.parametrize("n_fft,pct,win", [(64, 0, 5), (256, 10, 1), (1024, 25, 3), (2048, 25, 5), (4096, 49, 4), (128, 49, 0), (512, 0, 2)])
def test_oracle_matches_numpy_model(oracle, n_fft, pct, win):
    rng = np.random.default_rng(n_fft + pct)
    iq = sc.signal("noise", 6 * n_fft, rng)
    o = sc.OracleSpectrum(oracle, (n_fft, pct, 0, sc.NONE, win, 1))
    got = o.feed(iq, False)
    want = _np_frames(iq, n_fft, pct, o.window().astype(np.float64))
    assert got.shape == want.shape
    np.testing.assert_allclose(got, want, rtol=2e-3, atol=1e-9)


def test_oracle_frame_counts_follow_the_buffer_rule(oracle):
    for n_fft, pct in [(1024, 0), (1024, 25), (64, 49), (4096, 10)]:
        ov = n_fft * pct // 100
        s, fill, rng = n_fft - 2 * ov, ov, np.random.default_rng(1)
        o = sc.OracleSpectrum(oracle, (n_fft, pct, 0, sc.NONE, 1, 0))
        for n in [1, n_fft - 1, n_fft + 1, 3, 10 * n_fft + 7, s, s - 1]:
            got = o.feed(sc.signal("zero", n, rng), False).shape[0]
            need = (n_fft - ov) - fill
            want = 0 if n < need else 1 + (n - need) // s
            fill = fill + n if want == 0 else ov + (n - need - (want - 1) * s)
            assert got == want, (n_fft, pct, n)


def test_oracle_averaging_modes(oracle):
    rng = np.random.default_rng(5)
    iq = sc.signal("noise", 256 * 12, rng)
    plain = sc.OracleSpectrum(oracle, (256, 0, 0, sc.NONE, 1, 1)).feed(iq, False)
    mov = sc.OracleSpectrum(oracle, (256, 0, 3, sc.MOVING, 1, 1)).feed(iq, False)
    fix = sc.OracleSpectrum(oracle, (256, 0, 3, sc.FIXED, 1, 1)).feed(iq, False)
    assert plain.shape == (12, 256) and mov.shape == (12, 256) and fix.shape == (4, 256)
    # moving: sum over the last 3 frames (zeros before) / 3, in double
    p64 = plain.astype(np.float64) * 256 * 256
    acc = np.cumsum(np.vstack([np.zeros((2, 256)), p64]), axis=0)
    ref = ((acc[2:] - np.vstack([np.zeros((3, 256)), acc[:-3]])[2:]) / 3 / 65536).astype(np.float32)
    np.testing.assert_allclose(mov, ref, rtol=1e-5)
    # fixed + linear: the reference's quirk emits the block's LAST frame, not the average
    assert np.array_equal(fix, plain[2::3])


@pytest.mark.parametrize("cfg", [(1024, 50, 0, 0, 1, 0), (1024, 75, 0, 0, 1, 0), (64, 100, 0, 0, 1, 0), (1000, 0, 0, 0, 1, 0),
                                 (3000, 10, 0, 0, 1, 0), (1024, 0, 0, 0, 6, 0), (1024, 0, 0, 0, -1, 0), (1024, 0, 3, 3, 1, 0),
                                 (1024, 0, 3, -1, 1, 0)])
def test_rejected_configurations(oracle, cfg):
    with pytest.raises(ValueError):
        sc.OracleSpectrum(oracle, cfg)
    c = sa.SpectrumVis._cfg(*cfg, 32768.0)
    h = C.c_void_p()
    rc = sa.lib().sdrx_spectrum_create(C.byref(h), 0, C.byref(c))
    assert rc == -1 and not h.value                    # SDRX_EINVAL, before any device call
    assert sa.lib().sdrx_last_error()


def test_clamped_configurations_are_accepted(oracle):
    # handleConfigure clamps: N 8192 -> 4096, 32 -> 64, overlap -5 % -> 0 %
    for cfg in [(8192, 0, 0, 0, 1, 0), (32, -5, 0, 0, 1, 0), (100000, 49, 0, 0, 1, 0)]:
        o = sc.OracleSpectrum(oracle, cfg)
        assert o.window().size == min(max(cfg[0], 64), 4096)


def test_bad_scalef_rejected():
    for scalef in (0.0, float("inf"), float("nan")):
        c = sa.SpectrumVis._cfg(1024, 0, 0, 0, 1, 0, scalef)
        h = C.c_void_p()
        assert sa.lib().sdrx_spectrum_create(C.byref(h), 0, C.byref(c)) == -1
