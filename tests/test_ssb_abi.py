"""CPU: sdrx_ssb_* exists, rejects bad configurations with SDRX_EINVAL and a message before any device is touched, fails loudly
without a device (no CPU fallback), and its accessors refuse a null handle."""
import ctypes as C

import pytest

import sdrangel_amd as sa

GOOD = dict(in_rate=60000, nco_freq=-3000, audio_rate=48000, rf_bandwidth=3000.0, low_cutoff=300.0, volume=3.0, span_log2=3, audio_binaural=0,
            audio_flip=0, dsb=0, audio_mute=0, agc=1, agc_clamping=0, agc_time_log2=7, agc_power_threshold=-40, agc_threshold_gate=4)
ENTRIES = ("create", "destroy", "reset", "feed", "feed_dev", "feed_bank", "read", "last_dev", "read_spectrum", "spectrum_last_dev", "audio_active",
           "levels", "get_design", "sync", "set_stream", "get_stream", "set_timing", "get_timing", "last_launch")


def _create(n_ch=1, cfgs=None, **kw):
    d = dict(GOOD); d.update(kw)
    arr = (sa.SsbCfg * max(n_ch, 1))(*(cfgs or [sa.SsbCfg(**d)] * max(n_ch, 1)))
    h = C.c_void_p()
    # device 1 << 20 does not exist anywhere: a configuration that passes validation must then fail with SDRX_ENODEV
    rc = sa.lib().sdrx_ssb_create(C.byref(h), 1 << 20, n_ch, arr)
    assert not h.value
    return rc, sa.lib().sdrx_last_error().decode()


def test_symbols_exist_and_are_declared():
    declared = set(sa.exported_symbols())
    for name in ENTRIES:
        assert f"sdrx_ssb_{name}" in declared, name
        assert getattr(sa.lib(), f"sdrx_ssb_{name}")
    assert [f[0] for f in sa.SsbCfg._fields_] == list(GOOD)
    assert C.sizeof(sa.SsbCfg) == 16 * 4


@pytest.mark.parametrize("kw", [
    dict(audio_rate=60001), dict(audio_rate=0), dict(audio_rate=999), dict(audio_rate=-48000), dict(in_rate=0), dict(in_rate=-5), dict(in_rate=24000),
    dict(in_rate=400000, audio_rate=192001),                                     # keeps hn == 12000 out of reach
    dict(in_rate=375000, audio_rate=375000, agc_time_log2=5),                    # ... which this one would be
    dict(audio_rate=1000, agc_time_log2=0),                                      # hn = 1 < 2
    dict(agc_time_log2=12),                                                      # hn = 196608 > 131072
    dict(agc_time_log2=-1), dict(agc_time_log2=31), dict(agc_time_log2=40),
    dict(span_log2=0), dict(span_log2=9), dict(span_log2=-1),
    dict(rf_bandwidth=float("nan")), dict(rf_bandwidth=2.0e7), dict(rf_bandwidth=float("inf")), dict(low_cutoff=float("nan")), dict(low_cutoff=-2.0e7),
    dict(volume=float("nan")), dict(volume=float("inf")), dict(agc_threshold_gate=-1), dict(agc_threshold_gate=10001),
    dict(agc_power_threshold=301), dict(agc_power_threshold=-301)])
def test_bad_configurations_are_rejected_before_the_device(kw):
    rc, msg = _create(**kw)
    assert rc == -1 and "sdrx_ssb_create" in msg, (rc, msg)         # SDRX_EINVAL, not SDRX_ENODEV


@pytest.mark.parametrize("kw", [dict(), dict(rf_bandwidth=-3000.0, low_cutoff=-300.0), dict(rf_bandwidth=50.0), dict(dsb=1), dict(agc_power_threshold=100),
                                dict(in_rate=192000, audio_rate=192000, agc_time_log2=9), dict(audio_rate=8000, in_rate=8000, agc_time_log2=1),
                                dict(audio_rate=2000, in_rate=48000, agc_time_log2=0), dict(agc_time_log2=11), dict(span_log2=1), dict(span_log2=8)])
def test_good_configurations_pass_validation_and_fail_on_the_device(kw):
    rc, msg = _create(**kw)
    assert rc not in (0, -1), (rc, msg)                              # no device of that number: not EINVAL, and no CPU fallback


def test_bad_arguments():
    assert _create(n_ch=0)[0] == -1
    assert sa.lib().sdrx_ssb_create(None, 0, 1, (sa.SsbCfg * 1)(sa.SsbCfg(**GOOD))) == -1
    h = C.c_void_p()
    assert sa.lib().sdrx_ssb_create(C.byref(h), 0, 1, None) == -1
    # a bad channel anywhere in the list
    cfgs = [sa.SsbCfg(**GOOD), sa.SsbCfg(**dict(GOOD, audio_rate=96000))]
    assert _create(n_ch=2, cfgs=cfgs)[0] == -1
    assert sa.lib().sdrx_ssb_destroy(None) == 0


def test_null_handle_accessors():
    L = sa.lib()
    ptrs, ns = (C.c_void_p * 1)(), (C.c_int64 * 1)(0)
    out, p, n = (C.c_int16 * 8)(), C.c_void_p(), C.c_int64()
    d, d2, d3, g, g2, nt, vol = C.c_double(), C.c_double(), C.c_double(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_float()
    name, a, b, c = C.create_string_buffer(64), C.c_int(), C.c_int(), C.c_int()
    calls = [(L.sdrx_ssb_reset, (None,)), (L.sdrx_ssb_sync, (None,)), (L.sdrx_ssb_feed, (None, ptrs, ns)), (L.sdrx_ssb_feed_dev, (None, ptrs, ns)),
             (L.sdrx_ssb_feed_bank, (None, None)), (L.sdrx_ssb_read, (None, 0, out, 4)), (L.sdrx_ssb_last_dev, (None, 0, C.byref(p), C.byref(n))),
             (L.sdrx_ssb_read_spectrum, (None, 0, out, 4)), (L.sdrx_ssb_spectrum_last_dev, (None, 0, C.byref(p), C.byref(n))),
             (L.sdrx_ssb_audio_active, (None, 0)), (L.sdrx_ssb_levels, (None, 0, C.byref(d), C.byref(d2), C.byref(d3), C.byref(n), 0)),
             (L.sdrx_ssb_get_design, (None, 0, C.byref(nt), None, 0, None, C.byref(g), C.byref(g), C.byref(g2), C.byref(d), C.byref(vol))),
             (L.sdrx_ssb_set_stream, (None, None)), (L.sdrx_ssb_get_stream, (None, C.byref(p))), (L.sdrx_ssb_set_timing, (None, 1)),
             (L.sdrx_ssb_get_timing, (None, C.byref(d), C.byref(n), 0)),
             (L.sdrx_ssb_last_launch, (None, name, 64, C.byref(a), C.byref(b), C.byref(c)))]
    for fn, args in calls:
        assert fn(*args) == -1, fn.__name__
