"""CPU: sdrx_nfm_* rejects bad configurations with SDRX_EINVAL and a message before any device is touched, fails loudly
without a device (no CPU fallback), and its accessors refuse a null handle."""
import ctypes as C

import pytest

import sdrangel_amd as sa

GOOD = dict(in_rate=60000, nco_freq=-3000, audio_rate=48000, rf_bandwidth=12500.0, af_bandwidth=3000.0, fm_deviation=2000, volume=2.0,
            squelch=-300.0, squelch_gate=5, audio_mute=0)


def _create(n_ch=1, cfgs=None, **kw):
    d = dict(GOOD); d.update(kw)
    arr = (sa.NfmCfg * max(n_ch, 1))(*(cfgs or [sa.NfmCfg(**d)] * max(n_ch, 1)))
    h = C.c_void_p()
    # device 1 << 20 does not exist anywhere: a configuration that passes validation must then fail with SDRX_ENODEV
    rc = sa.lib().sdrx_nfm_create(C.byref(h), 1 << 20, n_ch, arr)
    assert not h.value
    return rc, sa.lib().sdrx_last_error().decode()


@pytest.mark.parametrize("kw", [dict(audio_rate=60001), dict(audio_rate=0), dict(audio_rate=999), dict(audio_rate=-48000), dict(in_rate=0),
                                dict(in_rate=-5), dict(in_rate=24000), dict(rf_bandwidth=0.0), dict(rf_bandwidth=-5000.0),
                                dict(rf_bandwidth=float("nan")), dict(rf_bandwidth=2.0e7), dict(af_bandwidth=300.0), dict(af_bandwidth=0.0),
                                dict(af_bandwidth=-3000.0), dict(af_bandwidth=float("nan")), dict(af_bandwidth=2.0e7),
                                dict(fm_deviation=0), dict(fm_deviation=-2000), dict(squelch_gate=-1), dict(squelch_gate=1001),
                                dict(volume=float("nan")), dict(volume=float("inf")), dict(squelch=float("inf")), dict(squelch=float("nan"))])
def test_bad_configurations_are_rejected_before_the_device(kw):
    rc, msg = _create(**kw)
    assert rc == -1 and "sdrx_nfm_create" in msg, (rc, msg)         # SDRX_EINVAL, not SDRX_ENODEV


def test_bad_arguments():
    assert _create(n_ch=0)[0] == -1
    assert sa.lib().sdrx_nfm_create(None, 0, 1, (sa.NfmCfg * 1)(sa.NfmCfg(**GOOD))) == -1
    h = C.c_void_p()
    assert sa.lib().sdrx_nfm_create(C.byref(h), 0, 1, None) == -1
    # a bad channel anywhere in the list
    cfgs = [sa.NfmCfg(**GOOD), sa.NfmCfg(**dict(GOOD, audio_rate=96000))]
    assert _create(n_ch=2, cfgs=cfgs)[0] == -1
    assert sa.lib().sdrx_nfm_destroy(None) == 0


def test_null_handle_accessors():
    L = sa.lib()
    ptrs, ns = (C.c_void_p * 1)(), (C.c_int64 * 1)(0)
    out, p, n = (C.c_int16 * 4)(), C.c_void_p(), C.c_int64()
    d, d2, d3, g, nt, lvl = C.c_double(), C.c_double(), C.c_double(), C.c_int32(), C.c_int32(), C.c_float()
    name, a, b, c = C.create_string_buffer(64), C.c_int(), C.c_int(), C.c_int()
    calls = [(L.sdrx_nfm_reset, (None,)), (L.sdrx_nfm_sync, (None,)), (L.sdrx_nfm_feed, (None, ptrs, ns)), (L.sdrx_nfm_feed_dev, (None, ptrs, ns)),
             (L.sdrx_nfm_feed_bank, (None, None)), (L.sdrx_nfm_read, (None, 0, out, 4)), (L.sdrx_nfm_last_dev, (None, 0, C.byref(p), C.byref(n))),
             (L.sdrx_nfm_squelch_open, (None, 0)), (L.sdrx_nfm_levels, (None, 0, C.byref(d), C.byref(d2), C.byref(d3), C.byref(n), 0)),
             (L.sdrx_nfm_get_design, (None, 0, C.byref(nt), None, 0, None, C.byref(g), C.byref(lvl), C.byref(g))),
             (L.sdrx_nfm_set_stream, (None, None)), (L.sdrx_nfm_get_stream, (None, C.byref(p))), (L.sdrx_nfm_set_timing, (None, 1)),
             (L.sdrx_nfm_get_timing, (None, C.byref(d), C.byref(n), 0)),
             (L.sdrx_nfm_last_launch, (None, name, 64, C.byref(a), C.byref(b), C.byref(c)))]
    for fn, args in calls:
        assert fn(*args) == -1, fn.__name__


@pytest.mark.parametrize("kw", [dict(), dict(audio_rate=1000, in_rate=1000), dict(audio_rate=60000), dict(squelch_gate=0, audio_mute=1),
                                dict(squelch_gate=1000, fm_deviation=1), dict(af_bandwidth=300.5)])
def test_a_good_configuration_reaches_the_device_check(kw):
    rc, msg = _create(**kw)
    assert rc == -2, (rc, msg)                                      # SDRX_ENODEV: validation passed, the device index did not


def test_no_cpu_fallback():
    if sa.lib().sdrx_device_count() > 0:
        pytest.skip("a HIP device is present")
    with pytest.raises(sa.SdrxError) as e:
        sa.NfmDemodBank([sa.NfmCfg(**GOOD)])
    assert "rc=-2" in str(e.value)


def test_cfg_struct_matches_the_header():
    assert C.sizeof(sa.NfmCfg) == 40 and sa.NfmCfg.audio_mute.offset == 36 and sa.NfmCfg.fm_deviation.offset == 20
    assert sa.NfmCfg.squelch.offset == 28
    for name in ("create", "destroy", "reset", "feed", "feed_dev", "feed_bank", "read", "last_dev", "squelch_open", "levels", "get_design",
                 "sync", "set_stream", "get_stream", "set_timing", "get_timing", "last_launch"):
        assert f"sdrx_nfm_{name}" in sa.exported_symbols(), name
