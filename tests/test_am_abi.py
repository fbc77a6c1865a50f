"""CPU: sdrx_am_* rejects bad configurations with SDRX_EINVAL and a message before any device is touched, and fails loudly
without a device (no CPU fallback)."""
import ctypes as C

import pytest

import sdrangel_amd as sa

GOOD = dict(in_rate=60000, nco_freq=-3000, audio_rate=48000, rf_bandwidth=5000.0, volume=2.0, squelch_db=-40.0, audio_mute=0, bandpass_enable=0)


def _create(n_ch=1, cfgs=None, **kw):
    d = dict(GOOD); d.update(kw)
    arr = (sa.AmCfg * max(n_ch, 1))(*(cfgs or [sa.AmCfg(**d)] * max(n_ch, 1)))
    h = C.c_void_p()
    # device 1 << 20 does not exist anywhere: a configuration that passes validation must then fail with SDRX_ENODEV
    rc = sa.lib().sdrx_am_create(C.byref(h), 1 << 20, n_ch, arr)
    assert not h.value
    return rc, sa.lib().sdrx_last_error().decode()


@pytest.mark.parametrize("kw", [dict(audio_rate=60001), dict(audio_rate=0), dict(audio_rate=999), dict(audio_rate=-48000), dict(in_rate=0),
                                dict(in_rate=-5), dict(in_rate=24000), dict(rf_bandwidth=0.0), dict(rf_bandwidth=-5000.0),
                                dict(rf_bandwidth=float("nan")), dict(rf_bandwidth=2.0e7), dict(volume=float("nan")),
                                dict(volume=float("inf")), dict(squelch_db=float("inf")), dict(squelch_db=float("nan"))])
def test_bad_configurations_are_rejected_before_the_device(kw):
    rc, msg = _create(**kw)
    assert rc == -1 and "sdrx_am_create" in msg, (rc, msg)          # SDRX_EINVAL, not SDRX_ENODEV


def test_bad_arguments():
    assert _create(n_ch=0)[0] == -1
    assert sa.lib().sdrx_am_create(None, 0, 1, (sa.AmCfg * 1)(sa.AmCfg(**GOOD))) == -1
    h = C.c_void_p()
    assert sa.lib().sdrx_am_create(C.byref(h), 0, 1, None) == -1
    # a bad channel anywhere in the list
    cfgs = [sa.AmCfg(**GOOD), sa.AmCfg(**dict(GOOD, audio_rate=96000))]
    assert _create(n_ch=2, cfgs=cfgs)[0] == -1
    for fn in ("sdrx_am_reset", "sdrx_am_sync"):
        assert getattr(sa.lib(), fn)(None) == -1
    assert sa.lib().sdrx_am_destroy(None) == 0


@pytest.mark.parametrize("kw", [dict(), dict(audio_rate=1000, in_rate=1000), dict(audio_rate=60000), dict(bandpass_enable=1, audio_mute=1)])
def test_a_good_configuration_reaches_the_device_check(kw):
    rc, msg = _create(**kw)
    assert rc == -2, (rc, msg)                                      # SDRX_ENODEV: validation passed, the device index did not


def test_no_cpu_fallback():
    if sa.lib().sdrx_device_count() > 0:
        pytest.skip("a HIP device is present")
    with pytest.raises(sa.SdrxError) as e:
        sa.AmDemodBank([sa.AmCfg(**GOOD)])
    assert "rc=-2" in str(e.value)


def test_cfg_struct_matches_the_header():
    assert C.sizeof(sa.AmCfg) == 32 and sa.AmCfg.bandpass_enable.offset == 28 and sa.AmCfg.rf_bandwidth.offset == 12
