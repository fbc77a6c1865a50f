"""CPU: sdrx_wfm_* rejects bad configurations with SDRX_EINVAL and a message before any device is touched, and fails loudly
without a device (no CPU fallback)."""
import ctypes as C

import pytest

import sdrangel_amd as sa

GOOD = dict(in_rate=240000, nco_freq=0, audio_rate=48000, rf_bandwidth=80000.0, af_bandwidth=15000.0, volume=2.0, squelch_db=-60.0,
            audio_mute=0)


def _create(n_ch=1, cfgs=None, **kw):
    d = dict(GOOD); d.update(kw)
    arr = (sa.WfmCfg * max(n_ch, 1))(*(cfgs or [sa.WfmCfg(**d)] * max(n_ch, 1)))
    h = C.c_void_p()
    # device 1 << 20 does not exist anywhere: a configuration that passes validation must then fail with SDRX_ENODEV
    rc = sa.lib().sdrx_wfm_create(C.byref(h), 1 << 20, n_ch, arr)
    assert not h.value
    return rc, sa.lib().sdrx_last_error().decode()


@pytest.mark.parametrize("kw", [dict(audio_rate=240001), dict(audio_rate=0), dict(in_rate=0), dict(in_rate=-5), dict(rf_bandwidth=0.0),
                                dict(rf_bandwidth=-80000.0), dict(rf_bandwidth=float("nan")), dict(rf_bandwidth=2.0e7), dict(af_bandwidth=0.0),
                                dict(af_bandwidth=float("inf")), dict(volume=float("nan")), dict(squelch_db=float("inf"))])
def test_bad_configurations_are_rejected_before_the_device(kw):
    rc, msg = _create(**kw)
    assert rc == -1 and "sdrx_wfm_create" in msg, (rc, msg)         # SDRX_EINVAL, not SDRX_ENODEV


def test_bad_arguments():
    assert _create(n_ch=0)[0] == -1
    assert sa.lib().sdrx_wfm_create(None, 0, 1, (sa.WfmCfg * 1)(sa.WfmCfg(**GOOD))) == -1
    h = C.c_void_p()
    assert sa.lib().sdrx_wfm_create(C.byref(h), 0, 1, None) == -1
    # a bad channel anywhere in the list
    cfgs = [sa.WfmCfg(**GOOD), sa.WfmCfg(**dict(GOOD, audio_rate=300000))]
    assert _create(n_ch=2, cfgs=cfgs)[0] == -1
    for fn in ("sdrx_wfm_reset", "sdrx_wfm_sync"):
        assert getattr(sa.lib(), fn)(None) == -1
    assert sa.lib().sdrx_wfm_destroy(None) == 0


def test_a_good_configuration_reaches_the_device_check():
    rc, msg = _create()
    assert rc == -2, (rc, msg)                                      # SDRX_ENODEV: validation passed, the device index did not


def test_no_cpu_fallback():
    if sa.lib().sdrx_device_count() > 0:
        pytest.skip("a HIP device is present")
    with pytest.raises(sa.SdrxError) as e:
        sa.WfmDemodBank([sa.WfmCfg(**GOOD)])
    assert "rc=-2" in str(e.value)


def test_required_bw():
    assert sa.wfm_required_bw(80000) == 120000 and sa.wfm_required_bw(250000) == 375000 and sa.wfm_required_bw(12500) == 48000
