"""CPU: sdrx_nfm_create_ex rejects bad tone configurations with SDRX_EINVAL and a message before any device is touched, fails
loudly without a device, takes a null tone list like sdrx_nfm_create, and the CTCSS accessors refuse a null handle."""
import ctypes as C

import pytest

import sdrangel_amd as sa

GOOD = dict(in_rate=60000, nco_freq=-3000, audio_rate=48000, rf_bandwidth=12500.0, af_bandwidth=3000.0, fm_deviation=2000, volume=2.0,
            squelch=-300.0, squelch_gate=5, audio_mute=0)


def _create(tone_kw, n_ch=1, null_tone=False, **kw):
    d = dict(GOOD); d.update(kw)
    arr = (sa.NfmCfg * n_ch)(*[sa.NfmCfg(**d)] * n_ch)
    tones = tone_kw if isinstance(tone_kw, list) else [tone_kw] * n_ch
    tarr = None if null_tone else (sa.NfmToneCfg * n_ch)(*[sa.NfmToneCfg(**t) for t in tones])
    h = C.c_void_p()
    # device 1 << 20 does not exist anywhere: a configuration that passes validation must then fail with SDRX_ENODEV
    rc = sa.lib().sdrx_nfm_create_ex(C.byref(h), 1 << 20, n_ch, arr, tarr)
    assert not h.value
    return rc, sa.lib().sdrx_last_error().decode()


@pytest.mark.parametrize("tone", [dict(ctcss_on=2), dict(ctcss_on=-1), dict(ctcss_on=1, ctcss_index=33), dict(ctcss_index=-1), dict(ctcss_index=33),
                                  dict(reserved=1), dict(ctcss_on=1, reserved=-1), dict(delta_squelch=2), dict(delta_squelch=-1)])
def test_bad_tone_configurations_are_rejected_before_the_device(tone):
    rc, msg = _create(tone)
    assert rc == -1 and "sdrx_nfm_create_ex" in msg, (rc, msg)      # SDRX_EINVAL, not SDRX_ENODEV


@pytest.mark.parametrize("kw", [dict(squelch=float("inf")), dict(squelch=float("nan")), dict(audio_rate=96000), dict(squelch_gate=-1)])
def test_bad_base_configurations_are_still_rejected(kw):
    rc, msg = _create(dict(ctcss_on=1, ctcss_index=12), **kw)
    assert rc == -1 and "sdrx_nfm_create" in msg, (rc, msg)


def test_a_bad_channel_anywhere_in_the_list():
    assert _create([dict(ctcss_on=1), dict(ctcss_on=1, ctcss_index=40)], n_ch=2)[0] == -1


@pytest.mark.parametrize("tone", [dict(), dict(ctcss_on=1), dict(ctcss_on=1, ctcss_index=32), dict(ctcss_on=0, ctcss_index=5), dict(ctcss_on=1, ctcss_index=1),
                                  dict(delta_squelch=1), dict(delta_squelch=1, ctcss_on=1, ctcss_index=12), dict(delta_squelch=1, ctcss_index=3)])
def test_a_good_configuration_reaches_the_device_check(tone):
    rc, msg = _create(tone)
    assert rc == -2, (rc, msg)                                      # SDRX_ENODEV: validation passed, the device index did not
    assert _create([tone, dict(), dict(ctcss_on=1, ctcss_index=12), dict(delta_squelch=1)], n_ch=4)[0] == -2


def test_null_tone_list_is_accepted_like_create():
    assert _create(None, null_tone=True)[0] == -2
    assert _create(None, null_tone=True, audio_rate=96000)[0] == -1


def test_bad_arguments():
    L = sa.lib()
    cfg, tone = (sa.NfmCfg * 1)(sa.NfmCfg(**GOOD)), (sa.NfmToneCfg * 1)(sa.NfmToneCfg(ctcss_on=1))
    h = C.c_void_p()
    assert L.sdrx_nfm_create_ex(None, 0, 1, cfg, tone) == -1
    assert L.sdrx_nfm_create_ex(C.byref(h), 0, 0, cfg, tone) == -1
    assert L.sdrx_nfm_create_ex(C.byref(h), 0, 1, None, tone) == -1 and not h.value


def test_null_handle_accessors():
    L = sa.lib()
    i, f, n, d = C.c_int32(), C.c_float(), C.c_int64(), C.c_int32()
    at, idx, p, coef, lp = (C.c_int64 * 4)(), (C.c_int32 * 4)(), (C.c_float * 32)(), (C.c_float * 32)(), (C.c_float * 151)()
    calls = [(L.sdrx_nfm_ctcss, (None, 0, C.byref(i), C.byref(f), C.byref(n))), (L.sdrx_nfm_ctcss_events, (None, 0, at, idx, 4)),
             (L.sdrx_nfm_ctcss_powers, (None, 0, p, C.byref(d), C.byref(i), C.byref(n))),
             (L.sdrx_nfm_af_squelch, (None, 0, C.byref(d), (C.c_double * 2)(), C.byref(i))),
             (L.sdrx_nfm_get_tone_design, (None, 0, C.byref(i), C.byref(d), coef, lp, C.byref(d), (C.c_double * 2)(), (C.c_double * 2)(), C.byref(C.c_double())))]
    for fn, args in calls:
        assert fn(*args) == -1, fn.__name__


def test_no_cpu_fallback():
    if sa.lib().sdrx_device_count() > 0:
        pytest.skip("a HIP device is present")
    with pytest.raises(sa.SdrxError) as e:
        sa.NfmDemodBank([sa.NfmCfg(**GOOD)], tone=[sa.NfmToneCfg(ctcss_on=1, ctcss_index=12)])
    assert "rc=-2" in str(e.value)
    with pytest.raises(ValueError):
        sa.NfmDemodBank([sa.NfmCfg(**GOOD)] * 2, tone=[sa.NfmToneCfg()])


def test_structs_match_the_header():
    assert C.sizeof(sa.NfmToneCfg) == 16 and C.sizeof(sa.NfmCfg) == 40
    assert [getattr(sa.NfmToneCfg, n).offset for n in ("delta_squelch", "ctcss_on", "ctcss_index", "reserved")] == [0, 4, 8, 12]
    for name in ("create_ex", "ctcss", "ctcss_events", "ctcss_powers", "af_squelch", "get_tone_design"):
        assert f"sdrx_nfm_{name}" in sa.exported_symbols(), name
    assert len(sa.CTCSS_TONES) == 32 and sa.CTCSS_TONES[11] == 100.0 and sa.CTCSS_TONES[31] == 203.5
