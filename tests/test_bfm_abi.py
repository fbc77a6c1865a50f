"""CPU: the sdrx_bfm_* entry points exist and are declared, their set is exactly the documented one, bad configurations are
rejected with SDRX_EINVAL and a message that names the field before any device is touched, and a good one fails loudly without a
device (no CPU fallback)."""
import ctypes as C
import os
import subprocess

import pytest

import sdrangel_amd as sa

GOOD = dict(in_rate=240000, nco_freq=0, audio_rate=48000, rf_bandwidth=80000.0, af_bandwidth=15000.0, volume=2.0, squelch_db=-60.0,
            audio_stereo=1, lsb_stereo=0, show_pilot=0)

CALLS = {"create", "destroy", "reset", "feed", "feed_dev", "feed_bank", "read", "last_dev", "read_sink", "sink_last_dev", "pilot",
         "squelch_open", "levels", "get_design", "sync", "set_stream", "get_stream", "set_timing", "get_timing", "last_launch"}


def _create(n_ch=1, cfgs=None, **kw):
    d = dict(GOOD); d.update(kw)
    arr = (sa.BfmCfg * max(n_ch, 1))(*(cfgs or [sa.BfmCfg(**d)] * max(n_ch, 1)))
    h = C.c_void_p()
    # device 1 << 20 does not exist anywhere: a configuration that passes validation must then fail with something else
    rc = sa.lib().sdrx_bfm_create(C.byref(h), 1 << 20, n_ch, arr)
    assert not h.value
    return rc, sa.lib().sdrx_last_error().decode()


def test_symbols_are_exactly_the_documented_set():
    declared = {s for s in sa.exported_symbols() if s.startswith("sdrx_bfm_")}
    assert declared == {"sdrx_bfm_" + c for c in CALLS}
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(os.path.dirname(sa.__file__), "libsdrx.so")], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l and l.split()[-1].startswith("sdrx_bfm_")}
    assert exported == declared
    for s in declared:
        assert getattr(sa.lib(), s).argtypes is not None, s          # bound with a prototype by sa.lib()


def test_cfg_layout():
    assert C.sizeof(sa.BfmCfg) == 40
    assert [f[0] for f in sa.BfmCfg._fields_] == ["in_rate", "nco_freq", "audio_rate", "rf_bandwidth", "af_bandwidth", "volume", "squelch_db",
                                                   "audio_stereo", "lsb_stereo", "show_pilot"]


@pytest.mark.parametrize("field,value", [("audio_rate", 240001), ("audio_rate", 0), ("audio_rate", -48000), ("in_rate", 0), ("in_rate", -5),
                                         ("rf_bandwidth", 0.0), ("rf_bandwidth", -80000.0), ("rf_bandwidth", float("nan")), ("rf_bandwidth", 2.0e7),
                                         ("rf_bandwidth", float("inf")), ("af_bandwidth", 0.0), ("af_bandwidth", float("inf")),
                                         ("af_bandwidth", float("nan")), ("volume", float("nan")), ("volume", float("inf")),
                                         ("squelch_db", float("inf")), ("squelch_db", float("nan")), ("audio_stereo", 2), ("audio_stereo", -1),
                                         ("lsb_stereo", 2), ("show_pilot", 7)])
def test_bad_fields_are_rejected_before_the_device(field, value):
    rc, msg = _create(**{field: value})
    assert rc == -1 and "sdrx_bfm_create" in msg and field in msg, (rc, msg)         # SDRX_EINVAL, and the field by name


@pytest.mark.parametrize("kw", [dict(), dict(audio_stereo=0), dict(lsb_stereo=1), dict(show_pilot=1, audio_stereo=0), dict(in_rate=384000),
                                dict(in_rate=250000, nco_freq=-31000), dict(in_rate=48000, audio_rate=48000), dict(volume=0.0)])
def test_good_configurations_reach_the_device_check(kw):
    rc, msg = _create(**kw)
    assert rc not in (0, -1), (rc, msg)                              # validation passed, the device index did not


def test_bad_arguments():
    assert _create(n_ch=0)[0] == -1
    assert sa.lib().sdrx_bfm_create(None, 0, 1, (sa.BfmCfg * 1)(sa.BfmCfg(**GOOD))) == -1
    h = C.c_void_p()
    assert sa.lib().sdrx_bfm_create(C.byref(h), 0, 1, None) == -1
    cfgs = [sa.BfmCfg(**GOOD), sa.BfmCfg(**dict(GOOD, lsb_stereo=3))]              # a bad channel anywhere in the list
    rc, msg = _create(n_ch=2, cfgs=cfgs)
    assert rc == -1 and "lsb_stereo" in msg
    L = sa.lib()
    for fn in ("reset", "sync"):
        assert getattr(L, "sdrx_bfm_" + fn)(None) == -1
    assert L.sdrx_bfm_feed(None, None, None) == -1 and L.sdrx_bfm_feed_dev(None, None, None) == -1 and L.sdrx_bfm_feed_bank(None, None) == -1
    assert L.sdrx_bfm_read(None, 0, None, 0) == -1 and L.sdrx_bfm_read_sink(None, 0, None, 0) == -1
    assert L.sdrx_bfm_last_dev(None, 0, None, None) == -1 and L.sdrx_bfm_sink_last_dev(None, 0, None, None) == -1
    assert L.sdrx_bfm_pilot(None, 0, None, None, None, None) == -1 and L.sdrx_bfm_squelch_open(None, 0) == -1
    assert L.sdrx_bfm_levels(None, 0, None, None, None, 0) == -1
    assert L.sdrx_bfm_get_design(None, 0, None, None, 0, None, None, None, None, None, None) == -1
    assert L.sdrx_bfm_set_stream(None, None) == -1 and L.sdrx_bfm_get_stream(None, None) == -1
    assert L.sdrx_bfm_set_timing(None, 0) == -1 and L.sdrx_bfm_get_timing(None, None, None, 0) == -1
    assert L.sdrx_bfm_last_launch(None, None, 0, None, None, None) == -1
    assert L.sdrx_bfm_destroy(None) == 0


def test_no_cpu_fallback():
    if sa.lib().sdrx_device_count() > 0:
        pytest.skip("a HIP device is present")
    with pytest.raises(sa.SdrxError) as e:
        sa.BfmBank([sa.BfmCfg(**GOOD)])
    assert "rc=-2" in str(e.value)
