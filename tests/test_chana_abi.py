"""CPU: sdrx_chana_* exists, rejects bad configurations with SDRX_EINVAL and a message naming the reason before any device is
touched, fails loudly without a device (no CPU fallback), and its accessors refuse a null handle."""
import ctypes as C

import pytest

import sdrangel_amd as sa

GOOD = dict(in_rate=48000, nco_freq=-3000, down_sample=0, down_sample_rate=0, bandwidth=5000, low_cutoff=300, span_log2=0, ssb=0, rrc=0,
            rrc_rolloff=35, input_type=0, pll=0, fll=0)
ENTRIES = ("create", "destroy", "reset", "feed", "feed_dev", "feed_bank", "read", "last_dev", "positive_only", "magsq", "get_design", "seek",
           "sync", "set_stream", "get_stream", "set_timing", "get_timing", "last_launch")


def _create(n_ch=1, cfgs=None, **kw):
    d = dict(GOOD); d.update(kw)
    arr = (sa.ChanaCfg * max(n_ch, 1))(*(cfgs or [sa.ChanaCfg(**d)] * max(n_ch, 1)))
    h = C.c_void_p()
    # device 1 << 20 does not exist anywhere: a configuration that passes validation must then fail with SDRX_ENODEV
    rc = sa.lib().sdrx_chana_create(C.byref(h), 1 << 20, n_ch, arr)
    assert not h.value
    return rc, sa.lib().sdrx_last_error().decode()


def test_symbols_exist_and_are_declared():
    declared = set(sa.exported_symbols())
    for name in ENTRIES:
        assert f"sdrx_chana_{name}" in declared, name
        assert getattr(sa.lib(), f"sdrx_chana_{name}")
    assert {s for s in declared if s.startswith("sdrx_chana_")} == {f"sdrx_chana_{n}" for n in ENTRIES}
    assert [f[0] for f in sa.ChanaCfg._fields_] == list(GOOD)
    assert C.sizeof(sa.ChanaCfg) == 13 * 4


@pytest.mark.parametrize("kw,reason", [
    (dict(pll=1), "PLL"), (dict(fll=1), "FLL"), (dict(pll=1, fll=1), "PLL"), (dict(input_type=1), "PLL input"),
    (dict(input_type=3), "input_type"), (dict(input_type=-1), "input_type"),
    (dict(span_log2=-1), "span_log2"), (dict(span_log2=9), "span_log2"),
    (dict(rrc_rolloff=101), "rrc_rolloff"), (dict(rrc=1, rrc_rolloff=1000), "rrc_rolloff"), (dict(rrc_rolloff=-1), "rrc_rolloff"),
    (dict(down_sample=1, down_sample_rate=0), "down_sample_rate"), (dict(down_sample=1, down_sample_rate=48001), "down_sample_rate"),
    (dict(down_sample=1, down_sample_rate=-12000), "down_sample_rate"),
    (dict(in_rate=0), "in_rate"), (dict(in_rate=-48000), "in_rate"), (dict(nco_freq=48001), "nco_freq"), (dict(nco_freq=-(1 << 31)), "nco_freq")])
def test_bad_configurations_are_rejected_before_the_device(kw, reason):
    rc, msg = _create(**kw)
    assert rc == -1 and "sdrx_chana_create" in msg and reason in msg, (rc, msg)         # SDRX_EINVAL, not SDRX_ENODEV


@pytest.mark.parametrize("kw", [dict(), dict(ssb=1), dict(ssb=1, bandwidth=-5000), dict(bandwidth=50), dict(rrc=1, rrc_rolloff=0), dict(rrc=1, rrc_rolloff=100),
                                dict(span_log2=8), dict(input_type=2), dict(down_sample=1, down_sample_rate=48000), dict(down_sample=1, down_sample_rate=1),
                                dict(down_sample_rate=99999), dict(nco_freq=48000), dict(nco_freq=-48000), dict(ssb=1, bandwidth=2000, low_cutoff=6000)])
def test_good_configurations_pass_validation_and_fail_on_the_device(kw):
    rc, msg = _create(**kw)
    assert rc not in (0, -1), (rc, msg)                              # no device of that number: not EINVAL, and no CPU fallback


def test_bad_arguments():
    assert _create(n_ch=0)[0] == -1
    assert sa.lib().sdrx_chana_create(None, 0, 1, (sa.ChanaCfg * 1)(sa.ChanaCfg(**GOOD))) == -1
    h = C.c_void_p()
    assert sa.lib().sdrx_chana_create(C.byref(h), 0, 1, None) == -1
    # a bad channel anywhere in the list
    cfgs = [sa.ChanaCfg(**GOOD), sa.ChanaCfg(**dict(GOOD, span_log2=9))]
    assert _create(n_ch=2, cfgs=cfgs)[0] == -1
    assert sa.lib().sdrx_chana_destroy(None) == 0


def test_null_handle_accessors():
    L = sa.lib()
    ptrs, ns = (C.c_void_p * 1)(), (C.c_int64 * 1)(0)
    out, p, n = (C.c_int16 * 8)(), C.c_void_p(), C.c_int64()
    d, nt, inc = C.c_double(), C.c_int32(), C.c_float()
    name, a, b, c = C.create_string_buffer(64), C.c_int(), C.c_int(), C.c_int()
    calls = [(L.sdrx_chana_reset, (None,)), (L.sdrx_chana_sync, (None,)), (L.sdrx_chana_feed, (None, ptrs, ns)), (L.sdrx_chana_feed_dev, (None, ptrs, ns)),
             (L.sdrx_chana_feed_bank, (None, None)), (L.sdrx_chana_read, (None, 0, out, 4)), (L.sdrx_chana_last_dev, (None, 0, C.byref(p), C.byref(n))),
             (L.sdrx_chana_positive_only, (None, 0)), (L.sdrx_chana_magsq, (None, 0, C.byref(d))),
             (L.sdrx_chana_get_design, (None, 0, C.byref(nt), None, 0, None, C.byref(inc))), (L.sdrx_chana_seek, (None, 0, 5)),
             (L.sdrx_chana_set_stream, (None, None)), (L.sdrx_chana_get_stream, (None, C.byref(p))), (L.sdrx_chana_set_timing, (None, 1)),
             (L.sdrx_chana_get_timing, (None, C.byref(d), C.byref(n), 0)),
             (L.sdrx_chana_last_launch, (None, name, 64, C.byref(a), C.byref(b), C.byref(c)))]
    for fn, args in calls:
        assert fn(*args) == -1, fn.__name__
