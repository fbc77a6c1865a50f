"""CPU: sdrx_datv_* binds (lib() stamps every symbol's signature, a missing one raises), rejects bad configurations with
SDRX_EINVAL and a text before any device is touched, fails loudly without a device (no CPU fallback), and its accessors refuse a
null handle.  The design getters and the tables are held against the recording where there is a device (tests/test_datv_gpu.py)."""
import ctypes as C

import pytest

import sdrangel_amd as sa
from tests import datv_cases as dc


def _create(n_ch=1, cfgs=None, **kw):
    arr = (sa.DatvCfg * max(n_ch, 1))(*(cfgs or [dc.as_struct(dc.cfg(**kw), sa.DatvCfg)] * max(n_ch, 1)))
    h = C.c_void_p()
    # device 1 << 20 does not exist anywhere: a configuration that passes validation must then fail with SDRX_ENODEV
    rc = sa.lib().sdrx_datv_create(C.byref(h), 1 << 20, n_ch, arr)
    assert not h.value
    return rc, sa.lib().sdrx_last_error().decode()


def test_the_symbols_bind_and_the_header_declares_them():
    names = [n for n in sa.exported_symbols() if n.startswith("sdrx_datv_")]
    assert len(names) == 21, names
    for n in names:
        assert getattr(sa.lib(), n).argtypes is not None, n


def test_the_structs_have_the_headers_layout():
    assert C.sizeof(sa.DatvCfg) == 64 and C.sizeof(sa.DatvState) == 112 and C.sizeof(sa.DatvDesign) == 48 and sa.DATV_MEAS.itemsize == 24
    assert [f[0] for f in sa.DatvCfg._fields_] == [k for k, _ in dc.CFG_FIELDS]
    assert C.sizeof(dc.Cfg) == C.sizeof(sa.DatvCfg) and C.sizeof(dc.State) == C.sizeof(sa.DatvState) and C.sizeof(dc.Design) == C.sizeof(sa.DatvDesign)
    assert C.sizeof(dc.Meas) == sa.DATV_MEAS.itemsize == dc.MEAS_DTYPE.itemsize
    assert sa.DatvState.held.offset == 84 and sa.DatvState.chunks.offset == 88


@pytest.mark.parametrize("kw,text", [
    (dict(notch_filters=1), "notch_filters > 0: auto_notch is not part of the bank"),
    (dict(notch_filters=3), "notch_filters > 0"),
    (dict(modulation=dc.APSK16, fec=dc.FEC12), "Code rate not supported with APSK16"),
    (dict(modulation=dc.APSK16, fec=dc.FEC78), "Code rate not supported with APSK16"),
    (dict(modulation=dc.APSK32, fec=dc.FEC12), "Code rate not supported with APSK32"),
    (dict(modulation=dc.APSK32, fec=dc.FEC23), "Code rate not supported with APSK32"),
    (dict(modulation=dc.APSK32, fec=dc.FEC46), "Code rate not supported with APSK32"),
    (dict(modulation=dc.APSK32, fec=dc.FEC78), "Code rate not supported with APSK32"),
    (dict(rolloff=0.0), "rolloff <= 0 with the RRC sampler"),
    (dict(rolloff=-0.35), "rolloff <= 0 with the RRC sampler"),
    (dict(rolloff=float("nan")), "rolloff <= 0 with the RRC sampler"),
    (dict(rolloff=1.5), "bad rolloff or excursion"),
    (dict(excursion=0), "bad rolloff or excursion"),
    (dict(rolloff=0.01, excursion=40), "more than 4096 coefficients"),
    (dict(rolloff=1.0e-30, excursion=40), "more than 4096 coefficients"),
    (dict(symbol_rate=125000, excursion=40), "more than 64 taps per symbol"),
    (dict(symbol_rate=125000, excursion=30, rolloff=0.339), "more than 64 taps per symbol"),       # 515 coefficients at 8 steps: 65
    (dict(finfo=50000.0), "meas_decimation under 64"),
    (dict(finfo=-1.0), "bad finfo"),
    (dict(finfo=float("nan")), "bad finfo"),
    (dict(modulation=9), "no such modulation"),
    (dict(modulation=-1), "no such modulation"),
    (dict(fec=9), "no such code rate"),
    (dict(sampler=3), "no such sampler"),
    (dict(msps=0), "must be positive"),
    (dict(sample_rate=-1), "must be positive"),
    (dict(symbol_rate=0), "must be positive"),
    (dict(symbol_rate=1000001), "symbol_rate exceeds sample_rate"),
    (dict(rf_bandwidth=-1), "negative rf_bandwidth"),
])
def test_bad_configurations_are_rejected_before_the_device(kw, text):
    rc, msg = _create(**kw)
    assert rc == -1 and msg.startswith("sdrx_datv_create: channel 0: ") and text in msg, (rc, msg)      # SDRX_EINVAL, not SDRX_ENODEV


def test_what_the_rrc_limits_do_not_touch():
    """a rolloff of 0 or an excursion of 0 is refused for the RRC sampler alone; the supported APSK rates pass"""
    for kw in (dict(rolloff=0.0, sampler=dc.LINEAR), dict(rolloff=0.0, excursion=0, sampler=dc.NEAREST), dict(modulation=dc.APSK16, fec=dc.FEC46),
               dict(modulation=dc.APSK32, fec=dc.FEC910), dict(modulation=dc.APSK64E, fec=dc.FEC12), dict(symbol_rate=1000000, sampler=dc.NEAREST),
               dict(symbol_rate=125000, excursion=30, rolloff=0.345), dict(symbol_rate=3333, sampler=dc.LINEAR)):       # 64 taps; omega of 300
        rc, msg = _create(**kw)
        assert rc == -2, (kw, rc, msg)


def test_a_good_configuration_fails_loudly_without_a_device():
    for case in dc.CASES[:8] + dc.random_cases()[:20]:
        rc, msg = _create(**case["cfg"])
        assert rc == -2, (case["name"], rc, msg)                        # SDRX_ENODEV


def test_bad_arguments():
    assert _create(n_ch=0)[0] == -1
    good = dc.as_struct(dc.cfg(), sa.DatvCfg)
    assert sa.lib().sdrx_datv_create(None, 0, 1, (sa.DatvCfg * 1)(good)) == -1
    h = C.c_void_p()
    assert sa.lib().sdrx_datv_create(C.byref(h), 0, 1, None) == -1
    rc, msg = _create(n_ch=2, cfgs=[good, dc.as_struct(dc.cfg(notch_filters=1), sa.DatvCfg)])       # a bad channel anywhere in the list
    assert rc == -1 and "channel 1" in msg
    assert sa.lib().sdrx_datv_destroy(None) == 0


def test_null_handle_accessors():
    L = sa.lib()
    ptrs, ns = (C.c_void_p * 1)(), (C.c_int64 * 1)(0)
    out, p, q, n = (C.c_int16 * 16)(), C.c_void_p(), C.c_void_p(), C.c_int64()
    d = C.c_double()
    st, de = sa.DatvState(), sa.DatvDesign()
    name, a, b, e = C.create_string_buffer(64), C.c_int(), C.c_int(), C.c_int()
    calls = [(L.sdrx_datv_reset, (None,)), (L.sdrx_datv_sync, (None,)), (L.sdrx_datv_feed, (None, ptrs, ns)), (L.sdrx_datv_feed_dev, (None, ptrs, ns)),
             (L.sdrx_datv_feed_bank, (None, None)), (L.sdrx_datv_read, (None, 0, out, None, 1)), (L.sdrx_datv_read_points, (None, 0, out, 1)),
             (L.sdrx_datv_read_meas, (None, 0, out, 1)), (L.sdrx_datv_last_dev, (None, 0, C.byref(p), C.byref(q), C.byref(n))),
             (L.sdrx_datv_points_last_dev, (None, 0, C.byref(p), C.byref(n))), (L.sdrx_datv_meas_last_dev, (None, 0, C.byref(p), C.byref(n))),
             (L.sdrx_datv_state, (None, 0, C.byref(st))), (L.sdrx_datv_get_design, (None, 0, C.byref(de))),
             (L.sdrx_datv_get_tables, (None, 0, None, 0, None, None, None)), (L.sdrx_datv_set_stream, (None, None)), (L.sdrx_datv_get_stream, (None, C.byref(p))),
             (L.sdrx_datv_set_timing, (None, 1)), (L.sdrx_datv_get_timing, (None, C.byref(d), C.byref(n), 0)),
             (L.sdrx_datv_last_launch, (None, name, 64, C.byref(a), C.byref(b), C.byref(e)))]
    for fn, args in calls:
        assert fn(*args) < 0, fn.__name__
