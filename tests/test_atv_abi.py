"""CPU: sdrx_atv_* binds (lib() stamps every symbol's signature, a missing one raises), rejects bad configurations with
SDRX_EINVAL and a text before any device is touched, fails loudly without a device (no CPU fallback), and its accessors refuse a
null handle.  The design getters are held against the recording's integers where there is a device (tests/test_atv_gpu.py), and
the same integers from atv_scan.hpp against the recording here (tests/test_atv_host.py)."""
import ctypes as C

import pytest

import sdrangel_amd as sa
from tests import atv_cases as ac


def _create(n_ch=1, cfgs=None, **kw):
    arr = (sa.AtvCfg * max(n_ch, 1))(*(cfgs or [ac.as_struct(ac.cfg(**kw), sa.AtvCfg)] * max(n_ch, 1)))
    h = C.c_void_p()
    # device 1 << 20 does not exist anywhere: a configuration that passes validation must then fail with SDRX_ENODEV
    rc = sa.lib().sdrx_atv_create(C.byref(h), 1 << 20, n_ch, arr)
    assert not h.value
    return rc, sa.lib().sdrx_last_error().decode()


def test_the_symbols_bind_and_the_header_declares_them():
    names = [n for n in sa.exported_symbols() if n.startswith("sdrx_atv_")]
    assert len(names) == 23, names
    for n in names:
        assert getattr(sa.lib(), n).argtypes is not None, n


def test_the_structs_have_the_headers_layout():
    assert C.sizeof(sa.AtvCfg) == 80 and C.sizeof(sa.AtvState) == 112 and C.sizeof(sa.AtvDesign) == 48
    assert [f[0] for f in sa.AtvCfg._fields_] == [k for k, _ in ac.CFG_FIELDS]
    assert C.sizeof(ac.Cfg) == C.sizeof(sa.AtvCfg) and C.sizeof(ac.State) == C.sizeof(sa.AtvState) and C.sizeof(ac.Design) == C.sizeof(sa.AtvDesign)


@pytest.mark.parametrize("kw,text", [
    (dict(modulation=ac.USB), "USB and LSB are left out"),
    (dict(modulation=ac.LSB), "USB and LSB are left out"),
    (dict(modulation=6), "bad modulation"),
    (dict(modulation=-1), "bad modulation"),
    (dict(standard=6), "bad standard"),
    (dict(level_black=1.0), "level_black >= 1"),
    (dict(level_black=1.5), "level_black >= 1"),
    (dict(level_black=float("nan")), "level_black >= 1"),
    (dict(n_lines=1, frames_per_s=0.5), "n_lines * frames_per_s < 1"),
    (dict(n_lines=0), "n_lines * frames_per_s < 1"),
    (dict(frames_per_s=0.0), "n_lines * frames_per_s < 1"),
    (dict(frames_per_s=float("nan")), "n_lines * frames_per_s < 1"),
    (dict(n_lines=4), "no rows or no columns"),                     # the Short standard's four black lines leave no row
    (dict(line_duration=0.0), "no rows or no columns"),
    (dict(line_duration=1.0e-6), "no rows or no columns"),
    (dict(line_duration=-1.0), "bad line or top duration"),
    (dict(top_duration=float("nan")), "bad line or top duration"),
    (dict(line_duration=1.0e9), "bad line or top duration"),
    (dict(in_rate=0), "bad rate"),
    (dict(in_rate=-160000), "bad rate"),
    (dict(fm_deviation=0.0), "bad fm_deviation"),
    (dict(fm_deviation=float("nan")), "bad fm_deviation"),
    (dict(frames_cap=0), "frames_cap < 1"),
    (dict(frames_cap=1 << 30), "exceed 1 GiB"),
    (dict(fft_filtering=1, rf_bw=0.0), "bad rf_bw"),
    (dict(decimator_enable=1, rf_bw=float("nan")), "bad rf_bw"),
    (dict(decimator_enable=1, rf_bw=-5.0), "bad rf_bw"),
    (dict(fft_filtering=1, rf_opp_bw=-1.0), "bad rf_opp_bw"),
])
def test_bad_configurations_are_rejected_before_the_device(kw, text):
    rc, msg = _create(**kw)
    assert rc == -1 and msg.startswith("sdrx_atv_create: channel 0: ") and text in msg, (rc, msg)      # SDRX_EINVAL, not SDRX_ENODEV


def test_a_good_configuration_fails_loudly_without_a_device():
    for case in ac.CASES[:8]:
        rc, msg = _create(**case["cfg"])
        assert rc == -2, (case["name"], rc, msg)                        # SDRX_ENODEV


def test_bad_arguments():
    assert _create(n_ch=0)[0] == -1
    good = ac.as_struct(ac.cfg(), sa.AtvCfg)
    assert sa.lib().sdrx_atv_create(None, 0, 1, (sa.AtvCfg * 1)(good)) == -1
    h = C.c_void_p()
    assert sa.lib().sdrx_atv_create(C.byref(h), 0, 1, None) == -1
    rc, msg = _create(n_ch=2, cfgs=[good, ac.as_struct(ac.cfg(modulation=ac.USB), sa.AtvCfg)])       # a bad channel anywhere in the list
    assert rc == -1 and "channel 1" in msg
    assert sa.lib().sdrx_atv_destroy(None) == 0


def test_null_handle_accessors():
    L = sa.lib()
    ptrs, ns = (C.c_void_p * 1)(), (C.c_int64 * 1)(0)
    out, p, n, m = (C.c_int16 * 4)(), C.c_void_p(), C.c_int64(), C.c_int64()
    r, c, d = C.c_int32(), C.c_int32(), C.c_double()
    st, de = sa.AtvState(), sa.AtvDesign()
    name, a, b, e = C.create_string_buffer(64), C.c_int(), C.c_int(), C.c_int()
    calls = [(L.sdrx_atv_reset, (None,)), (L.sdrx_atv_sync, (None,)), (L.sdrx_atv_feed, (None, ptrs, ns)), (L.sdrx_atv_feed_dev, (None, ptrs, ns)),
             (L.sdrx_atv_feed_bank, (None, None)), (L.sdrx_atv_frames, (None, 0, C.byref(n))), (L.sdrx_atv_read_events, (None, 0, out, 1)),
             (L.sdrx_atv_read_frame, (None, 0, 0, out, 8)), (L.sdrx_atv_read_screen, (None, 0, out, 8)),
             (L.sdrx_atv_frames_last_dev, (None, 0, C.byref(p), C.byref(n), C.byref(m))), (L.sdrx_atv_screen_last_dev, (None, 0, C.byref(p), C.byref(r), C.byref(c))),
             (L.sdrx_atv_read, (None, 0, out, 1)), (L.sdrx_atv_last_dev, (None, 0, C.byref(p), C.byref(n))), (L.sdrx_atv_state, (None, 0, C.byref(st))),
             (L.sdrx_atv_get_design, (None, 0, C.byref(de))), (L.sdrx_atv_get_filters, (None, 0, C.byref(r), None, 0, None, None)), (L.sdrx_atv_set_stream, (None, None)), (L.sdrx_atv_get_stream, (None, C.byref(p))),
             (L.sdrx_atv_set_timing, (None, 1)), (L.sdrx_atv_get_timing, (None, C.byref(d), C.byref(n), 0)),
             (L.sdrx_atv_last_launch, (None, name, 64, C.byref(a), C.byref(b), C.byref(e)))]
    for fn, args in calls:
        assert fn(*args) < 0, fn.__name__
