"""CPU: sdrx_chanapll_create and sdrx_chanapll_state exist next to sdrx_chana_*, whose create still rejects the PLL; the new create
accepts it, rejects a psk_order outside 1 .. 31 and what the old one rejected otherwise with SDRX_EINVAL before any device is
touched, and fails loudly without a device (no CPU fallback)."""
import ctypes as C

import pytest

import sdrangel_amd as sa

GOOD = dict(in_rate=48000, nco_freq=-3000, down_sample=0, down_sample_rate=0, bandwidth=5000, low_cutoff=300, span_log2=0, ssb=0, rrc=0,
            rrc_rolloff=35, input_type=0, pll=1, fll=0)


def _create(n_ch=1, order=None, old=False, **kw):
    d = dict(GOOD); d.update(kw)
    arr = (sa.ChanaCfg * n_ch)(*[sa.ChanaCfg(**d)] * n_ch)
    h = C.c_void_p()
    # device 1 << 20 does not exist anywhere: a configuration that passes validation must then fail with something else than EINVAL
    if old:
        rc = sa.lib().sdrx_chana_create(C.byref(h), 1 << 20, n_ch, arr)
    else:
        rc = sa.lib().sdrx_chanapll_create(C.byref(h), 1 << 20, n_ch, arr, (C.c_int32 * n_ch)(*order) if order is not None else None)
    assert not h.value
    return rc, sa.lib().sdrx_last_error().decode()


def test_symbols_exist_and_are_declared():
    declared = set(sa.exported_symbols())
    for name in ("sdrx_chanapll_create", "sdrx_chanapll_state"):
        assert name in declared and getattr(sa.lib(), name)
    assert {s for s in declared if s.startswith("sdrx_chanapll_")} == {"sdrx_chanapll_create", "sdrx_chanapll_state"}


@pytest.mark.parametrize("kw,reason", [(dict(pll=1), "PLL"), (dict(pll=0, fll=1), "FLL"), (dict(pll=1, fll=1), "PLL"), (dict(pll=0, input_type=1), "PLL input")])
def test_the_old_create_still_rejects_the_pll(kw, reason):
    rc, msg = _create(old=True, **kw)
    assert rc == -1 and "sdrx_chana_create" in msg and reason in msg, (rc, msg)


@pytest.mark.parametrize("kw", [dict(), dict(fll=1), dict(pll=0, fll=1), dict(pll=0), dict(input_type=1), dict(pll=0, input_type=1), dict(input_type=2),
                                dict(ssb=1, bandwidth=-5000, input_type=1, fll=1), dict(span_log2=8), dict(down_sample=1, down_sample_rate=12000)])
@pytest.mark.parametrize("order", [None, [1], [2], [31]])
def test_pll_configurations_pass_validation_and_fail_on_the_device(kw, order):
    rc, msg = _create(order=order, **kw)
    assert rc not in (0, -1), (rc, msg)


@pytest.mark.parametrize("order", [[0], [32], [-1], [1 << 20]])
def test_psk_order_out_of_range_is_rejected_before_the_device(order):
    rc, msg = _create(order=order)
    assert rc == -1 and "sdrx_chanapll_create" in msg and "psk_order" in msg, (rc, msg)
    rc, msg = _create(n_ch=3, order=[1, 4] + order)
    assert rc == -1 and "psk_order" in msg, (rc, msg)


@pytest.mark.parametrize("kw,reason", [
    (dict(input_type=3), "input_type"), (dict(input_type=-1), "input_type"), (dict(span_log2=-1), "span_log2"), (dict(span_log2=9), "span_log2"),
    (dict(rrc_rolloff=101), "rrc_rolloff"), (dict(rrc_rolloff=-1), "rrc_rolloff"), (dict(down_sample=1, down_sample_rate=0), "down_sample_rate"),
    (dict(down_sample=1, down_sample_rate=48001), "down_sample_rate"), (dict(in_rate=0), "in_rate"), (dict(nco_freq=48001), "nco_freq")])
def test_the_old_bad_configurations_are_rejected_before_the_device(kw, reason):
    rc, msg = _create(order=[2], **kw)
    assert rc == -1 and "sdrx_chanapll_create" in msg and reason in msg, (rc, msg)


def test_bad_arguments_and_null_handle():
    L = sa.lib()
    arr = (sa.ChanaCfg * 1)(sa.ChanaCfg(**GOOD))
    assert L.sdrx_chanapll_create(None, 0, 1, arr, None) == -1
    h = C.c_void_p()
    assert L.sdrx_chanapll_create(C.byref(h), 0, 0, arr, None) == -1 and not h.value
    assert L.sdrx_chanapll_create(C.byref(h), 0, 1, None, None) == -1 and not h.value
    k, f, d, p = C.c_int32(), C.c_float(), C.c_float(), C.c_float()
    assert L.sdrx_chanapll_state(None, 0, C.byref(k), C.byref(f), C.byref(d), C.byref(p)) == -1
    assert L.sdrx_chanapll_state(None, 0, None, None, None, None) == -1
