"""CPU: the RDS entry points of the broadcast-FM bank (sdrx_bfmrds_*, on a sdrx_bfm_t).  sdrx_bfmrds_create with a null or all-zero
rds list answers exactly as sdrx_bfm_create does, bad rds_active values are rejected with SDRX_EINVAL and the field's name before
any device is touched, a good configuration fails loudly without a device, and every call refuses a null handle."""
import ctypes as C
import os
import subprocess

import pytest

import sdrangel_amd as sa

GOOD = dict(in_rate=250000, nco_freq=0, audio_rate=48000, rf_bandwidth=200000.0, af_bandwidth=15000.0, volume=2.0, squelch_db=-60.0,
            audio_stereo=1, lsb_stereo=0, show_pilot=0)
CALLS = {"create", "read_bits", "bits_last_dev", "read_groups", "groups_last_dev", "read_bb", "report", "state", "unsure"}
NO_DEVICE = 1 << 20                     # exists nowhere: a configuration that passes validation must then fail with something else


def _create(rds, n_ch=1, cfgs=None, plain=False, **kw):
    d = dict(GOOD); d.update(kw)
    arr = (sa.BfmCfg * max(n_ch, 1))(*(cfgs or [sa.BfmCfg(**d)] * max(n_ch, 1)))
    h = C.c_void_p()
    if plain:
        rc = sa.lib().sdrx_bfm_create(C.byref(h), NO_DEVICE, n_ch, arr)
    else:
        flags = None if rds is None else (sa.BfmRdsCfg * max(n_ch, 1))(*[sa.BfmRdsCfg(int(v)) for v in rds])
        rc = sa.lib().sdrx_bfmrds_create(C.byref(h), NO_DEVICE, n_ch, arr, flags)
    assert not h.value
    return rc, sa.lib().sdrx_last_error().decode()


def test_symbols():
    declared = {s for s in sa.exported_symbols() if s.startswith("sdrx_bfmrds_")}
    assert declared == {"sdrx_bfmrds_" + c for c in CALLS}
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(os.path.dirname(sa.__file__), "libsdrx.so")], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l and l.split()[-1].startswith("sdrx_bfmrds_")}
    assert exported == declared
    for s in declared:
        assert getattr(sa.lib(), s).argtypes is not None, s


def test_layouts():
    assert C.sizeof(sa.BfmRdsCfg) == 4 and C.sizeof(sa.BfmRdsState) == 208
    assert sa.BfmRdsState.reg.offset == 120 and sa.BfmRdsState.group.offset == 160 and sa.BfmRdsState.decoder_qua.offset == 200


@pytest.mark.parametrize("kw", [dict(), dict(audio_stereo=0), dict(in_rate=240000), dict(audio_rate=0), dict(rf_bandwidth=float("nan")),
                                dict(lsb_stereo=3), dict(in_rate=-1)])
def test_null_and_zero_rds_answer_as_create_does(kw):
    want = _create(None, plain=True, **kw)
    assert _create(None, **kw) == want and _create([0], **kw) == want
    assert _create([0, 0, 0], n_ch=3, **kw) == _create(None, n_ch=3, plain=True, **kw)


@pytest.mark.parametrize("value", [2, -1, 255])
def test_bad_rds_active_is_rejected_before_the_device(value):
    rc, msg = _create([value])
    assert rc == -1 and "rds_active" in msg, (rc, msg)
    rc, msg = _create([1, 0, value], n_ch=3)                         # anywhere in the list
    assert rc == -1 and "rds_active" in msg, (rc, msg)


@pytest.mark.parametrize("kw", [dict(), dict(audio_stereo=0), dict(in_rate=240000, rf_bandwidth=180000.0), dict(in_rate=384000), dict(in_rate=48000)])
def test_good_configurations_reach_the_device_check(kw):
    rc, msg = _create([1], **kw)
    assert rc not in (0, -1), (rc, msg)


def test_bad_arguments():
    L = sa.lib()
    arr = (sa.BfmCfg * 1)(sa.BfmCfg(**GOOD))
    one = (sa.BfmRdsCfg * 1)(sa.BfmRdsCfg(1))
    h = C.c_void_p()
    assert L.sdrx_bfmrds_create(None, 0, 1, arr, one) == -1
    assert L.sdrx_bfmrds_create(C.byref(h), 0, 0, arr, one) == -1 and not h.value
    assert L.sdrx_bfmrds_create(C.byref(h), 0, 1, None, one) == -1 and not h.value
    assert L.sdrx_bfmrds_read_bits(None, 0, None, 0) == -1 and L.sdrx_bfmrds_read_groups(None, 0, None, 0) == -1
    assert L.sdrx_bfmrds_read_bb(None, 0, None, 0) == -1
    assert L.sdrx_bfmrds_bits_last_dev(None, 0, None, None) == -1 and L.sdrx_bfmrds_groups_last_dev(None, 0, None, None) == -1
    assert L.sdrx_bfmrds_report(None, 0, None, None, None, None, None) == -1
    assert L.sdrx_bfmrds_state(None, 0, None) == -1 and L.sdrx_bfmrds_unsure(None, 0, 0) == -1
    for name in ("read_bits", "read_groups", "read_bb"):
        assert getattr(L, "sdrx_bfmrds_" + name)(None, 0, None, -1) == -1
        assert "sdrx_bfmrds_" + name in L.sdrx_last_error().decode()


def test_no_cpu_fallback():
    if sa.lib().sdrx_device_count() > 0:
        return                              # a HIP device is present: tests/test_bfm_rds_gpu.py runs there
    with pytest.raises(sa.SdrxError) as e:
        sa.BfmBank([sa.BfmCfg(**GOOD)], rds=[1])
    assert "rc=-2" in str(e.value)
