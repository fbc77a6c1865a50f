"""CPU: sdrx_am_create_ex rejects bad sync configurations with SDRX_EINVAL and a message that names the field before any device is
touched, fails loudly without a device, takes a null sync list like sdrx_am_create, and the new symbols are exported and
declared in include/sdrx.h."""
import ctypes as C
import os
import re

import pytest

import sdrangel_amd as sa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOOD = dict(in_rate=16000, nco_freq=-300, audio_rate=8000, rf_bandwidth=3000.0, volume=1.0, squelch_db=-40.0, audio_mute=0, bandpass_enable=0)


def _create(sync_kw, n_ch=1, null_sync=False, **kw):
    d = dict(GOOD); d.update(kw)
    arr = (sa.AmCfg * n_ch)(*[sa.AmCfg(**d)] * n_ch)
    syncs = sync_kw if isinstance(sync_kw, list) else [sync_kw] * n_ch
    sarr = None if null_sync else (sa.AmSyncCfg * n_ch)(*[sa.AmSyncCfg(**s) for s in syncs])
    h = C.c_void_p()
    # device 1 << 20 does not exist anywhere: a configuration that passes validation must then fail with SDRX_ENODEV
    rc = sa.lib().sdrx_am_create_ex(C.byref(h), 1 << 20, n_ch, arr, sarr)
    assert not h.value
    return rc, sa.lib().sdrx_last_error().decode()


def test_symbols_are_exported_and_declared():
    header = open(os.path.join(ROOT, "include", "sdrx.h")).read()
    for fn in ("sdrx_am_create_ex", "sdrx_am_pll", "sdrx_am_get_sync_design"):
        assert hasattr(sa.lib(), fn), fn
        assert re.search(r"\bint\s+" + fn + r"\s*\(", header), fn
    assert "typedef struct sdrx_am_sync_cfg" in header
    left_out = header[header.index("AM demodulator bank:"):header.index("typedef struct sdrx_am sdrx_am_t")]
    assert "left out: m_pll" not in left_out and "mode\n *     change" in left_out


def test_sync_struct_matches_the_header():
    assert C.sizeof(sa.AmSyncCfg) == 16
    assert [getattr(sa.AmSyncCfg, f).offset for f in ("pll", "sync_op", "ssb_design_rate", "ssb_design_bw")] == [0, 4, 8, 12]
    assert C.sizeof(sa.AmCfg) == 32


@pytest.mark.parametrize("sync,field", [(dict(pll=1, sync_op=3), "sync_op"), (dict(pll=1, sync_op=-1), "sync_op"), (dict(sync_op=7), "sync_op"),
                                        (dict(pll=1, ssb_design_rate=-1), "ssb_design_rate"), (dict(pll=1, sync_op=1, ssb_design_rate=-48000), "ssb_design_rate"),
                                        (dict(pll=1, ssb_design_bw=-1.0), "ssb_design_bw"), (dict(pll=1, ssb_design_bw=float("nan")), "ssb_design_bw"),
                                        (dict(pll=1, sync_op=2, ssb_design_bw=float("inf")), "ssb_design_bw")])
def test_bad_sync_configurations_are_rejected_before_the_device(sync, field):
    rc, msg = _create(sync)
    assert rc == -1 and "sdrx_am_create_ex" in msg and field in msg, (rc, msg)      # SDRX_EINVAL, not SDRX_ENODEV


@pytest.mark.parametrize("kw", [dict(audio_rate=16001), dict(audio_rate=999), dict(rf_bandwidth=0.0), dict(volume=float("nan"))])
def test_bad_base_configurations_are_still_rejected(kw):
    rc, msg = _create(dict(pll=1, sync_op=1), **kw)
    assert rc == -1 and "sdrx_am_create" in msg, (rc, msg)


def test_a_bad_channel_anywhere_in_the_list():
    assert _create([dict(pll=1), dict(pll=1, sync_op=5)], n_ch=2)[0] == -1


@pytest.mark.parametrize("sync", [dict(), dict(pll=1), dict(pll=1, sync_op=1), dict(pll=1, sync_op=2), dict(pll=0, sync_op=2),
                                  dict(pll=1, sync_op=1, ssb_design_rate=8000, ssb_design_bw=3000.0), dict(pll=1, sync_op=2, ssb_design_rate=48000)])
def test_a_good_configuration_reaches_the_device_check(sync):
    rc, msg = _create(sync)
    assert rc == -2, (rc, msg)                                      # SDRX_ENODEV: validation passed, the device index did not
    assert _create([sync, dict(), dict(pll=1, sync_op=1), dict(pll=1, sync_op=2)], n_ch=4)[0] == -2


def test_null_sync_list_is_accepted_like_create():
    assert _create(None, null_sync=True)[0] == -2
    assert _create(None, null_sync=True, audio_rate=16001)[0] == -1


def test_bad_arguments():
    L = sa.lib()
    cfg, sync = (sa.AmCfg * 1)(sa.AmCfg(**GOOD)), (sa.AmSyncCfg * 1)(sa.AmSyncCfg(pll=1))
    h = C.c_void_p()
    assert L.sdrx_am_create_ex(None, 0, 1, cfg, sync) == -1
    assert L.sdrx_am_create_ex(C.byref(h), 0, 0, cfg, sync) == -1
    assert L.sdrx_am_create_ex(C.byref(h), 0, 1, None, sync) == -1
    k, f = C.c_int32(), C.c_float()
    assert L.sdrx_am_pll(None, 0, C.byref(k), C.byref(f)) == -1
    assert L.sdrx_am_get_sync_design(None, 0, None, None, None, None) == -1


def test_python_face():
    with pytest.raises(ValueError):
        sa.AmDemodBank([sa.AmCfg(**GOOD)], sync=[])
    # no CPU fallback: a device index that does not exist is an error with or without a GPU in the machine
    with pytest.raises(sa.SdrxError) as e:
        sa.AmDemodBank([sa.AmCfg(**GOOD)], device=1 << 20, sync=[sa.AmSyncCfg(pll=1)])
    assert "rc=-2" in str(e.value) and "sdrx_am_create_ex" in str(e.value)
