"""sdrangel_amd -- ctypes face of libsdrx.so (the MI355X engine for SDRangel's sdrbase/dsp RX path).

The product is the C-ABI shared library (include/sdrx.h); this module only loads it and gives
tests / bench.py numpy-friendly wrappers whose names follow the reference classes
(`Decimators`, `DownChannelizer` bank, `SampleSinkFifo`).  There is no CPU fallback: if the
library is missing, or no HIP device is present when a GPU object is created, it raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libsdrx.so")

FC_INF, FC_SUP, FC_CEN = 0, 1, 2
MODE_CENTER, MODE_LOWER, MODE_UPPER = 0, 1, 2

_lib = None


class SdrxError(RuntimeError):
    pass


def _share_hip_runtime_with_torch() -> None:
    """One HIP runtime per process.  PyTorch-ROCm wheels carry a private libamdhip64.so with the
    same SONAME (libamdhip64.so.7) as /opt/rocm's.  If libsdrx.so pulled in ROCm's copy first and
    torch its own later, the process would hold two runtimes and the second would see no GPU.
    Loading torch's copy first (by path, without importing torch) makes both resolve to it."""
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    p = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(p):
        C.CDLL(p, mode=C.RTLD_GLOBAL)


def lib() -> C.CDLL:
    """Load libsdrx.so (built in-tree by `make -C sdrangel_amd/csrc` / __graft_entry__.build())."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SdrxError(f"{LIB_PATH} not built: run `python -c 'import __graft_entry__ as g; g.build()'`")
    _share_hip_runtime_with_torch()
    L = C.CDLL(LIB_PATH)
    vp, i32, i64, u32 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint32
    pp = C.POINTER(C.c_void_p)
    sig = {
        "sdrx_version": (C.c_char_p, []),
        "sdrx_last_error": (C.c_char_p, []),
        "sdrx_device_count": (C.c_int, []),
        "sdrx_decim_create": (C.c_int, [pp, C.c_int, C.c_int, C.c_int, C.c_int]),
        "sdrx_decim_create_u8": (C.c_int, [pp, C.c_int, C.c_int, C.c_int, C.c_int]),
        "sdrx_decim_process_u8": (C.c_int, [vp, vp, i32, vp, C.POINTER(i32)]),
        "sdrx_decim_process_dev_u8": (C.c_int, [vp, vp, i64, vp, C.POINTER(i64)]),
        "sdrx_decim_destroy": (C.c_int, [vp]),
        "sdrx_decim_reset": (C.c_int, [vp]),
        "sdrx_decim_process": (C.c_int, [vp, vp, i32, vp, C.POINTER(i32)]),
        "sdrx_decim_process_dev": (C.c_int, [vp, vp, i64, vp, C.POINTER(i64)]),
        "sdrx_decim_process_dev_batch": (C.c_int, [vp, i32, vp, vp, vp, vp]),
        "sdrx_decim_ring_create": (C.c_int, [vp, i32, i32, i32]),
        "sdrx_decim_ring_destroy": (C.c_int, [vp]),
        "sdrx_decim_ring_acquire": (vp, [vp]),
        "sdrx_decim_ring_submit": (C.c_int, [vp, i32]),
        "sdrx_decim_ring_retire": (C.c_int, [vp, C.POINTER(vp), C.POINTER(i32)]),
        "sdrx_decim_group_int16": (C.c_int, [C.c_int, C.c_int]),
        "sdrx_decim_state_bytes": (i64, [vp]),
        "sdrx_decim_get_state": (C.c_int, [vp, vp]),
        "sdrx_decim_set_state": (C.c_int, [vp, vp]),
        "sdrx_decim_last_fallback": (C.c_int, [vp, C.POINTER(i64), C.POINTER(i64), vp, i64]),
        "sdrx_chan_bank_create": (C.c_int, [pp, C.c_int, i32, i32, vp, vp]),
        "sdrx_chan_bank_destroy": (C.c_int, [vp]),
        "sdrx_chan_bank_info": (C.c_int, [vp, i32, C.POINTER(i32), vp, C.POINTER(i32), C.POINTER(i32)]),
        "sdrx_chan_plan": (C.c_int, [i32, i32, i32, vp, C.POINTER(i32), C.POINTER(i32)]),
        "sdrx_chan_bank_reconfigure": (C.c_int, [vp, i32, i32, i32]),
        "sdrx_chan_bank_reset": (C.c_int, [vp]),
        "sdrx_chan_bank_add_channel": (C.c_int, [vp, i32, i32, C.POINTER(i32)]),
        "sdrx_chan_bank_remove_channel": (C.c_int, [vp, i32]),
        "sdrx_chan_bank_group_count": (i32, [vp]),
        "sdrx_chan_bank_feed": (C.c_int, [vp, vp, i64]),
        "sdrx_chan_bank_feed_dev": (C.c_int, [vp, vp, i64]),
        "sdrx_chan_bank_available": (i64, [vp, i32]),
        "sdrx_chan_bank_read": (i64, [vp, i32, vp, i64]),
        "sdrx_chan_bank_skip": (i64, [vp, i32, i64]),
        "sdrx_chan_bank_last_dev": (C.c_int, [vp, i32, pp, C.POINTER(i64)]),
        "sdrx_backend_create": (C.c_int, [pp, C.c_int, i32, vp]),
        "sdrx_backend_destroy": (C.c_int, [vp]),
        "sdrx_backend_feed": (C.c_int, [vp, vp, vp]),
        "sdrx_backend_feed_dev": (C.c_int, [vp, vp, vp]),
        "sdrx_backend_feed_bank": (C.c_int, [vp, vp]),
        "sdrx_measure_hbm_read": (C.c_int, [C.c_int, C.c_uint64, C.c_int32, C.POINTER(C.c_double)]),
        "sdrx_dccorr_create": (C.c_int, [C.POINTER(vp), C.c_int]),
        "sdrx_dccorr_destroy": (C.c_int, [vp]),
        "sdrx_dccorr_reset": (C.c_int, [vp]),
        "sdrx_dccorr_process": (C.c_int, [vp, vp, C.c_int64]),
        "sdrx_dccorr_process_dev": (C.c_int, [vp, vp, vp, C.c_int64]),
        "sdrx_iqimb_create": (C.c_int, [C.POINTER(vp), C.c_int, i32]),
        "sdrx_iqimb_destroy": (C.c_int, [vp]),
        "sdrx_iqimb_reset": (C.c_int, [vp]),
        "sdrx_iqimb_process": (C.c_int, [vp, vp, vp]),
        "sdrx_iqimb_process_dev": (C.c_int, [vp, vp, vp, vp]),
        "sdrx_fdecim_create": (C.c_int, [C.POINTER(vp), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
        "sdrx_fdecim_destroy": (C.c_int, [vp]),
        "sdrx_fdecim_reset": (C.c_int, [vp]),
        "sdrx_fdecim_process": (C.c_int, [vp, vp, C.c_int32, vp, C.POINTER(C.c_int32)]),
        "sdrx_fdecim_process_dev": (C.c_int, [vp, vp, C.c_int64, vp, C.POINTER(C.c_int64)]),
        "sdrx_fdecim_group": (C.c_int32, [C.c_int, C.c_int]),
        "sdrx_backend_read": (i64, [vp, i32, vp, i64]),
        "sdrx_backend_last_dev": (C.c_int, [vp, i32, pp, C.POINTER(i64)]),
        "sdrx_backend_get_design": (C.c_int, [vp, i32, C.POINTER(i32), vp, i32, vp, C.POINTER(i32)]),
        "sdrx_audiotail_create": (C.c_int, [pp, C.c_int, i32, vp]),
        "sdrx_audiotail_destroy": (C.c_int, [vp]),
        "sdrx_audiotail_reset": (C.c_int, [vp]),
        "sdrx_audiotail_feed": (C.c_int, [vp, vp, vp, vp]),
        "sdrx_audiotail_feed_dev": (C.c_int, [vp, vp, vp, vp]),
        "sdrx_iir_create": (C.c_int, [pp, C.c_int, i32, vp]),
        "sdrx_iir_destroy": (C.c_int, [vp]),
        "sdrx_iir_reset": (C.c_int, [vp]),
        "sdrx_iir_feed": (C.c_int, [vp, vp, vp, vp]),
        "sdrx_decim24_create": (C.c_int, [pp, C.c_int, C.c_int, C.c_int, C.c_int]),
        "sdrx_decim24_destroy": (C.c_int, [vp]),
        "sdrx_decim24_reset": (C.c_int, [vp]),
        "sdrx_decim24_process": (C.c_int, [vp, vp, i32, vp, C.POINTER(i32)]),
        "sdrx_decim_stages_create": (C.c_int, [pp, C.c_int]),
        "sdrx_decim_stages_destroy": (C.c_int, [vp]),
        "sdrx_decim_save_stages": (C.c_int, [vp, vp]),
        "sdrx_decim_load_stages": (C.c_int, [vp, vp]),
        "sdrx_fanout_create": (C.c_int, [pp, C.c_int, i32, vp, i64]),
        "sdrx_fanout_destroy": (C.c_int, [vp]),
        "sdrx_fanout_send": (C.c_int, [vp, vp, i64, vp]),
        "sdrx_fanout_buffer": (vp, [vp, i32]),
        "sdrx_fanout_wait": (C.c_int, [vp, i32]),
        "sdrx_fanout_stream_wait": (C.c_int, [vp, i32, vp]),
        "sdrx_spectrum_create": (C.c_int, [pp, C.c_int, vp]),
        "sdrx_spectrum_destroy": (C.c_int, [vp]),
        "sdrx_spectrum_reset": (C.c_int, [vp]),
        "sdrx_spectrum_configure": (C.c_int, [vp, vp]),
        "sdrx_spectrum_feed": (C.c_int, [vp, vp, i64, C.c_int]),
        "sdrx_spectrum_feed_dev": (C.c_int, [vp, vp, i64, C.c_int]),
        "sdrx_spectrum_available": (i64, [vp]),
        "sdrx_spectrum_read": (i64, [vp, vp, i64]),
        "sdrx_spectrum_skip": (i64, [vp, i64]),
        "sdrx_spectrum_window": (C.c_int, [vp, vp, i32]),
        "sdrx_wfm_create": (C.c_int, [pp, C.c_int, i32, vp]),
        "sdrx_wfm_destroy": (C.c_int, [vp]),
        "sdrx_wfm_reset": (C.c_int, [vp]),
        "sdrx_wfm_feed": (C.c_int, [vp, vp, vp]),
        "sdrx_wfm_feed_dev": (C.c_int, [vp, vp, vp]),
        "sdrx_wfm_feed_bank": (C.c_int, [vp, vp]),
        "sdrx_wfm_read": (i64, [vp, i32, vp, i64]),
        "sdrx_wfm_last_dev": (C.c_int, [vp, i32, pp, C.POINTER(i64)]),
        "sdrx_wfm_squelch_open": (C.c_int, [vp, i32]),
        "sdrx_wfm_levels": (C.c_int, [vp, i32, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(i64), C.c_int]),
        "sdrx_wfm_get_design": (C.c_int, [vp, i32, C.POINTER(i32), vp, i32, vp, C.POINTER(i32), C.POINTER(C.c_float)]),
        "sdrx_bfm_create": (C.c_int, [pp, C.c_int, i32, vp]),
        "sdrx_bfm_destroy": (C.c_int, [vp]),
        "sdrx_bfm_reset": (C.c_int, [vp]),
        "sdrx_bfm_feed": (C.c_int, [vp, vp, vp]),
        "sdrx_bfm_feed_dev": (C.c_int, [vp, vp, vp]),
        "sdrx_bfm_feed_bank": (C.c_int, [vp, vp]),
        "sdrx_bfm_read": (i64, [vp, i32, vp, i64]),
        "sdrx_bfm_last_dev": (C.c_int, [vp, i32, pp, C.POINTER(i64)]),
        "sdrx_bfm_read_sink": (i64, [vp, i32, vp, i64]),
        "sdrx_bfm_sink_last_dev": (C.c_int, [vp, i32, pp, C.POINTER(i64)]),
        "sdrx_bfm_pilot": (C.c_int, [vp, i32, C.POINTER(i32), C.POINTER(C.c_float), C.POINTER(u32), C.POINTER(u32)]),
        "sdrx_bfm_squelch_open": (C.c_int, [vp, i32]),
        "sdrx_bfm_levels": (C.c_int, [vp, i32, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(i64), C.c_int]),
        "sdrx_bfm_get_design": (C.c_int, [vp, i32, C.POINTER(i32), vp, i32, vp, C.POINTER(i32), C.POINTER(C.c_float), vp, C.POINTER(i32), vp]),
        "sdrx_bfmrds_create": (C.c_int, [pp, C.c_int, i32, vp, vp]),
        "sdrx_bfmrds_read_bits": (i64, [vp, i32, vp, i64]),
        "sdrx_bfmrds_bits_last_dev": (C.c_int, [vp, i32, pp, C.POINTER(i64)]),
        "sdrx_bfmrds_read_groups": (i64, [vp, i32, vp, i64]),
        "sdrx_bfmrds_groups_last_dev": (C.c_int, [vp, i32, pp, C.POINTER(i64)]),
        "sdrx_bfmrds_read_bb": (i64, [vp, i32, vp, i64]),
        "sdrx_bfmrds_report": (C.c_int, [vp, i32, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(i32)]),
        "sdrx_bfmrds_state": (C.c_int, [vp, i32, vp]),
        "sdrx_bfmrds_unsure": (i64, [vp, i32, C.c_int]),
        "sdrx_lora_create": (C.c_int, [pp, C.c_int, i32, vp]),
        "sdrx_lora_destroy": (C.c_int, [vp]),
        "sdrx_lora_reset": (C.c_int, [vp]),
        "sdrx_lora_feed": (C.c_int, [vp, vp, vp]),
        "sdrx_lora_feed_dev": (C.c_int, [vp, vp, vp]),
        "sdrx_lora_feed_bank": (C.c_int, [vp, vp]),
        "sdrx_lora_read": (i64, [vp, i32, vp, i64]),
        "sdrx_lora_last_dev": (C.c_int, [vp, i32, pp, C.POINTER(i64)]),
        "sdrx_lora_read_text": (i64, [vp, i32, vp, i64]),
        "sdrx_lora_state": (C.c_int, [vp, i32, vp]),
        "sdrx_lora_get_design": (C.c_int, [vp, i32, C.POINTER(i32), vp, i32, C.POINTER(i32), vp, C.POINTER(C.c_float), vp, vp]),
        "sdrx_am_create": (C.c_int, [pp, C.c_int, i32, vp]),
        "sdrx_am_destroy": (C.c_int, [vp]),
        "sdrx_am_reset": (C.c_int, [vp]),
        "sdrx_am_feed": (C.c_int, [vp, vp, vp]),
        "sdrx_am_feed_dev": (C.c_int, [vp, vp, vp]),
        "sdrx_am_feed_bank": (C.c_int, [vp, vp]),
        "sdrx_am_read": (i64, [vp, i32, vp, i64]),
        "sdrx_am_last_dev": (C.c_int, [vp, i32, pp, C.POINTER(i64)]),
        "sdrx_am_squelch_open": (C.c_int, [vp, i32]),
        "sdrx_am_levels": (C.c_int, [vp, i32, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(i64), C.c_int]),
        "sdrx_am_get_design": (C.c_int, [vp, i32, C.POINTER(i32), vp, i32, vp, C.POINTER(i32), C.POINTER(C.c_float)]),
        "sdrx_am_create_ex": (C.c_int, [pp, C.c_int, i32, vp, vp]),
        "sdrx_am_pll": (C.c_int, [vp, i32, C.POINTER(i32), C.POINTER(C.c_float)]),
        "sdrx_am_get_sync_design": (C.c_int, [vp, i32, vp, vp, C.POINTER(i32), vp]),
        "sdrx_nfm_create": (C.c_int, [pp, C.c_int, i32, vp]),
        "sdrx_nfm_create_ex": (C.c_int, [pp, C.c_int, i32, vp, vp]),
        "sdrx_nfm_ctcss": (C.c_int, [vp, i32, C.POINTER(i32), C.POINTER(C.c_float), C.POINTER(i64)]),
        "sdrx_nfm_ctcss_events": (i64, [vp, i32, vp, vp, i64]),
        "sdrx_nfm_ctcss_powers": (C.c_int, [vp, i32, vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i64)]),
        "sdrx_nfm_af_squelch": (C.c_int, [vp, i32, C.POINTER(i32), vp, C.POINTER(i32)]),
        "sdrx_nfm_get_tone_design": (C.c_int, [vp, i32, C.POINTER(i32), C.POINTER(i32), vp, vp, C.POINTER(i32), vp, vp, C.POINTER(C.c_double)]),
        "sdrx_nfm_destroy": (C.c_int, [vp]),
        "sdrx_nfm_reset": (C.c_int, [vp]),
        "sdrx_nfm_feed": (C.c_int, [vp, vp, vp]),
        "sdrx_nfm_feed_dev": (C.c_int, [vp, vp, vp]),
        "sdrx_nfm_feed_bank": (C.c_int, [vp, vp]),
        "sdrx_nfm_read": (i64, [vp, i32, vp, i64]),
        "sdrx_nfm_last_dev": (C.c_int, [vp, i32, pp, C.POINTER(i64)]),
        "sdrx_nfm_squelch_open": (C.c_int, [vp, i32]),
        "sdrx_nfm_levels": (C.c_int, [vp, i32, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(i64), C.c_int]),
        "sdrx_nfm_get_design": (C.c_int, [vp, i32, C.POINTER(i32), vp, i32, vp, C.POINTER(i32), C.POINTER(C.c_float), C.POINTER(i32)]),
        "sdrx_ssb_create": (C.c_int, [pp, C.c_int, i32, vp]),
        "sdrx_ssb_destroy": (C.c_int, [vp]),
        "sdrx_ssb_reset": (C.c_int, [vp]),
        "sdrx_ssb_feed": (C.c_int, [vp, vp, vp]),
        "sdrx_ssb_feed_dev": (C.c_int, [vp, vp, vp]),
        "sdrx_ssb_feed_bank": (C.c_int, [vp, vp]),
        "sdrx_ssb_read": (i64, [vp, i32, vp, i64]),
        "sdrx_ssb_last_dev": (C.c_int, [vp, i32, pp, C.POINTER(i64)]),
        "sdrx_ssb_read_spectrum": (i64, [vp, i32, vp, i64]),
        "sdrx_ssb_spectrum_last_dev": (C.c_int, [vp, i32, pp, C.POINTER(i64)]),
        "sdrx_ssb_audio_active": (C.c_int, [vp, i32]),
        "sdrx_ssb_levels": (C.c_int, [vp, i32, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(i64), C.c_int]),
        "sdrx_ssb_get_design": (C.c_int, [vp, i32, C.POINTER(i32), vp, i32, vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32),
                                          C.POINTER(C.c_double), C.POINTER(C.c_float)]),
        "sdrx_udpsrc_create": (C.c_int, [pp, C.c_int, i32, vp]),
        "sdrx_udpsrc_create_ex": (C.c_int, [pp, C.c_int, i32, vp, C.c_uint32]),
        "sdrx_chana_create": (C.c_int, [pp, C.c_int, i32, vp]),
        "sdrx_chana_destroy": (C.c_int, [vp]),
        "sdrx_chana_reset": (C.c_int, [vp]),
        "sdrx_chana_feed": (C.c_int, [vp, vp, vp]),
        "sdrx_chana_feed_dev": (C.c_int, [vp, vp, vp]),
        "sdrx_chana_feed_bank": (C.c_int, [vp, vp]),
        "sdrx_chana_read": (i64, [vp, i32, vp, i64]),
        "sdrx_chana_last_dev": (C.c_int, [vp, i32, pp, C.POINTER(i64)]),
        "sdrx_chana_positive_only": (C.c_int, [vp, i32]),
        "sdrx_chana_magsq": (C.c_int, [vp, i32, C.POINTER(C.c_double)]),
        "sdrx_chana_get_design": (C.c_int, [vp, i32, C.POINTER(i32), vp, i32, vp, C.POINTER(C.c_float)]),
        "sdrx_chana_seek": (C.c_int, [vp, i32, C.c_uint64]),
        "sdrx_chanapll_create": (C.c_int, [pp, C.c_int, i32, vp, vp]),
        "sdrx_chanapll_state": (C.c_int, [vp, i32, C.POINTER(i32), C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
        "sdrx_udpsrc_ssb_state": (C.c_int, [vp, i32, C.POINTER(i32), C.POINTER(i64), vp]),
        "sdrx_udpsrc_destroy": (C.c_int, [vp]),
        "sdrx_udpsrc_reset": (C.c_int, [vp]),
        "sdrx_udpsrc_feed": (C.c_int, [vp, vp, vp]),
        "sdrx_udpsrc_feed_dev": (C.c_int, [vp, vp, vp]),
        "sdrx_udpsrc_feed_bank": (C.c_int, [vp, vp]),
        "sdrx_udpsrc_sample_bytes": (i32, [vp, i32]),
        "sdrx_udpsrc_read": (i64, [vp, i32, vp, i64]),
        "sdrx_udpsrc_last_dev": (C.c_int, [vp, i32, pp, C.POINTER(i64)]),
        "sdrx_udpsrc_read_spectrum": (i64, [vp, i32, vp, i64]),
        "sdrx_udpsrc_spectrum_last_dev": (C.c_int, [vp, i32, pp, C.POINTER(i64)]),
        "sdrx_udpsrc_squelch_open": (C.c_int, [vp, i32]),
        "sdrx_udpsrc_squelch_counts": (C.c_int, [vp, i32, C.POINTER(i32), C.POINTER(i32)]),
        "sdrx_udpsrc_in_magsq": (C.c_int, [vp, i32, C.POINTER(C.c_double)]),
        "sdrx_udpsrc_total": (i64, [vp, i32]),
        "sdrx_udpsrc_get_design": (C.c_int, [vp, i32, C.POINTER(i32), vp, i32, vp, C.POINTER(i32), vp, C.POINTER(i32), C.POINTER(i32),
                                             C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_float), vp, C.POINTER(C.c_double)]),
        "sdrx_fdecim_state_bytes": (i64, [vp]),
        "sdrx_fdecim_get_state": (C.c_int, [vp, vp]),
        "sdrx_fdecim_set_state": (C.c_int, [vp, vp]),
        "sdrx_chan_bank_state_bytes": (i64, [vp]),
        "sdrx_chan_bank_get_state": (C.c_int, [vp, vp]),
        "sdrx_chan_bank_set_state": (C.c_int, [vp, vp]),
        "sdrx_fdecim_stages_create": (C.c_int, [pp, C.c_int]),
        "sdrx_fdecim_stages_destroy": (C.c_int, [vp]),
        "sdrx_fdecim_save_stages": (C.c_int, [vp, vp]),
        "sdrx_fdecim_load_stages": (C.c_int, [vp, vp]),
        "sdrx_decim24_process_dev": (C.c_int, [vp, vp, i64, vp, C.POINTER(i64)]),
        "sdrx_chan24_bank_feed_dev": (C.c_int, [vp, vp, i64]),
        "sdrx_chan24_bank_out_dev": (C.c_int, [vp, i32, C.POINTER(vp), C.POINTER(i64)]),
        "sdrx_chan24_bank_create": (C.c_int, [pp, C.c_int, i32, i32, vp, vp]),
        "sdrx_chan24_bank_destroy": (C.c_int, [vp]),
        "sdrx_chan24_bank_reset": (C.c_int, [vp]),
        "sdrx_chan24_bank_info": (C.c_int, [vp, i32, C.POINTER(i32), vp, C.POINTER(i32), C.POINTER(i32)]),
        "sdrx_chan24_bank_feed": (C.c_int, [vp, vp, i64]),
        "sdrx_chan24_bank_read": (i64, [vp, i32, vp, i64]),
        "sdrx_firbank_create": (C.c_int, [pp, C.c_int, i32, vp]),
        "sdrx_firbank_destroy": (C.c_int, [vp]),
        "sdrx_atv_create": (C.c_int, [pp, C.c_int, i32, vp]),
        "sdrx_atv_destroy": (C.c_int, [vp]),
        "sdrx_atv_reset": (C.c_int, [vp]),
        "sdrx_atv_feed": (C.c_int, [vp, vp, vp]),
        "sdrx_atv_feed_dev": (C.c_int, [vp, vp, vp]),
        "sdrx_atv_feed_bank": (C.c_int, [vp, vp]),
        "sdrx_atv_frames": (i64, [vp, i32, C.POINTER(i64)]),
        "sdrx_atv_read_events": (i64, [vp, i32, vp, i64]),
        "sdrx_atv_read_frame": (i64, [vp, i32, i64, vp, i64]),
        "sdrx_atv_read_screen": (i64, [vp, i32, vp, i64]),
        "sdrx_atv_frames_last_dev": (C.c_int, [vp, i32, pp, C.POINTER(i64), C.POINTER(i64)]),
        "sdrx_atv_screen_last_dev": (C.c_int, [vp, i32, pp, C.POINTER(i32), C.POINTER(i32)]),
        "sdrx_atv_read": (i64, [vp, i32, vp, i64]),
        "sdrx_atv_last_dev": (C.c_int, [vp, i32, pp, C.POINTER(i64)]),
        "sdrx_atv_state": (C.c_int, [vp, i32, vp]),
        "sdrx_atv_get_design": (C.c_int, [vp, i32, vp]),
        "sdrx_atv_get_filters": (C.c_int, [vp, i32, C.POINTER(i32), vp, i32, vp, vp]),
        "sdrx_datv_create": (C.c_int, [pp, C.c_int, i32, vp]),
        "sdrx_datv_destroy": (C.c_int, [vp]),
        "sdrx_datv_reset": (C.c_int, [vp]),
        "sdrx_datv_feed": (C.c_int, [vp, vp, vp]),
        "sdrx_datv_feed_dev": (C.c_int, [vp, vp, vp]),
        "sdrx_datv_feed_bank": (C.c_int, [vp, vp]),
        "sdrx_datv_read": (i64, [vp, i32, vp, vp, i64]),
        "sdrx_datv_read_points": (i64, [vp, i32, vp, i64]),
        "sdrx_datv_read_meas": (i64, [vp, i32, vp, i64]),
        "sdrx_datv_last_dev": (C.c_int, [vp, i32, pp, pp, C.POINTER(i64)]),
        "sdrx_datv_points_last_dev": (C.c_int, [vp, i32, pp, C.POINTER(i64)]),
        "sdrx_datv_meas_last_dev": (C.c_int, [vp, i32, pp, C.POINTER(i64)]),
        "sdrx_datv_state": (C.c_int, [vp, i32, vp]),
        "sdrx_datv_get_design": (C.c_int, [vp, i32, vp]),
        "sdrx_datv_get_tables": (C.c_int, [vp, i32, vp, i32, vp, vp, vp]),
        "sdrx_firbank_feed": (C.c_int, [vp, vp, vp, vp]),
        "sdrx_firbank_get_taps": (C.c_int, [vp, i32, vp, i32]),
        "sdrx_sdriq_parse_header": (C.c_int, [vp, C.c_uint64, vp]),
        "sdrx_sdriq_write_header": (C.c_int, [vp, vp]),
        "sdrx_fifo_create": (C.c_int, [pp, u32]),
        "sdrx_fifo_destroy": (C.c_int, [vp]),
        "sdrx_fifo_set_size": (C.c_int, [vp, u32]),
        "sdrx_fifo_size": (u32, [vp]),
        "sdrx_fifo_fill": (u32, [vp]),
        "sdrx_fifo_write_bytes": (u32, [vp, vp, u32]),
        "sdrx_fifo_write": (u32, [vp, vp, u32]),
        "sdrx_fifo_read": (u32, [vp, vp, u32]),
        "sdrx_fifo_read_begin": (u32, [vp, u32, pp, C.POINTER(u32), pp, C.POINTER(u32)]),
        "sdrx_fifo_read_commit": (u32, [vp, u32]),
        "sdrx_fifo_dropped": (C.c_uint64, [vp]),
    }
    # the stream / timing / launch-record accessors: one row per kind, stamped per handle family that exports it
    acc = {
        "sync": [vp],
        "set_stream": [vp, vp],
        "get_stream": [vp, pp],
        "set_timing": [vp, C.c_int],
        "get_timing": [vp, C.POINTER(C.c_double), C.POINTER(i64), C.c_int],
        "last_launch": [vp, C.c_char_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)],
    }
    five = ("sync", "set_stream", "set_timing", "get_timing", "last_launch")
    families = {"decim": five, "fdecim": five, "chan_bank": five + ("get_stream",), "spectrum": five + ("get_stream",),
                "wfm": five + ("get_stream",), "bfm": five + ("get_stream",), "am": five + ("get_stream",), "nfm": five + ("get_stream",),
                "ssb": five + ("get_stream",), "udpsrc": five + ("get_stream",), "chana": five + ("get_stream",), "lora": five + ("get_stream",), "atv": five + ("get_stream",), "datv": five + ("get_stream",), "dccorr": five[:2], "iqimb": five[:2],
                "backend": five[:1], "audiotail": five[:1], "decim24": five[:1], "chan24_bank": five[:1]}
    for prefix, names in families.items():
        for name in names:
            sig[f"sdrx_{prefix}_{name}"] = (C.c_int, acc[name])
    for name, (res, args) in sig.items():
        fn = getattr(L, name)          # AttributeError here == the header and the library disagree
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


#: every symbol include/sdrx.h declares (checked against the built library by tests/test_abi.py)
def exported_symbols(header_path: str | None = None) -> list[str]:
    import re
    header_path = header_path or os.path.join(os.path.dirname(_HERE), "include", "sdrx.h")
    txt = open(header_path).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(sdrx_[a-z0-9_]+)\s*\(", txt)) - {"sdrx_fifo_data_ready_cb"})


def _check(rc: int, what: str) -> None:
    if rc != 0:
        raise SdrxError(f"{what}: rc={rc}: {lib().sdrx_last_error().decode()}")


def _i16(a) -> np.ndarray:
    a = np.ascontiguousarray(a)
    if a.dtype != np.int16:
        raise TypeError("expected int16 I/Q")
    return a


class _Handle:
    """Owner of one C handle; `_prefix` names its entry points (sdrx_<prefix>_*)."""

    _prefix = ""

    def _fn(self, name: str):
        return getattr(lib(), f"sdrx_{self._prefix}_{name}")

    def _open(self, *args, create: str = "create"):
        self._h = C.c_void_p()
        _check(self._fn(create)(C.byref(self._h), *args), f"sdrx_{self._prefix}_{create}")

    def _call(self, name: str, *args, what: str | None = None):
        _check(self._fn(name)(self._h, *args), what or f"sdrx_{self._prefix}_{name}")

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._fn("destroy")(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:                               # quietly: at interpreter shutdown the module's globals may already be gone
            self.close()
        except Exception:
            pass


# The accessors every stream-owning handle family shares, written once; a class lists the mixins whose entry points its
# family exports (lib() binds the same rows per prefix).
class _Sync:
    def sync(self):
        self._call("sync")


class _SetStream:
    def set_stream(self, hip_stream: int | None):
        self._call("set_stream", hip_stream)


class _GetStream:
    def get_stream(self) -> int:
        p = C.c_void_p()
        self._call("get_stream", C.byref(p))
        return p.value or 0


class _Timed:
    def set_timing(self, on: bool):
        self._call("set_timing", int(on))

    def get_timing(self, reset: bool = True):
        """(total kernel ms, launches) measured with HIP events on the launch stream"""
        ms, n = C.c_double(), C.c_int64()
        self._call("get_timing", C.byref(ms), C.byref(n), int(reset))
        return ms.value, n.value

    def last_launch(self) -> dict:
        name = C.create_string_buffer(128)
        g, b, l = C.c_int(), C.c_int(), C.c_int()
        self._call("last_launch", name, 128, C.byref(g), C.byref(b), C.byref(l), what="last_launch")
        return {"kernel": name.value.decode(), "grid": g.value, "block": b.value, "lds_bytes": l.value}


class Decimators(_Handle, _Sync, _SetStream, _Timed):
    """Decimators<qint32, qint16, 16, input_bits> used with one (log2, fcpos)
    (sdrbase/dsp/decimators.h:279-341).  `decimate(buf)` == decimateK_{inf,sup,cen}(&it, buf, len)."""
    _prefix = "decim"

    def __init__(self, log2_decim: int, fcpos: int = FC_CEN, input_bits: int = 12, device: int = 0):
        self._open(device, log2_decim, fcpos, input_bits)
        self.log2, self.fcpos, self.input_bits = log2_decim, fcpos, input_bits

    def reset(self):
        self._call("reset")

    def decimate(self, buf) -> np.ndarray:
        """buf: int16 interleaved I,Q (len = reference `len`).  Returns int16 array of 2*n_out."""
        buf = _i16(buf)
        out = np.empty(max(2 * ((buf.size // 2) >> self.log2), 2), np.int16)
        n = C.c_int32()
        self._call("process", buf.ctypes.data, buf.size, out.ctypes.data, C.byref(n))
        return out[: 2 * n.value]

    def decimate_dev(self, d_in_ptr: int, n_int16: int, d_out_ptr: int) -> int:
        """device pointers; asynchronous on the handle's stream; returns #complex outputs"""
        n = C.c_int64()
        self._call("process_dev", d_in_ptr, n_int16, d_out_ptr, C.byref(n))
        return n.value

    def save_stages(self, stages: "DecimStages"):
        """stages 1..log2 of `stages` := what this variant's filters hold now"""
        self._call("save_stages", stages._h)

    def load_stages(self, stages: "DecimStages"):
        """continue from the shared filter set of one reference Decimators object (decimators.h:326-333)"""
        self._call("load_stages", stages._h)

    # ---- pinned double-buffered host path: the receive buffer IS a slot of the handle's pinned ring
    def ring_create(self, slot_elems: int, n_slots: int, flush_slots: int = 1):
        self._call("ring_create", slot_elems, n_slots, flush_slots)
        self._slot_elems = slot_elems

    def ring_acquire(self) -> np.ndarray:
        """numpy view of the next free pinned input slot (int16, or uint8 for DecimatorsU)"""
        p = lib().sdrx_decim_ring_acquire(self._h)
        if not p:
            raise SdrxError(f"sdrx_decim_ring_acquire: {lib().sdrx_last_error().decode()}")
        ct = C.c_uint8 if self.input_bits == 8 and isinstance(self, DecimatorsU) else C.c_int16
        return np.ctypeslib.as_array((ct * self._slot_elems).from_address(p))

    def ring_submit(self, n_elems: int):
        self._call("ring_submit", n_elems)

    def ring_retire(self) -> np.ndarray:
        """outputs of the oldest submitted block (a view of the pinned output slot: copy it before that slot is reused)"""
        out, n = C.c_void_p(), C.c_int32()
        self._call("ring_retire", C.byref(out), C.byref(n))
        if n.value == 0:
            return np.empty(0, np.int16)
        return np.ctypeslib.as_array((C.c_int16 * (2 * n.value)).from_address(out.value))

    def get_state(self) -> bytes:
        nb = lib().sdrx_decim_state_bytes(self._h)
        buf = C.create_string_buffer(nb)
        self._call("get_state", buf)
        return buf.raw

    def set_state(self, state: bytes):
        if len(state) != lib().sdrx_decim_state_bytes(self._h):
            raise ValueError("state size")
        self._call("set_state", state)

    def last_fallback(self) -> dict:
        """chunks (4096 input samples) of the most recent call that the FAST kernel flagged for the EXACT recompute;
        total = 0 when that call ran no FAST launch.  Synchronises the handle's stream."""
        f, t = C.c_int64(), C.c_int64()
        _check(lib().sdrx_decim_last_fallback(self._h, C.byref(f), C.byref(t), None, 0), "last_fallback")
        flags = np.zeros(t.value, np.uint8)
        if t.value:
            _check(lib().sdrx_decim_last_fallback(self._h, C.byref(f), C.byref(t), flags.ctypes.data, flags.size), "last_fallback")
        return {"flagged": f.value, "total": t.value, "flags": flags}


def decimate_dev_batch(handles, d_in_ptrs, n_elems, d_out_ptrs) -> list:
    """sdrx_decim_process_dev_batch: many device streams (one Decimators / DecimatorsU object each, same configuration),
    one launch.  Device pointers; asynchronous on handles[0]'s stream; returns #complex outputs per stream."""
    n = len(handles)
    if not (n == len(d_in_ptrs) == len(n_elems) == len(d_out_ptrs)):
        raise ValueError("one pointer / count per handle")
    hs = (C.c_void_p * n)(*[h._h.value for h in handles])
    ins = (C.c_void_p * n)(*d_in_ptrs)
    outs = (C.c_void_p * n)(*d_out_ptrs)
    ns = (C.c_int64 * n)(*n_elems)
    no = (C.c_int64 * n)()
    _check(lib().sdrx_decim_process_dev_batch(hs, n, ins, ns, outs, no), "sdrx_decim_process_dev_batch")
    return list(no)


class DecimStages(_Handle):
    """The six IntHalfbandFilterEO states that all decimateK_x of ONE reference Decimators object share."""
    _prefix = "decim_stages"

    def __init__(self, device: int = 0):
        self._open(device)


class DecimatorsObject:
    """One reference Decimators / DecimatorsU object: any decimateK_x per call, all on the same six stage states
    (what include/sdrx/dsp.hpp's sdrx::Decimators does in C++)."""

    def __init__(self, input_bits: int = 12, device: int = 0, u8_shift=None):
        self.bits, self.device, self.u8_shift = input_bits, device, u8_shift
        self._variants, self._stages, self._last = {}, DecimStages(device), None

    def decimate(self, log2: int, fcpos: int, buf) -> np.ndarray:
        d = self._variants.get((log2, fcpos))
        if d is None:
            d = DecimatorsU(log2, fcpos, self.u8_shift, self.device) if self.u8_shift is not None else Decimators(log2, fcpos, self.bits, self.device)
            self._variants[(log2, fcpos)] = d
        if log2 > 0 and d is not self._last:
            if self._last is not None:
                self._last.save_stages(self._stages)
            d.load_stages(self._stages)
            self._last = d
        return d.decimate(buf)

    def close(self):
        for d in self._variants.values():
            d.close()
        self._variants = {}
        self._stages.close()


class DecimatorsU(Decimators):
    """DecimatorsU<qint32, quint8, 16, 8, shift> (sdrbase/dsp/decimatorsu.h): unsigned 8-bit I/Q (RTL-SDR)."""

    def __init__(self, log2_decim: int, fcpos: int = FC_CEN, shift: int = 127, device: int = 0):
        self._open(device, log2_decim, fcpos, shift, create="create_u8")
        self.log2, self.fcpos, self.input_bits = log2_decim, fcpos, 8

    def decimate(self, buf) -> np.ndarray:
        buf = np.ascontiguousarray(buf)
        if buf.dtype != np.uint8:
            raise TypeError("expected uint8 I/Q")
        out = np.empty(max(2 * ((buf.size // 2) >> self.log2), 2), np.int16)
        n = C.c_int32()
        _check(lib().sdrx_decim_process_u8(self._h, buf.ctypes.data, buf.size, out.ctypes.data, C.byref(n)), "sdrx_decim_process_u8")
        return out[: 2 * n.value]

    def decimate_dev(self, d_in_ptr: int, n_uint8: int, d_out_ptr: int) -> int:
        """device pointers (d_in 8-byte aligned); asynchronous on the handle's stream; returns #complex outputs"""
        n = C.c_int64()
        _check(lib().sdrx_decim_process_dev_u8(self._h, d_in_ptr, n_uint8, d_out_ptr, C.byref(n)), "sdrx_decim_process_dev_u8")
        return n.value


class Fanout(_Handle):
    """One staged source stream copied to several GPUs point-to-point (sdrx_fanout_*; xGMI peer copies on a multi-GPU node)."""
    _prefix = "fanout"

    def __init__(self, src_device: int, dst_devices, max_bytes: int):
        d = np.ascontiguousarray(dst_devices, dtype=np.int32)
        self.n = d.size
        self._open(src_device, self.n, d.ctypes.data, max_bytes)

    def send(self, d_src: int, n_bytes: int, producer_stream: int | None = None):
        self._call("send", d_src, n_bytes, producer_stream)

    def buffer(self, i: int) -> int:
        return lib().sdrx_fanout_buffer(self._h, i) or 0

    def wait(self, i: int):
        self._call("wait", i)


class FloatDecimStages(_Handle):
    """The six IntHalfbandFilterEOF states that all decimateK_x of ONE DecimatorsFI / FF / IF object share."""
    _prefix = "fdecim_stages"

    def __init__(self, device: int = 0):
        self._open(device)


class FloatDecimatorsObject:
    """One reference DecimatorsFI ("fi") / FF ("ff") / IF ("if") object: any decimateK_x per call on the same six filters
    (what include/sdrx/dsp.hpp's sdrx::DecimatorsFI etc. do in C++)."""

    def __init__(self, kind: str, input_bits: int = 16, device: int = 0):
        self.kind, self.bits, self.device = kind, input_bits, device
        self._variants, self._stages, self._last = {}, FloatDecimStages(device), None

    def decimate(self, log2: int, fcpos: int, buf) -> np.ndarray:
        d = self._variants.get((log2, fcpos))
        if d is None:
            d = FloatDecimators(self.kind, log2, fcpos, self.bits, self.device)
            self._variants[(log2, fcpos)] = d
        if d is not self._last:
            if self._last is not None:
                _check(lib().sdrx_fdecim_save_stages(self._last._h, self._stages._h), "sdrx_fdecim_save_stages")
            _check(lib().sdrx_fdecim_load_stages(d._h, self._stages._h), "sdrx_fdecim_load_stages")
            self._last = d
        return d.decimate(buf)

    def close(self):
        for d in self._variants.values():
            d.close()
        self._variants = {}
        self._stages.close()


class FloatDecimators(_Handle, _Sync, _SetStream, _Timed):
    """The float half-band decimators over IntHalfbandFilterEOF<64>, one (log2, fcpos) per object:
    kind "fi" = DecimatorsFI (float I/Q -> int16 Sample; AirspyHF), "ff" = DecimatorsFF (float -> float),
    "if" = DecimatorsIF<qint16, input_bits> (int16 -> float).  `decimate(buf)` == decimateK_{inf,sup,cen}(&it, buf, nbIAndQ)."""
    _prefix = "fdecim"

    KINDS = {"fi": (0, 0), "ff": (0, 1), "if": (1, 1)}

    def __init__(self, kind: str, log2_decim: int, fcpos: int = FC_CEN, input_bits: int = 16, device: int = 0):
        self.in_kind, self.out_kind = self.KINDS[kind]
        self._open(device, log2_decim, fcpos, self.in_kind, self.out_kind, input_bits)
        self.kind, self.log2, self.fcpos = kind, log2_decim, fcpos

    def reset(self):
        self._call("reset")

    def decimate(self, buf) -> np.ndarray:
        buf = np.ascontiguousarray(buf, dtype=np.float32 if self.in_kind == 0 else np.int16)
        out = np.empty(buf.size + 8, np.int16 if self.out_kind == 0 else np.float32)
        n = C.c_int32()
        self._call("process", buf.ctypes.data, buf.size, out.ctypes.data, C.byref(n))
        return out[: 2 * n.value]

    def decimate_dev(self, d_in_ptr: int, n_elems: int, d_out_ptr: int) -> int:
        n = C.c_int64()
        self._call("process_dev", d_in_ptr, n_elems, d_out_ptr, C.byref(n))
        return n.value


class DcCorrection(_Handle, _Sync, _SetStream):
    """DSPDeviceSourceEngine::iqCorrections(begin, end, false): the DC offset correction of the device stream"""
    _prefix = "dccorr"

    def __init__(self, device: int = 0):
        self._open(device)

    def reset(self):
        self._call("reset")

    def process(self, iq) -> np.ndarray:
        """returns the corrected copy of an int16 I/Q span (the C call works in place)"""
        buf = np.array(iq, dtype=np.int16, copy=True)
        self._call("process", buf.ctypes.data, buf.size // 2)
        return buf

    def process_dev(self, d_in_ptr: int, d_out_ptr: int, n_cplx: int):
        self._call("process_dev", d_in_ptr, d_out_ptr, n_cplx)


# FFTWindow::Function and SpectrumVis::AveragingMode (include/sdrx.h SDRX_SPECTRUM_*)
WIN_BARTLETT, WIN_BLACKMAN_HARRIS, WIN_FLATTOP, WIN_HAMMING, WIN_HANNING, WIN_RECTANGLE = range(6)
AVG_NONE, AVG_MOVING, AVG_FIXED = 0, 1, 2


class SpectrumCfg(C.Structure):
    _fields_ = [("fft_size", C.c_int32), ("overlap_percent", C.c_int32), ("avg_nb", C.c_uint32), ("avg_mode", C.c_int32),
                ("window", C.c_int32), ("linear", C.c_int32), ("scalef", C.c_float)]


class SpectrumVis(_Handle, _Sync, _SetStream, _GetStream, _Timed):
    """SpectrumVis (sdrgui/dsp/spectrumvis.{h,cpp}) on the GPU: every frame the reference hands to
    GLSpectrum::newSpectrum is queued on the device until read() -> (frames, N) float32."""
    _prefix = "spectrum"

    def __init__(self, fft_size: int = 1024, overlap_percent: int = 0, avg_nb: int = 0, avg_mode: int = AVG_NONE,
                 window: int = WIN_BLACKMAN_HARRIS, linear: bool = False, scalef: float = 32768.0, device: int = 0):
        cfg = self._cfg(fft_size, overlap_percent, avg_nb, avg_mode, window, linear, scalef)
        self._open(device, C.byref(cfg))
        self.scalef = scalef

    @staticmethod
    def _cfg(fft_size, overlap_percent, avg_nb, avg_mode, window, linear, scalef) -> SpectrumCfg:
        return SpectrumCfg(int(fft_size), int(overlap_percent), int(avg_nb), int(avg_mode), int(window), int(bool(linear)), float(scalef))

    @property
    def fft_size(self) -> int:
        return lib().sdrx_spectrum_window(self._h, None, 0)

    def configure(self, fft_size: int, overlap_percent: int, avg_nb: int, avg_mode: int, window: int, linear: bool):
        """handleConfigure: keeps the 4096-entry buffer, zeroes the averages"""
        cfg = self._cfg(fft_size, overlap_percent, avg_nb, avg_mode, window, linear, self.scalef)
        self._call("configure", C.byref(cfg))

    def reset(self):
        self._call("reset")

    def feed(self, iq, positive_only: bool = False):
        iq = _i16(iq)
        self._call("feed", iq.ctypes.data, iq.size // 2, int(positive_only))

    def feed_dev(self, t, positive_only: bool = False):
        """t: a contiguous int16 torch tensor of interleaved I/Q on the handle's device, ordered against the handle's
        stream by the caller (synchronise, or hand the torch stream over with set_stream)"""
        if not t.is_contiguous() or str(t.dtype) != "torch.int16":
            raise TypeError("expected a contiguous int16 tensor")
        self._call("feed_dev", t.data_ptr(), t.numel() // 2, int(positive_only))

    def available(self) -> int:
        return lib().sdrx_spectrum_available(self._h)

    def read(self, max_frames: int | None = None) -> np.ndarray:
        n = self.fft_size
        k = self.available() if max_frames is None else min(max_frames, self.available())
        out = np.empty((k, n), np.float32)
        got = lib().sdrx_spectrum_read(self._h, out.ctypes.data, k)
        if got < 0:
            raise SdrxError(f"sdrx_spectrum_read rc={got}: {lib().sdrx_last_error().decode()}")
        return out[:got]

    def skip(self, n: int = -1) -> int:
        return lib().sdrx_spectrum_skip(self._h, n)

    def window(self) -> np.ndarray:
        n = self.fft_size
        out = np.empty(n, np.float32)
        lib().sdrx_spectrum_window(self._h, out.ctypes.data, n)
        return out


def chan_plan(in_rate: int, req_rate: int, req_fc: int):
    """DownChannelizer::applyConfiguration's float bisection -> (modes, out_rate, residual_ofs)."""
    modes = np.zeros(32, np.uint8)
    r, f = C.c_int32(), C.c_int32()
    n = lib().sdrx_chan_plan(in_rate, req_rate, req_fc, modes.ctypes.data, C.byref(r), C.byref(f))
    if n < 0:
        raise SdrxError(f"sdrx_chan_plan rc={n}")
    return modes[:n].copy(), r.value, f.value


class ChannelizerBank(_Handle, _Sync, _SetStream, _Timed):
    """N x DownChannelizer fed from one device stream (sdrbase/dsp/downchannelizer.{h,cpp})."""
    _prefix = "chan_bank"

    def __init__(self, in_rate: int, req_rates, req_fcs, device: int = 0):
        rr = np.ascontiguousarray(req_rates, dtype=np.int32)
        fc = np.ascontiguousarray(req_fcs, dtype=np.int32)
        assert rr.size == fc.size
        self.n_ch = int(rr.size)
        self._open(device, in_rate, self.n_ch, rr.ctypes.data, fc.ctypes.data)

    def info(self, ch: int):
        n, r, f = C.c_int32(), C.c_int32(), C.c_int32()
        modes = np.zeros(32, np.uint8)
        self._call("info", ch, C.byref(n), modes.ctypes.data, C.byref(r), C.byref(f))
        return modes[: n.value].copy(), r.value, f.value

    def add_channel(self, req_rate: int, req_fc: int) -> int:
        c = C.c_int32(-1)
        self._call("add_channel", req_rate, req_fc, C.byref(c))
        self.n_ch = max(getattr(self, "n_ch", 0), c.value + 1)
        return c.value

    def remove_channel(self, ch: int):
        self._call("remove_channel", ch)

    @property
    def group_count(self) -> int:
        return lib().sdrx_chan_bank_group_count(self._h)

    def reconfigure(self, ch: int, req_rate: int, req_fc: int):
        self._call("reconfigure", ch, req_rate, req_fc)

    def reset(self):
        self._call("reset")

    def feed(self, iq):
        iq = _i16(iq)
        self._call("feed", iq.ctypes.data, iq.size // 2)

    def feed_dev(self, d_ptr: int, n_cplx: int):
        self._call("feed_dev", d_ptr, n_cplx)

    def available(self, ch: int) -> int:
        return lib().sdrx_chan_bank_available(self._h, ch)

    def read(self, ch: int, cap: int | None = None) -> np.ndarray:
        cap = self.available(ch) if cap is None else cap
        out = np.empty(max(2 * cap, 2), np.int16)
        n = lib().sdrx_chan_bank_read(self._h, ch, out.ctypes.data, cap)
        if n < 0:
            raise SdrxError(f"sdrx_chan_bank_read rc={n}: {lib().sdrx_last_error().decode()}")
        return out[: 2 * n]

    def last_dev(self, ch: int):
        """(device pointer, n_cplx) of what the last feed produced for channel ch"""
        p, n = C.c_void_p(), C.c_int64()
        self._call("last_dev", ch, C.byref(p), C.byref(n))
        return p.value or 0, n.value

    def skip(self, ch: int, n: int = -1) -> int:
        return lib().sdrx_chan_bank_skip(self._h, ch, n)


class FirCfg(C.Structure):
    """sdrx_fir_cfg"""
    _fields_ = [("kind", C.c_int32), ("ntaps", C.c_int32), ("sample_rate", C.c_float), ("f1", C.c_float), ("f2", C.c_float)]


class FirBank(_Handle):
    """Lowpass<Real> / Bandpass<Real> (sdrbase/dsp/lowpass.h, bandpass.h) for N channels."""
    _prefix = "firbank"

    def __init__(self, cfgs, device: int = 0):
        self.n_ch = len(cfgs)
        arr = (FirCfg * self.n_ch)(*cfgs)
        self._open(device, self.n_ch, arr)

    def taps(self, ch: int) -> np.ndarray:
        t = np.zeros(4096, np.float32)
        n = lib().sdrx_firbank_get_taps(self._h, ch, t.ctypes.data, t.size)
        return t[:n].copy()

    def feed(self, per_channel):
        ins = [np.ascontiguousarray(x, dtype=np.float32) for x in per_channel]
        outs = [np.empty(max(x.size, 1), np.float32) for x in ins]
        pi = (C.c_void_p * self.n_ch)(*[x.ctypes.data for x in ins])
        po = (C.c_void_p * self.n_ch)(*[x.ctypes.data for x in outs])
        ns = (C.c_int64 * self.n_ch)(*[x.size for x in ins])
        self._call("feed", pi, ns, po)
        return [o[: x.size] for o, x in zip(outs, ins)]


class SdriqHeader(C.Structure):
    """sdrx_sdriq_header (FileRecord::Header, sdrbase/dsp/filerecord.h:17-23)"""
    _fields_ = [("sample_rate", C.c_int32), ("center_frequency", C.c_uint64), ("start_timestamp", C.c_int64), ("sample_size", C.c_uint32)]


def sdriq_parse(data: bytes):
    """-> (SdriqHeader, int16 I/Q array of the samples that follow the 24-byte header)"""
    h = SdriqHeader()
    _check(lib().sdrx_sdriq_parse_header(data, len(data), C.byref(h)), "sdrx_sdriq_parse_header")
    body = np.frombuffer(data, dtype=np.int16, offset=24, count=(len(data) - 24) // 4 * 2) if h.sample_size == 16 else None
    return h, body


def sdriq_header_bytes(sample_rate: int, center_frequency: int, timestamp: int = 0, sample_size: int = 16) -> bytes:
    h = SdriqHeader(sample_rate, center_frequency, timestamp, sample_size)
    buf = C.create_string_buffer(24)
    _check(lib().sdrx_sdriq_write_header(buf, C.byref(h)), "sdrx_sdriq_write_header")
    return buf.raw


class BackendCfg(C.Structure):
    """sdrx_backend_cfg"""
    _fields_ = [("in_rate", C.c_int32), ("nco_freq", C.c_int32), ("out_rate", C.c_int32),
                ("interp_cutoff", C.c_float), ("taps_per_phase", C.c_float), ("filt_mode", C.c_int32),
                ("f1", C.c_float), ("f2", C.c_float), ("discri", C.c_int32), ("fm_scaling", C.c_float)]


class BackendBank(_Handle, _Sync):
    """NCO -> Interpolator -> fftfilt -> discriminator for N channels (front of the channelrx demods)."""
    _prefix = "backend"

    def __init__(self, cfgs, device: int = 0):
        self.n_ch = len(cfgs)
        arr = (BackendCfg * self.n_ch)(*cfgs)
        self._open(device, self.n_ch, arr)
        self.cfgs = list(cfgs)

    def feed(self, per_channel_iq):
        bufs = [_i16(x) for x in per_channel_iq]
        ptrs = (C.c_void_p * self.n_ch)(*[b.ctypes.data for b in bufs])
        ns = (C.c_int64 * self.n_ch)(*[b.size // 2 for b in bufs])
        self._call("feed", ptrs, ns)

    def feed_bank(self, bank: "ChannelizerBank"):
        """channel c takes what the bank's last feed produced for its channel c; ordered on the device, no host sync"""
        self._call("feed_bank", bank._h)

    def feed_dev(self, ptrs, counts):
        p = (C.c_void_p * self.n_ch)(*ptrs)
        n = (C.c_int64 * self.n_ch)(*counts)
        self._call("feed_dev", p, n)

    def read(self, ch: int, cap_floats: int = 1 << 24) -> np.ndarray:
        out = np.empty(cap_floats, np.float32)
        n = lib().sdrx_backend_read(self._h, ch, out.ctypes.data, cap_floats)
        if n < 0:
            raise SdrxError(f"sdrx_backend_read rc={n}: {lib().sdrx_last_error().decode()}")
        return out[:n].copy()

    def last_dev(self, ch: int):
        """(device pointer, number of floats) of the last feed's output of channel ch"""
        p, n = C.c_void_p(), C.c_int64()
        self._call("last_dev", ch, C.byref(p), C.byref(n))
        return p.value or 0, n.value

    def design(self, ch: int):
        nt, inc = C.c_int32(), C.c_int32()
        taps = np.zeros(16 * 256, np.float32)
        filt = np.zeros(4096, np.float32)
        self._call("get_design", ch, C.byref(nt), taps.ctypes.data, taps.size, filt.ctypes.data, C.byref(inc))
        return nt.value, taps[: 16 * nt.value].copy(), filt, inc.value


class WfmCfg(C.Structure):
    """sdrx_wfm_cfg: one WFMDemod (in_rate, nco_freq = -frequencyOffset, audio_rate, WFMDemodSettings)"""
    _fields_ = [("in_rate", C.c_int32), ("nco_freq", C.c_int32), ("audio_rate", C.c_int32),
                ("rf_bandwidth", C.c_float), ("af_bandwidth", C.c_float), ("volume", C.c_float), ("squelch_db", C.c_float),
                ("audio_mute", C.c_int32)]


class BfmCfg(C.Structure):
    """sdrx_bfm_cfg: one BFMDemod (in_rate, nco_freq = -frequencyOffset, audio_rate, BFMDemodSettings without RDS)"""
    _fields_ = [("in_rate", C.c_int32), ("nco_freq", C.c_int32), ("audio_rate", C.c_int32),
                ("rf_bandwidth", C.c_float), ("af_bandwidth", C.c_float), ("volume", C.c_float), ("squelch_db", C.c_float),
                ("audio_stereo", C.c_int32), ("lsb_stereo", C.c_int32), ("show_pilot", C.c_int32)]


class BfmRdsCfg(C.Structure):
    """sdrx_bfmrds_cfg: m_rdsActive of one BFMDemod"""
    _fields_ = [("rds_active", C.c_int32)]


class BfmRdsState(C.Structure):
    """sdrx_bfmrds_state_t: RDSDemod's and RDSDecoder's carried state, floats and doubles as their bits"""
    _fields_ = [("subcarr_phi", C.c_uint64), ("clock_offset", C.c_uint64), ("clock_phi", C.c_uint64), ("prev_clock_phi", C.c_uint64),
                ("d_cphi", C.c_uint64), ("xv", C.c_uint32 * 3), ("yv", C.c_uint32 * 3), ("prev_bb", C.c_uint32), ("acc", C.c_uint32),
                ("prev_acc", C.c_uint32), ("lo_clock", C.c_uint32), ("prev_lo_clock", C.c_uint32), ("numsamples", C.c_int32),
                ("counter", C.c_int32), ("reading_frame", C.c_int32), ("tot_errs", C.c_int32 * 2), ("dbit", C.c_int32),
                ("distance_remain", C.c_uint32), ("mix_phase", C.c_uint32), ("n_rds", C.c_int32), ("reg", C.c_uint64),
                ("lastseen_offset_counter", C.c_uint64), ("bit_counter", C.c_uint64), ("block_bit_counter", C.c_uint32),
                ("wrong_blocks_counter", C.c_uint32), ("blocks_counter", C.c_uint32), ("group_good_blocks_counter", C.c_uint32),
                ("group", C.c_uint32 * 4), ("sync", C.c_int32), ("presync", C.c_int32), ("lastseen_offset", C.c_int32),
                ("block_number", C.c_int32), ("group_assembly_started", C.c_int32), ("good_block", C.c_int32),
                ("decoder_qua", C.c_uint32), ("reserved", C.c_int32)]


class LoraCfg(C.Structure):
    """sdrx_lora_cfg: one LoRaDemod (in_rate, nco_freq = -frequencyOffset, bandwidth = m_Bandwidth)"""
    _fields_ = [("in_rate", C.c_int32), ("nco_freq", C.c_int32), ("bandwidth", C.c_int32)]


class LoraState(C.Structure):
    """sdrx_lora_state_t: m_tune, m_time, m_result, m_bin, the 64-bit m_count and the lines printed so far"""
    _fields_ = [("tune", C.c_int32), ("time", C.c_int32), ("result", C.c_int32), ("bin", C.c_int32), ("count", C.c_int64), ("lines", C.c_int64)]


class AmCfg(C.Structure):
    """sdrx_am_cfg: one AMDemod in envelope mode (in_rate, nco_freq = -frequencyOffset, audio_rate, AMDemodSettings)"""
    _fields_ = [("in_rate", C.c_int32), ("nco_freq", C.c_int32), ("audio_rate", C.c_int32),
                ("rf_bandwidth", C.c_float), ("volume", C.c_float), ("squelch_db", C.c_float),
                ("audio_mute", C.c_int32), ("bandpass_enable", C.c_int32)]


class AmSyncCfg(C.Structure):
    """sdrx_am_sync_cfg: the synchronous-AM options of one AMDemod (pll = m_pll; sync_op 0 DSB, 1 USB, 2 LSB; ssb_design_rate and
    ssb_design_bw: the audio rate and RF bandwidth SSBFilter was designed from, 0 = 48000 and 5000)"""
    _fields_ = [("pll", C.c_int32), ("sync_op", C.c_int32), ("ssb_design_rate", C.c_int32), ("ssb_design_bw", C.c_float)]


class NfmCfg(C.Structure):
    """sdrx_nfm_cfg: one NFMDemod, power squelch (in_rate, nco_freq = -frequencyOffset, audio_rate, NFMDemodSettings)"""
    _fields_ = [("in_rate", C.c_int32), ("nco_freq", C.c_int32), ("audio_rate", C.c_int32),
                ("rf_bandwidth", C.c_float), ("af_bandwidth", C.c_float), ("fm_deviation", C.c_int32), ("volume", C.c_float),
                ("squelch", C.c_float), ("squelch_gate", C.c_int32), ("audio_mute", C.c_int32)]


class NfmToneCfg(C.Structure):
    """sdrx_nfm_tone_cfg: the tone options of one NFMDemod (delta_squelch 1 = AF squelch, NfmCfg.squelch is then "negative millis";
    ctcss_index 0 = any tone, 1..32 = that EIA tone)"""
    _fields_ = [("delta_squelch", C.c_int32), ("ctcss_on", C.c_int32), ("ctcss_index", C.c_int32), ("reserved", C.c_int32)]


#: the 32 EIA tones of CTCSSDetector, index 1..32 of NfmToneCfg.ctcss_index
CTCSS_TONES = (67.0, 71.9, 74.4, 77.0, 79.7, 82.5, 85.4, 88.5, 91.5, 94.8, 97.4, 100.0, 103.5, 107.2, 110.9, 114.8, 118.8, 123.0, 127.3, 131.8,
               136.5, 141.3, 146.2, 151.4, 156.7, 162.2, 167.9, 173.8, 179.9, 186.2, 192.8, 203.5)


class SsbCfg(C.Structure):
    """sdrx_ssb_cfg: one SSBDemod (in_rate, nco_freq = -frequencyOffset, audio_rate, SSBDemodSettings; rf_bandwidth < 0 is LSB)"""
    _fields_ = [("in_rate", C.c_int32), ("nco_freq", C.c_int32), ("audio_rate", C.c_int32),
                ("rf_bandwidth", C.c_float), ("low_cutoff", C.c_float), ("volume", C.c_float), ("span_log2", C.c_int32),
                ("audio_binaural", C.c_int32), ("audio_flip", C.c_int32), ("dsb", C.c_int32), ("audio_mute", C.c_int32),
                ("agc", C.c_int32), ("agc_clamping", C.c_int32), ("agc_time_log2", C.c_int32), ("agc_power_threshold", C.c_int32),
                ("agc_threshold_gate", C.c_int32)]


class ChanaCfg(C.Structure):
    """sdrx_chana_cfg: one ChannelAnalyzer (in_rate, nco_freq = -frequencyOffset, ChannelAnalyzerSettings; bandwidth < 0 is the
    lower side; input_type 0 signal, 2 autocorrelation)"""
    _fields_ = [("in_rate", C.c_int32), ("nco_freq", C.c_int32), ("down_sample", C.c_int32), ("down_sample_rate", C.c_int32),
                ("bandwidth", C.c_int32), ("low_cutoff", C.c_int32), ("span_log2", C.c_int32), ("ssb", C.c_int32), ("rrc", C.c_int32),
                ("rrc_rolloff", C.c_int32), ("input_type", C.c_int32), ("pll", C.c_int32), ("fll", C.c_int32)]


def wfm_required_bw(rf_bw: int) -> int:
    """WFMDemod::requiredBW: the rate the demodulator asks its channelizer for"""
    return 48000 if rf_bw <= 48000 else (3 * rf_bw) // 2


class _DemodBank(_Handle, _Sync, _SetStream, _GetStream, _Timed):
    """N demodulators of one kind: int16 I/Q at the channelizer's output rate in, mono qint16 audio out.  A subclass
    names its entry points (`_prefix`) and its cfg struct (`_cfg`) and adds what differs per kind: levels() and design()."""

    _cfg = None

    def __init__(self, cfgs, device: int = 0):
        self.n_ch = len(cfgs)
        arr = (self._cfg * self.n_ch)(*cfgs)
        self._open(device, self.n_ch, arr)
        self.cfgs = list(cfgs)

    def reset(self):
        self._call("reset")

    def feed(self, per_channel_iq):
        bufs = [_i16(x) for x in per_channel_iq]
        ptrs = (C.c_void_p * self.n_ch)(*[b.ctypes.data for b in bufs])
        ns = (C.c_int64 * self.n_ch)(*[b.size // 2 for b in bufs])
        self._call("feed", ptrs, ns)

    def feed_dev(self, ptrs, counts):
        """device pointers (4-byte aligned) and complex sample counts per channel; asynchronous on the handle's stream"""
        p = (C.c_void_p * self.n_ch)(*ptrs)
        n = (C.c_int64 * self.n_ch)(*counts)
        self._call("feed_dev", p, n)

    def feed_bank(self, bank: "ChannelizerBank"):
        """channel c takes what the bank's last feed produced for its channel c; ordered on the device, no host sync"""
        self._call("feed_bank", bank._h)

    def read(self, ch: int, cap: int | None = None) -> np.ndarray:
        if cap is None:
            cap = self.last_dev(ch)[1]
        out = np.empty(max(cap, 1), np.int16)
        n = self._fn("read")(self._h, ch, out.ctypes.data, cap)
        if n < 0:
            raise SdrxError(f"sdrx_{self._prefix}_read rc={n}: {lib().sdrx_last_error().decode()}")
        return out[:n].copy()

    def last_dev(self, ch: int):
        """(device pointer, count) of the last feed's audio of channel ch"""
        p, n = C.c_void_p(), C.c_int64()
        self._call("last_dev", ch, C.byref(p), C.byref(n))
        return p.value or 0, n.value

    def squelch_open(self, ch: int) -> bool:
        rc = self._fn("squelch_open")(self._h, ch)
        if rc < 0:
            raise SdrxError(f"sdrx_{self._prefix}_squelch_open rc={rc}: {lib().sdrx_last_error().decode()}")
        return bool(rc)

    def _design(self, ch: int, third: np.ndarray):
        nt, inc, lvl = C.c_int32(), C.c_int32(), C.c_float()
        taps = np.zeros(16 * 128, np.float32)
        self._call("get_design", ch, C.byref(nt), taps.ctypes.data, taps.size, third.ctypes.data, C.byref(inc), C.byref(lvl))
        return nt.value, taps[: 16 * nt.value].copy(), third, inc.value, lvl.value


class WfmDemodBank(_DemodBank):
    """N wideband-FM demodulators (WFMDemod::feed): int16 I/Q at the channelizer's output rate in, mono qint16 audio out."""
    _prefix, _cfg = "wfm", WfmCfg

    def levels(self, ch: int, reset: bool = False):
        """(m_magsqSum, m_magsqPeak, m_magsqCount); reset: as getMagSqLevels"""
        s, p, n = C.c_double(), C.c_double(), C.c_int64()
        self._call("levels", ch, C.byref(s), C.byref(p), C.byref(n), int(reset))
        return s.value, p.value, n.value

    def design(self, ch: int):
        """(taps per phase, taps [16 * ntaps], filter spectrum as 2048 floats, NCO increment, squelch level)"""
        return self._design(ch, np.zeros(2048, np.float32))


class BfmBank(_DemodBank):
    """N broadcast-FM stereo demodulators (BFMDemod::feed without RDS): int16 I/Q at the channelizer's output rate in; qint16 l, r
    audio and the Samples of the sink stream out."""
    _prefix, _cfg = "bfm", BfmCfg

    def __init__(self, cfgs, device: int = 0, rds=None):
        """rds: per channel whether RDS is on (m_rdsActive); None is sdrx_bfm_create"""
        if rds is None:
            super().__init__(cfgs, device)
            return
        self.n_ch = len(cfgs)
        if len(rds) != self.n_ch:
            raise ValueError("one rds entry per channel")
        arr = (self._cfg * self.n_ch)(*cfgs)
        flags = (BfmRdsCfg * self.n_ch)(*[BfmRdsCfg(int(v)) for v in rds])
        self._h = C.c_void_p()
        _check(lib().sdrx_bfmrds_create(C.byref(self._h), device, self.n_ch, arr, flags), "sdrx_bfmrds_create")
        self.cfgs = list(cfgs)

    def _rds(self, name: str, *args):
        """sdrx_bfmrds_<name>: the RDS calls carry a prefix of their own"""
        fn = getattr(lib(), "sdrx_bfmrds_" + name)
        rc = fn(self._h, *args)
        if rc < 0:
            raise SdrxError(f"sdrx_bfmrds_{name} rc={rc}: {lib().sdrx_last_error().decode()}")
        return rc

    def _rds_read(self, name: str, ch: int, dtype, width: int, cap: int) -> np.ndarray:
        out = np.empty((max(cap, 1), width) if width > 1 else max(cap, 1), dtype)
        return out[:self._rds(name, ch, out.ctypes.data, cap)].copy()

    def rds_bits_last_dev(self, ch: int):
        p, n = C.c_void_p(), C.c_int64()
        self._rds("bits_last_dev", ch, C.byref(p), C.byref(n))
        return p.value or 0, n.value

    def rds_groups_last_dev(self, ch: int):
        p, n = C.c_void_p(), C.c_int64()
        self._rds("groups_last_dev", ch, C.byref(p), C.byref(n))
        return p.value or 0, n.value

    def rds_bits(self, ch: int) -> np.ndarray:
        """the bits RDSDemod::process returned during the last feed"""
        return self._rds_read("read_bits", ch, np.uint8, 1, self.rds_bits_last_dev(ch)[1])

    def rds_groups(self, ch: int) -> np.ndarray:
        """the groups RDSDecoder::frameSync completed during the last feed, [n, 4] blocks"""
        return self._rds_read("read_groups", ch, np.uint16, 4, self.rds_groups_last_dev(ch)[1])

    def rds_bb(self, ch: int) -> np.ndarray:
        """m_parms.subcarr_bb[0] of every RDS sample of the last feed"""
        return self._rds_read("read_bb", ch, np.float32, 1, self.rds_state(ch).n_rds)

    def rds_report(self, ch: int):
        """(m_report.acc, m_report.qua, m_report.fclk, RDSDecoder::m_qua, synced())"""
        a, q, f, dq, sy = C.c_float(), C.c_float(), C.c_float(), C.c_float(), C.c_int32()
        self._rds("report", ch, C.byref(a), C.byref(q), C.byref(f), C.byref(dq), C.byref(sy))
        return a.value, q.value, f.value, dq.value, bool(sy.value)

    def rds_state(self, ch: int) -> BfmRdsState:
        st = BfmRdsState()
        self._rds("state", ch, C.byref(st))
        return st

    def rds_unsure(self, ch: int, reset: bool = False) -> int:
        """samples whose mixer product the cosine's enclosure does not pin (include/sdrx.h)"""
        return self._rds("unsure", ch, int(reset))

    def read(self, ch: int, cap: int | None = None) -> np.ndarray:
        """the last feed's audio as an [n, 2] array of (l, r)"""
        if cap is None:
            cap = self.last_dev(ch)[1]
        out = np.empty((max(cap, 1), 2), np.int16)
        n = self._fn("read")(self._h, ch, out.ctypes.data, cap)
        if n < 0:
            raise SdrxError(f"sdrx_bfm_read rc={n}: {lib().sdrx_last_error().decode()}")
        return out[:n].copy()

    def sink_last_dev(self, ch: int):
        """(device pointer, count) of the sink stream's Samples of the last feed of channel ch"""
        p, n = C.c_void_p(), C.c_int64()
        self._call("sink_last_dev", ch, C.byref(p), C.byref(n))
        return p.value or 0, n.value

    def read_sink(self, ch: int, cap: int | None = None) -> np.ndarray:
        """the Samples the last feed put into m_sampleBuffer, as an [n, 2] array of (re, im)"""
        if cap is None:
            cap = self.sink_last_dev(ch)[1]
        out = np.empty((max(cap, 1), 2), np.int16)
        n = self._fn("read_sink")(self._h, ch, out.ctypes.data, cap)
        if n < 0:
            raise SdrxError(f"sdrx_bfm_read_sink rc={n}: {lib().sdrx_last_error().decode()}")
        return out[:n].copy()

    def pilot(self, ch: int):
        """(locked(), get_pilot_level(), the bits of m_freq, the bits of m_phase) after the last feed"""
        k, lv, f, p = C.c_int32(), C.c_float(), C.c_uint32(), C.c_uint32()
        self._call("pilot", ch, C.byref(k), C.byref(lv), C.byref(f), C.byref(p))
        return bool(k.value), lv.value, f.value, p.value

    def levels(self, ch: int, reset: bool = False):
        """(m_magsqSum, m_magsqPeak, m_magsqCount); reset: as getMagSqLevels"""
        s, p, n = C.c_double(), C.c_double(), C.c_int64()
        self._call("levels", ch, C.byref(s), C.byref(p), C.byref(n), int(reset))
        return s.value, p.value, n.value

    def design(self, ch: int):
        """(taps per phase, taps [16 * ntaps], filter spectrum as 2048 floats, NCO increment, squelch level, the pilot loop's
        m_minfreq, m_maxfreq, m_phasor_b0, m_phasor_a1, m_phasor_a2, m_loopfilter_b0, m_loopfilter_b1, m_lock_delay, the RC filters'
        (m_b0, m_a1))"""
        nt, inc, lvl, ld = C.c_int32(), C.c_int32(), C.c_float(), C.c_int32()
        taps, filt = np.zeros(16 * 128, np.float32), np.zeros(2048, np.float32)
        pll, rc = np.zeros(7, np.float32), np.zeros(2, np.float32)
        self._call("get_design", ch, C.byref(nt), taps.ctypes.data, taps.size, filt.ctypes.data, C.byref(inc), C.byref(lvl), pll.ctypes.data,
                   C.byref(ld), rc.ctypes.data)
        return nt.value, taps[: 16 * nt.value].copy(), filt, inc.value, lvl.value, pll, ld.value, rc


class AmDemodBank(_DemodBank):
    """N AM demodulators (AMDemod::feed): int16 I/Q at the channelizer's output rate in, mono qint16 audio out.  `sync`: one
    AmSyncCfg per channel (synchronous AM where its pll is set), None for envelope mode everywhere."""
    _prefix, _cfg = "am", AmCfg

    def __init__(self, cfgs, device: int = 0, sync=None):
        if sync is None:
            super().__init__(cfgs, device)
            return
        if len(sync) != len(cfgs):
            raise ValueError("one AmSyncCfg per channel")
        self.n_ch = len(cfgs)
        self._open(device, self.n_ch, (AmCfg * self.n_ch)(*cfgs), (AmSyncCfg * self.n_ch)(*sync), create="create_ex")
        self.cfgs = list(cfgs)

    def pll(self, ch: int):
        """(getPllLocked(), getPllFrequency()) after the last feed"""
        k, f = C.c_int32(), C.c_float()
        self._call("pll", ch, C.byref(k), C.byref(f))
        return bool(k.value), f.value

    def sync_design(self, ch: int):
        """(the 51 folded m_pllFilt taps, the frequency-domain filter as re, im pairs, m_pll's a1, a2, b0, b1, b2)"""
        taps, filt, coef = np.zeros(51, np.float32), np.zeros(2 * 2048, np.float32), np.zeros(5, np.float32)
        n = C.c_int32()
        self._call("get_sync_design", ch, taps.ctypes.data, filt.ctypes.data, C.byref(n), coef.ctypes.data)
        return taps, filt[: 2 * n.value].copy(), coef

    def levels(self, ch: int, reset: bool = False):
        """(m_magsq, m_magsqSum, m_magsqPeak, m_magsqCount); reset: as getMagSqLevels"""
        m, s, p, n = C.c_double(), C.c_double(), C.c_double(), C.c_int64()
        self._call("levels", ch, C.byref(m), C.byref(s), C.byref(p), C.byref(n), int(reset))
        return m.value, s.value, p.value, n.value

    def design(self, ch: int):
        """(taps per phase, taps [16 * ntaps], the 151 folded Bandpass taps, NCO increment, squelch level)"""
        return self._design(ch, np.zeros(151, np.float32))


class AtvCfg(C.Structure):
    """sdrx_atv_cfg: one ATVDemod (in_rate, nco_freq = -frequencyOffset, the arguments of configureRF and configure, frames_cap)"""
    _fields_ = [("in_rate", C.c_int32), ("nco_freq", C.c_int32), ("modulation", C.c_int32), ("rf_bw", C.c_float), ("rf_opp_bw", C.c_float),
                ("fft_filtering", C.c_int32), ("decimator_enable", C.c_int32), ("fm_deviation", C.c_float), ("line_duration", C.c_float),
                ("top_duration", C.c_float), ("frames_per_s", C.c_float), ("standard", C.c_int32), ("n_lines", C.c_int32),
                ("level_synchro_top", C.c_float), ("level_black", C.c_float), ("hsync", C.c_int32), ("vsync", C.c_int32),
                ("invert_video", C.c_int32), ("scope", C.c_int32), ("frames_cap", C.c_int32)]


class AtvState(C.Structure):
    """sdrx_atv_state_t: the PROCESSING block of atvdemod.h, floats as their bits"""
    _fields_ = [("image_index", C.c_int32), ("synchro_points", C.c_int32), ("synchro_detected", C.c_int32),
                ("vertical_synchro_detected", C.c_int32), ("col_index", C.c_int32), ("sample_index", C.c_int32), ("row_index", C.c_int32),
                ("line_index", C.c_int32), ("avg_col_index", C.c_int32), ("screen_row", C.c_int32), ("amp_line_average", C.c_uint32),
                ("eff_min", C.c_uint32), ("eff_max", C.c_uint32), ("amp_min", C.c_uint32), ("amp_max", C.c_uint32), ("amp_delta", C.c_uint32),
                ("buffer_i", C.c_uint32 * 6), ("buffer_q", C.c_uint32 * 6)]


class AtvDesign(C.Structure):
    """sdrx_atv_design_t: applySettings' and applyStandard's integers"""
    _fields_ = [(k, C.c_int32) for k in ("samples_per_line", "samples_per_top", "samples_per_line_signals", "samples_per_hsync", "sync_lines",
                                         "black_lines", "eq_lines", "interleaved", "tv_rate", "cols", "rows", "nco_inc")]


class ATVBank(_DemodBank):
    """N ATV demodulators (ATVDemod::feed): int16 I/Q at the channelizer's output rate in; the frames the screen was asked to render,
    the screen, the scope stream (read(), int16 real parts) and the state out."""
    _prefix, _cfg = "atv", AtvCfg

    def _count(self, name: str, *args) -> int:
        n = self._fn(name)(self._h, *args)
        if n < 0:
            raise SdrxError(f"sdrx_atv_{name} rc={n}: {lib().sdrx_last_error().decode()}")
        return n

    def design(self, ch: int) -> AtvDesign:
        d = AtvDesign()
        self._call("get_design", ch, C.byref(d))
        return d

    def filters(self, ch: int):
        """(the decimator's phase-0 taps, m_DSBFilter's filter and filterOpp as 4096 floats each); empty arrays where the stage is off"""
        nt = C.c_int32()
        taps, f, fo = np.zeros(128, np.float32), np.zeros(4096, np.float32), np.zeros(4096, np.float32)
        n = self._count("get_filters", ch, C.byref(nt), taps.ctypes.data, taps.size, f.ctypes.data, fo.ctypes.data)
        return taps[:nt.value].copy(), f[:2 * n].copy(), fo[:2 * n].copy()

    def state(self, ch: int) -> AtvState:
        st = AtvState()
        self._call("state", ch, C.byref(st))
        return st

    def frames(self, ch: int):
        """(frames of the last feed that kept a snapshot, renderImage calls of the last feed)"""
        n = C.c_int64()
        return self._count("frames", ch, C.byref(n)), n.value

    def events(self, ch: int) -> np.ndarray:
        """for each render of the last feed the index of its input sample within the feed"""
        cap = self.frames(ch)[1]
        out = np.empty(max(cap, 1), np.int32)
        return out[:self._count("read_events", ch, out.ctypes.data, cap)].copy()

    def _image(self, ch: int, name: str, *args) -> np.ndarray:
        d = self.design(ch)
        out = np.empty((d.rows, d.cols), np.uint8)
        self._count(name, ch, *args, out.ctypes.data, out.size)
        return out

    def frame(self, ch: int, k: int) -> np.ndarray:
        """the screen as it stood at render k of the last feed: [rows, cols] grey levels"""
        return self._image(ch, "read_frame", k)

    def screen(self, ch: int) -> np.ndarray:
        """the screen after the last feed"""
        return self._image(ch, "read_screen")

    def frames_last_dev(self, ch: int):
        """(device pointer, stored frames, bytes from one to the next)"""
        p, n, pitch = C.c_void_p(), C.c_int64(), C.c_int64()
        self._call("frames_last_dev", ch, C.byref(p), C.byref(n), C.byref(pitch))
        return p.value or 0, n.value, pitch.value

    def screen_last_dev(self, ch: int):
        """(device pointer, rows, cols)"""
        p, r, c = C.c_void_p(), C.c_int32(), C.c_int32()
        self._call("screen_last_dev", ch, C.byref(p), C.byref(r), C.byref(c))
        return p.value or 0, r.value, c.value


class DatvCfg(C.Structure):
    """sdrx_datv_cfg: one DATVDemod down to p_symbols (msps, the arguments of DATVDemod::configure, finfo)"""
    _fields_ = [("msps", C.c_int32), ("sample_rate", C.c_int32), ("centre_frequency", C.c_int32), ("rf_bandwidth", C.c_int32),
                ("symbol_rate", C.c_int32), ("modulation", C.c_int32), ("fec", C.c_int32), ("standard", C.c_int32), ("sampler", C.c_int32),
                ("rolloff", C.c_float), ("excursion", C.c_int32), ("hard_metric", C.c_int32), ("viterbi", C.c_int32), ("allow_drift", C.c_int32),
                ("notch_filters", C.c_int32), ("finfo", C.c_float)]


class DatvState(C.Structure):
    """sdrx_datv_state_t: cstln_receiver's and fir_sampler's members, floats as their bits"""
    _fields_ = [(k, C.c_uint32) for k in ("mu", "phase", "freqw", "agc_gain", "est_insp", "est_sp", "est_ep", "meas_count")] + [
        ("update_freq_phase", C.c_int32), ("hist_p", C.c_uint32 * 6), ("hist_c", C.c_uint32 * 6), ("held", C.c_int32), ("chunks", C.c_int64),
        ("n_in", C.c_int64), ("n_symbols", C.c_int64)]


class DatvDesign(C.Structure):
    """sdrx_datv_design_t"""
    _fields_ = [(k, C.c_float) for k in ("omega", "min_omega", "max_omega", "min_freqw", "max_freqw", "freq_beta")] + [
        (k, C.c_int32) for k in ("meas_decimation", "rrc_steps", "ncoeffs", "readahead", "nsymbols", "nco_inc")]


#: sdrx_datv_meas_t as a numpy record: freq_out, ss_out, mer_out and the three estimates behind them
DATV_MEAS = np.dtype([(k, np.float32) for k in ("freq", "ss", "mer", "est_insp", "est_sp", "est_ep")])


class DatvBank(_DemodBank):
    """N DATV receivers (DATVDemod::feed down to p_symbols): int16 I/Q at the channelizer's output rate in; soft symbols, constellation
    points, measurements and the receiver's state out."""
    _prefix, _cfg = "datv", DatvCfg

    def _count(self, name: str, *args) -> int:
        n = self._fn(name)(self._h, *args)
        if n < 0:
            raise SdrxError(f"sdrx_datv_{name} rc={n}: {lib().sdrx_last_error().decode()}")
        return n

    def last_dev(self, ch: int):
        """(device pointer to the costs, device pointer to the symbols, count) of the last feed's soft symbols"""
        pc, ps, n = C.c_void_p(), C.c_void_p(), C.c_int64()
        self._call("last_dev", ch, C.byref(pc), C.byref(ps), C.byref(n))
        return pc.value or 0, ps.value or 0, n.value

    def read(self, ch: int, cap: int | None = None):
        """the soft symbols of the last feed: (cost int16, symbol uint8)"""
        if cap is None:
            cap = self.last_dev(ch)[2]
        cost, sym = np.empty(max(cap, 1), np.int16), np.empty(max(cap, 1), np.uint8)
        n = self._count("read", ch, cost.ctypes.data, sym.ctypes.data, cap)
        return cost[:n].copy(), sym[:n].copy()

    def points(self, ch: int) -> np.ndarray:
        """the constellation points of the last feed, one per chunk that had a symbol: float32 [n, 2]"""
        p, n = C.c_void_p(), C.c_int64()
        self._call("points_last_dev", ch, C.byref(p), C.byref(n))
        out = np.empty((max(n.value, 1), 2), np.float32)
        return out[:self._count("read_points", ch, out.ctypes.data, n.value)].copy()

    def meas(self, ch: int) -> np.ndarray:
        """the measurements of the last feed as DATV_MEAS records; ss and mer are computed on the host"""
        p, n = C.c_void_p(), C.c_int64()
        self._call("meas_last_dev", ch, C.byref(p), C.byref(n))
        out = np.zeros(max(n.value, 1), DATV_MEAS)
        return out[:self._count("read_meas", ch, out.ctypes.data, n.value)].copy()

    def state(self, ch: int) -> DatvState:
        st = DatvState()
        self._call("state", ch, C.byref(st))
        return st

    def design(self, ch: int) -> DatvDesign:
        d = DatvDesign()
        self._call("get_design", ch, C.byref(d))
        return d

    def tables(self, ch: int):
        """(RRC coefficients, trig16 as 131072 floats, the constellation table as 65536 x 8 bytes, symbols[] as 512 int8)"""
        co, tr, lut, sy = np.zeros(4096, np.float32), np.zeros(2 * 65536, np.float32), np.zeros(65536 * 8, np.uint8), np.zeros(512, np.int8)
        nc = self._count("get_tables", ch, co.ctypes.data, co.size, tr.ctypes.data, lut.ctypes.data, sy.ctypes.data)
        return co[:nc].copy(), tr, lut, sy

    def table_digests(self, ch: int) -> list:
        """sha256 of the four tables, in tables()'s order"""
        import hashlib
        return [hashlib.sha256(np.ascontiguousarray(t).tobytes()).hexdigest() for t in self.tables(ch)]


class LoraDemodBank(_DemodBank):
    """N LoRa demodulators (LoRaDemod::feed): int16 I/Q at the channelizer's output rate in; the Samples of m_sampleBuffer and
    the lines dumpRaw prints out."""
    _prefix, _cfg = "lora", LoraCfg

    def read(self, ch: int, cap: int | None = None) -> np.ndarray:
        """the Samples of the last feed, as an [n, 2] array of (re, im)"""
        if cap is None:
            cap = self.last_dev(ch)[1]
        out = np.empty((max(cap, 1), 2), np.int16)
        n = self._fn("read")(self._h, ch, out.ctypes.data, cap)
        if n < 0:
            raise SdrxError(f"sdrx_lora_read rc={n}: {lib().sdrx_last_error().decode()}")
        return out[:n].copy()

    def read_text(self, ch: int, cap: int | None = None) -> str:
        """the lines dumpRaw printed during the last feed, a newline after each; cap: the buffer's size (None: large enough)"""
        if cap is None:
            cap = 256 * (self.last_dev(ch)[1] // 4544 + 2)
        buf = C.create_string_buffer(max(cap, 1))
        n = self._fn("read_text")(self._h, ch, buf, cap)
        if n < 0:
            raise SdrxError(f"sdrx_lora_read_text rc={n}: {lib().sdrx_last_error().decode()}")
        return buf.raw[:n].decode("latin-1")

    def state(self, ch: int) -> LoraState:
        st = LoraState()
        self._call("state", ch, C.byref(st))
        return st

    def design(self, ch: int):
        """(taps per phase, taps [16 * ntaps], NCO increment, vrot as 256 floats, k2, the dechirp table as 512 floats, the Sample
        table as [128, 2] int16)"""
        nt, inc, k2 = C.c_int32(), C.c_int32(), C.c_float()
        taps, vrot, chirp = np.zeros(16 * 128, np.float32), np.zeros(256, np.float32), np.zeros(512, np.float32)
        sample = np.zeros((128, 2), np.int16)
        self._call("get_design", ch, C.byref(nt), taps.ctypes.data, taps.size, C.byref(inc), vrot.ctypes.data, C.byref(k2), chirp.ctypes.data,
                   sample.ctypes.data)
        return nt.value, taps[: 16 * nt.value].copy(), inc.value, vrot, k2.value, chirp, sample


class NfmDemodBank(_DemodBank):
    """N narrowband-FM demodulators (NFMDemod::feed, power squelch): int16 I/Q at the channelizer's output rate in, mono qint16
    audio out.  `tone`: one NfmToneCfg per channel (CTCSS), None for none."""
    _prefix, _cfg = "nfm", NfmCfg

    def __init__(self, cfgs, tone=None, device: int = 0):
        if tone is None:
            super().__init__(cfgs, device)
            return
        if len(tone) != len(cfgs):
            raise ValueError("one NfmToneCfg per channel")
        self.n_ch = len(cfgs)
        self._open(device, self.n_ch, (NfmCfg * self.n_ch)(*cfgs), (NfmToneCfg * self.n_ch)(*tone), create="create_ex")
        self.cfgs = list(cfgs)

    def ctcss(self, ch: int):
        """(m_ctcssIndex after the last feed, its tone in Hz, changes since create / reset)"""
        i, f, n = C.c_int32(), C.c_float(), C.c_int64()
        self._call("ctcss", ch, C.byref(i), C.byref(f), C.byref(n))
        return i.value, f.value, n.value

    def ctcss_events(self, ch: int):
        """the changes of m_ctcssIndex during the last feed: (audio sample positions, new indices)"""
        n = self._fn("ctcss_events")(self._h, ch, None, None, 0)
        if n < 0:
            raise SdrxError(f"sdrx_nfm_ctcss_events rc={n}: {lib().sdrx_last_error().decode()}")
        at, idx = np.zeros(max(n, 1), np.int64), np.zeros(max(n, 1), np.int32)
        self._fn("ctcss_events")(self._h, ch, at.ctypes.data, idx.ctypes.data, n)
        return at[:n].copy(), idx[:n].copy()

    def ctcss_powers(self, ch: int):
        """(power[32], toneDetected, maxPowerIndex of the last completed detector block, blocks completed since create / reset)"""
        p = np.zeros(32, np.float32)
        d, m, n = C.c_int32(), C.c_int32(), C.c_int64()
        self._call("ctcss_powers", ch, p.ctypes.data, C.byref(d), C.byref(m), C.byref(n))
        return p, bool(d.value), m.value, n.value

    def af_squelch(self, ch: int):
        """(m_afSquelchOpen after the last feed, AFSquelch's two moving-average sums, its m_squelchCount)"""
        o, k = C.c_int32(), C.c_int32()
        sums = np.zeros(2, np.float64)
        self._call("af_squelch", ch, C.byref(o), sums.ctypes.data, C.byref(k))
        return bool(o.value), sums, k.value

    def tone_design(self, ch: int):
        """(CTCSS block length N, detector rate, coef[32], the 151 folded Lowpass taps, AF block length N, AF tones[2], AF coef[2],
        AF threshold)"""
        n, r, an, th = C.c_int32(), C.c_int32(), C.c_int32(), C.c_double()
        coef, lp = np.zeros(32, np.float32), np.zeros(151, np.float32)
        at, ac = np.zeros(2, np.float64), np.zeros(2, np.float64)
        self._call("get_tone_design", ch, C.byref(n), C.byref(r), coef.ctypes.data, lp.ctypes.data, C.byref(an), at.ctypes.data, ac.ctypes.data,
                   C.byref(th))
        return n.value, r.value, coef, lp, an.value, at, ac, th.value

    def levels(self, ch: int, reset: bool = False):
        """(m_movingAverage, m_magsqSum, m_magsqPeak, m_magsqCount); reset: as getMagSqLevels"""
        m, s, p, n = C.c_double(), C.c_double(), C.c_double(), C.c_int64()
        self._call("levels", ch, C.byref(m), C.byref(s), C.byref(p), C.byref(n), int(reset))
        return m.value, s.value, p.value, n.value

    def design(self, ch: int):
        """(taps per phase, taps [16 * ntaps], the 151 folded Bandpass taps, NCO increment, squelch level, gate in samples)"""
        nt, inc, lvl, gate = C.c_int32(), C.c_int32(), C.c_float(), C.c_int32()
        taps, bp = np.zeros(16 * 128, np.float32), np.zeros(151, np.float32)
        self._call("get_design", ch, C.byref(nt), taps.ctypes.data, taps.size, bp.ctypes.data, C.byref(inc), C.byref(lvl), C.byref(gate))
        return nt.value, taps[: 16 * nt.value].copy(), bp, inc.value, lvl.value, gate.value


class SsbDemodBank(_DemodBank):
    """N SSB / DSB demodulators (SSBDemod::feed): int16 I/Q at the channelizer's output rate in; qint16 l,r audio and the
    decimated sideband stream of the spectrum sink out."""
    _prefix, _cfg = "ssb", SsbCfg

    def read(self, ch: int, cap: int | None = None) -> np.ndarray:
        """the last feed's audio as an [n, 2] array of (l, r)"""
        if cap is None:
            cap = self.last_dev(ch)[1]
        out = np.empty((max(cap, 1), 2), np.int16)
        n = self._fn("read")(self._h, ch, out.ctypes.data, cap)
        if n < 0:
            raise SdrxError(f"sdrx_ssb_read rc={n}: {lib().sdrx_last_error().decode()}")
        return out[:n].copy()

    def spectrum_last_dev(self, ch: int):
        """(device pointer, count) of the spectrum Samples of the last feed of channel ch"""
        p, n = C.c_void_p(), C.c_int64()
        self._call("spectrum_last_dev", ch, C.byref(p), C.byref(n))
        return p.value or 0, n.value

    def read_spectrum(self, ch: int, cap: int | None = None) -> np.ndarray:
        """the Samples the last feed handed to the spectrum sink, as an [n, 2] array of (re, im)"""
        if cap is None:
            cap = self.spectrum_last_dev(ch)[1]
        out = np.empty((max(cap, 1), 2), np.int16)
        n = self._fn("read_spectrum")(self._h, ch, out.ctypes.data, cap)
        if n < 0:
            raise SdrxError(f"sdrx_ssb_read_spectrum rc={n}: {lib().sdrx_last_error().decode()}")
        return out[:n].copy()

    def audio_active(self, ch: int) -> bool:
        rc = self._fn("audio_active")(self._h, ch)
        if rc < 0:
            raise SdrxError(f"sdrx_ssb_audio_active rc={rc}: {lib().sdrx_last_error().decode()}")
        return bool(rc)

    def levels(self, ch: int, reset: bool = False):
        """(m_magsq, m_magsqSum, m_magsqPeak, m_magsqCount); reset: as getMagSqLevels"""
        m, s, p, n = C.c_double(), C.c_double(), C.c_double(), C.c_int64()
        self._call("levels", ch, C.byref(m), C.byref(s), C.byref(p), C.byref(n), int(reset))
        return m.value, s.value, p.value, n.value

    def design(self, ch: int):
        """(taps per phase, taps [16 * ntaps], filter spectrum as 4096 floats, NCO increment, hn, gate in samples, threshold, m_volume)"""
        nt, inc, hn, gate, thr, vol = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_double(), C.c_float()
        taps, filt = np.zeros(16 * 256, np.float32), np.zeros(4096, np.float32)
        self._call("get_design", ch, C.byref(nt), taps.ctypes.data, taps.size, filt.ctypes.data, C.byref(inc), C.byref(hn), C.byref(gate),
                   C.byref(thr), C.byref(vol))
        return nt.value, taps[: 16 * nt.value].copy(), filt, inc.value, hn.value, gate.value, thr.value, vol.value


class UdpSrcCfg(C.Structure):
    """sdrx_udpsrc_cfg: one UDPSrc (in_rate, nco_freq = -frequencyOffset, UDPSrcSettings with the reference's SampleFormat values)"""
    _fields_ = [("in_rate", C.c_int32), ("nco_freq", C.c_int32), ("output_sample_rate", C.c_float), ("sample_format", C.c_int32),
                ("rf_bandwidth", C.c_float), ("fm_deviation", C.c_int32), ("gain", C.c_float), ("squelch_db", C.c_int32),
                ("squelch_gate", C.c_int32), ("squelch_enabled", C.c_int32), ("agc", C.c_int32)]


#: numpy dtype of one payload sample per UDPSrcSettings::SampleFormat: Sample16, Sample24 (two int32), Sample16, int16 ...
UDPSRC_PAYLOAD_DTYPES = {0: np.dtype((np.int16, 2)), 1: np.dtype((np.int32, 2)), 2: np.dtype((np.int16, 2)), 3: np.dtype(np.int16),
                         4: np.dtype((np.int16, 2)), 5: np.dtype((np.int16, 2)), 6: np.dtype(np.int16), 7: np.dtype(np.int16),
                         8: np.dtype(np.int16), 9: np.dtype(np.int16), 10: np.dtype(np.int16)}
#: sdrx_udpsrc_create_ex: accept the SSB formats 4 .. 7
UDPSRC_SSB_FORMATS = 1
#: UDPSrc::udpBlockSize: bytes of one datagram
UDPSRC_BLOCK_BYTES = 512


class UdpPayloadCutter:
    """UDPSink<T>::write on the host: the running payload stream of one channel cut into the reference's datagrams, exactly
    samples [k * M, (k + 1) * M) with M = 512 / sizeof(T) (128, 256 or 64 samples); the remainder waits for the next feed."""

    def __init__(self, sample_bytes: int):
        self.sample_bytes = int(sample_bytes)
        self.per_datagram = UDPSRC_BLOCK_BYTES // self.sample_bytes
        self._rest = b""
        self.sent = 0                     # samples handed out in datagrams so far

    def push(self, raw: bytes) -> list:
        data = self._rest + bytes(raw)
        k = len(data) // UDPSRC_BLOCK_BYTES
        self._rest = data[k * UDPSRC_BLOCK_BYTES:]
        self.sent += k * self.per_datagram
        return [data[i * UDPSRC_BLOCK_BYTES: (i + 1) * UDPSRC_BLOCK_BYTES] for i in range(k)]

    @property
    def pending(self) -> int:
        """samples waiting for a full datagram"""
        return len(self._rest) // self.sample_bytes


class ChannelAnalyzerBank(_DemodBank):
    """N ChannelAnalyzers (ChannelAnalyzer::feed): int16 I/Q at the channelizer's output rate in; the Samples the analyzer
    hands to its scope / spectrum sink out: the signal itself, its autocorrelation or the PLL's oscillator.  A bank in which a
    cfg sets pll or fll, or input_type 1, or which is given psk_order (m_pllPskOrder per channel, 1 .. 31), is created through
    sdrx_chanapll_create; pll_state(ch) then reads the loop."""
    _prefix, _cfg = "chana", ChanaCfg

    def __init__(self, cfgs, device: int = 0, psk_order=None):
        if psk_order is None and not any(k.pll or k.fll or k.input_type == 1 for k in cfgs):
            super().__init__(cfgs, device)
            return
        self.n_ch = len(cfgs)
        arr = (self._cfg * self.n_ch)(*cfgs)
        order = None
        if psk_order is not None:
            if len(psk_order) != self.n_ch:
                raise ValueError("psk_order: one per channel")
            order = (C.c_int32 * self.n_ch)(*[int(v) for v in psk_order])
        self._h = C.c_void_p()
        _check(lib().sdrx_chanapll_create(C.byref(self._h), device, self.n_ch, arr, order), "sdrx_chanapll_create")
        self.cfgs = list(cfgs)

    def pll_state(self, ch: int):
        """(isPllLocked, getPllFrequency, getPllDeltaPhase, getPllPhase) after the last feed, the floats as np.float32"""
        k, f, d, p = C.c_int32(), C.c_float(), C.c_float(), C.c_float()
        _check(lib().sdrx_chanapll_state(self._h, ch, C.byref(k), C.byref(f), C.byref(d), C.byref(p)), "sdrx_chanapll_state")
        return bool(k.value), np.float32(f.value), np.float32(d.value), np.float32(p.value)

    def read(self, ch: int, cap: int | None = None) -> np.ndarray:
        """the last feed's Samples as an [n, 2] array of (re, im)"""
        if cap is None:
            cap = self.last_dev(ch)[1]
        out = np.empty((max(cap, 1), 2), np.int16)
        n = self._fn("read")(self._h, ch, out.ctypes.data, cap)
        if n < 0:
            raise SdrxError(f"sdrx_chana_read rc={n}: {lib().sdrx_last_error().decode()}")
        return out[:n].copy()

    def positive_only(self, ch: int) -> bool:
        rc = self._fn("positive_only")(self._h, ch)
        if rc < 0:
            raise SdrxError(f"sdrx_chana_positive_only rc={rc}: {lib().sdrx_last_error().decode()}")
        return bool(rc)

    def magsq(self, ch: int) -> float:
        m = C.c_double()
        self._call("magsq", ch, C.byref(m))
        return m.value

    def seek(self, ch: int, filtered_samples: int):
        """a fresh channel whose filter has already put out this many samples of silence (sdrx_chana_seek)"""
        self._call("seek", ch, C.c_uint64(filtered_samples))

    def design(self, ch: int):
        """(taps per phase, taps [16 * ntaps], filter spectrum as 4096 floats, NCOF's phase increment)"""
        nt, inc = C.c_int32(), C.c_float()
        taps, filt = np.zeros(16 * 256, np.float32), np.zeros(4096, np.float32)
        self._call("get_design", ch, C.byref(nt), taps.ctypes.data, taps.size, filt.ctypes.data, C.byref(inc))
        return nt.value, taps[: 16 * nt.value].copy(), filt, inc.value


class UdpSrcBank(_DemodBank):
    """N UDPSrc channels (UDPSrc::feed, every sample format): int16 I/Q at the channelizer's output rate in (MagAGC for the SSB
    and AM formats when agc is set), the datagram payload samples and the spectrum Samples out.  A bank with an SSB format
    (LSB, USB, LSBMono, USBMono: 4 .. 7) is created through sdrx_udpsrc_create_ex; such a channel's payload comes in blocks of 256
    elements, format 4's interleaved with one raw I/Q element per resampled sample.  No socket is opened anywhere: payloads(ch)
    returns the bytes of the datagrams the reference would send."""
    _prefix, _cfg = "udpsrc", UdpSrcCfg

    def __init__(self, cfgs, device: int = 0):
        self.n_ch = len(cfgs)
        arr = (self._cfg * self.n_ch)(*cfgs)
        if any(4 <= k.sample_format <= 7 for k in cfgs):
            self._open(device, self.n_ch, arr, UDPSRC_SSB_FORMATS, create="create_ex")
        else:
            self._open(device, self.n_ch, arr)
        self.cfgs = list(cfgs)
        self._cutters = [UdpPayloadCutter(self.sample_bytes(c)) for c in range(self.n_ch)]

    def reset(self):
        super().reset()
        self._cutters = [UdpPayloadCutter(self.sample_bytes(c)) for c in range(self.n_ch)]

    def sample_bytes(self, ch: int) -> int:
        n = self._fn("sample_bytes")(self._h, ch)
        if n < 0:
            raise SdrxError(f"sdrx_udpsrc_sample_bytes rc={n}: {lib().sdrx_last_error().decode()}")
        return n

    def read_raw(self, ch: int) -> bytes:
        """the last feed's payload samples as bytes"""
        cap, size = self.last_dev(ch)[1], self._cutters[ch].sample_bytes
        out = np.empty(max(cap, 1) * size, np.uint8)
        n = self._fn("read")(self._h, ch, out.ctypes.data, cap)
        if n < 0:
            raise SdrxError(f"sdrx_udpsrc_read rc={n}: {lib().sdrx_last_error().decode()}")
        return out[: n * size].tobytes()

    def read(self, ch: int, cap: int | None = None) -> np.ndarray:
        """the last feed's payload samples: [n, 2] int16 (formats 0, 2, 4, 5), [n, 2] int32 (format 1) or [n] int16"""
        dt = UDPSRC_PAYLOAD_DTYPES[self.cfgs[ch].sample_format]
        a = np.frombuffer(self.read_raw(ch), dt.base).reshape((-1,) + dt.shape)
        return (a if cap is None else a[:cap]).copy()

    def payloads(self, ch: int) -> list:
        """the datagrams (512 bytes each) that the last feed completes for channel ch.  Call it after every feed: the handle keeps
        the last feed's samples only.  A second call for the same feed returns nothing, and a call after a feed whose samples were
        never collected raises, because the datagram stream would go on with a hole in it."""
        cut = self._cutters[ch]
        new = self.total(ch) - (cut.sent + cut.pending)     # samples the cutter has not been given yet
        if new == 0:
            return []
        if new != self.last_dev(ch)[1]:
            raise SdrxError(f"UdpSrcBank.payloads({ch}): {new} samples are outstanding but the last feed holds {self.last_dev(ch)[1]}: "
                            "payloads() was not called after an earlier feed")
        return cut.push(self.read_raw(ch))

    def spectrum_last_dev(self, ch: int):
        p, n = C.c_void_p(), C.c_int64()
        self._call("spectrum_last_dev", ch, C.byref(p), C.byref(n))
        return p.value or 0, n.value

    def read_spectrum(self, ch: int) -> np.ndarray:
        """the Samples the last feed handed to the spectrum sink, as an [n, 2] array of (re, im)"""
        cap = self.spectrum_last_dev(ch)[1]
        out = np.empty((max(cap, 1), 2), np.int16)
        n = self._fn("read_spectrum")(self._h, ch, out.ctypes.data, cap)
        if n < 0:
            raise SdrxError(f"sdrx_udpsrc_read_spectrum rc={n}: {lib().sdrx_last_error().decode()}")
        return out[:n].copy()

    def squelch_counts(self, ch: int):
        """(m_squelchOpenCount, m_squelchCloseCount)"""
        a, b = C.c_int32(), C.c_int32()
        self._call("squelch_counts", ch, C.byref(a), C.byref(b))
        return a.value, b.value

    def in_magsq(self, ch: int) -> float:
        v = C.c_double()
        self._call("in_magsq", ch, C.byref(v))
        return v.value

    def total(self, ch: int) -> int:
        n = self._fn("total")(self._h, ch)
        if n < 0:
            raise SdrxError(f"sdrx_udpsrc_total rc={n}: {lib().sdrx_last_error().decode()}")
        return n

    def ssb_state(self, ch: int):
        """formats 4 .. 7: (fftfilt's inptr after the last feed, blocks completed since creation or reset, the shared filter design
        as 512 complex64 bins)"""
        pend, blocks = C.c_int32(), C.c_int64()
        filt = np.zeros(1024, np.float32)
        self._call("ssb_state", ch, C.byref(pend), C.byref(blocks), filt.ctypes.data)
        return pend.value, blocks.value, filt.view(np.complex64)

    def design(self, ch: int) -> dict:
        nt, inc, gate, rel, lvl, fms, step = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_double(), C.c_float(), C.c_float()
        taps, bp, win, agc = np.zeros(16 * 128, np.float64), np.zeros(151, np.float64), np.zeros(3, np.int32), np.zeros(4, np.int32)
        thr = C.c_double()
        self._call("get_design", ch, C.byref(nt), taps.ctypes.data, taps.size, bp.ctypes.data, C.byref(inc), win.ctypes.data, C.byref(gate),
                   C.byref(rel), C.byref(lvl), C.byref(fms), C.byref(step), agc.ctypes.data, C.byref(thr))
        return {"agc": agc.tolist(), "agc_threshold": thr.value, "ntaps": nt.value, "taps": taps[: 16 * nt.value].copy(), "bandpass": bp, "nco_inc": inc.value, "windows": win.tolist(),
                "gate": gate.value, "release": rel.value, "level": lvl.value, "fm_scaling": fms.value, "step": step.value}


class AudioTailCfg(C.Structure):
    """sdrx_audiotail_cfg (include/sdrx.h)"""
    _fields_ = [("kind", C.c_int32), ("audio_rate", C.c_int32), ("volume", C.c_float),
                ("fm_scaling", C.c_float), ("squelch_level", C.c_float), ("squelch_gate", C.c_int32), ("af_bandwidth", C.c_float),
                ("agc_active", C.c_int32), ("agc_nb_samples", C.c_int32), ("agc_threshold_enable", C.c_int32), ("agc_gate", C.c_int32),
                ("agc_clamping", C.c_int32), ("agc_threshold", C.c_double)]


class AudioTail(_Handle, _Sync):
    """audio-rate tail of the NFM / SSB demods (squelch / MagAGC / delay line / Bandpass -> qint16) for N channels"""
    _prefix = "audiotail"

    def __init__(self, cfgs, device: int = 0):
        self.n_ch = len(cfgs)
        arr = (AudioTailCfg * self.n_ch)(*cfgs)
        self._open(device, self.n_ch, arr)

    def reset(self):
        self._call("reset")

    def feed(self, per_channel_cplx):
        ins = [np.ascontiguousarray(x, dtype=np.float32) for x in per_channel_cplx]
        outs = [np.zeros(max(x.size // 2, 1), np.int16) for x in ins]
        pi = (C.c_void_p * self.n_ch)(*[x.ctypes.data for x in ins])
        po = (C.c_void_p * self.n_ch)(*[x.ctypes.data for x in outs])
        ns = (C.c_int64 * self.n_ch)(*[x.size // 2 for x in ins])
        self._call("feed", pi, ns, po)
        return [o[: x.size // 2] for o, x in zip(outs, ins)]

    def feed_dev(self, in_ptrs, counts, out_ptrs):
        """device pointers per channel: counts[c] complex floats in, counts[c] qint16 out; asynchronous, sync() waits"""
        pi = (C.c_void_p * self.n_ch)(*in_ptrs)
        ns = (C.c_int64 * self.n_ch)(*counts)
        po = (C.c_void_p * self.n_ch)(*out_ptrs)
        self._call("feed_dev", pi, ns, po)


class IirCfg(C.Structure):
    _fields_ = [("order", C.c_int32), ("a", C.c_float * 9), ("b", C.c_float * 9)]


class IirBank(_Handle):
    """IIRFilter<float, Order> (sdrbase/dsp/iirfilter.h), one filter per channel"""
    _prefix = "iir"

    def __init__(self, specs, device: int = 0):
        """specs: list of (order, a, b)"""
        self.n_ch = len(specs)
        arr = (IirCfg * self.n_ch)()
        for i, (o, a, b) in enumerate(specs):
            arr[i].order = o
            for j in range(o + 1):
                arr[i].a[j] = a[j]; arr[i].b[j] = b[j]
        self._open(device, self.n_ch, arr)

    def reset(self):
        self._call("reset")

    def feed(self, per_channel):
        ins = [np.ascontiguousarray(x, dtype=np.float32) for x in per_channel]
        outs = [np.zeros(max(x.size, 1), np.float32) for x in ins]
        pi = (C.c_void_p * self.n_ch)(*[x.ctypes.data for x in ins])
        po = (C.c_void_p * self.n_ch)(*[x.ctypes.data for x in outs])
        ns = (C.c_int64 * self.n_ch)(*[x.size for x in ins])
        self._call("feed", pi, ns, po)
        return [o[: x.size] for o, x in zip(outs, ins)]


class Decimators24(_Handle, _Sync):
    """Decimators<qint32, qint16, 24, InputBits> of the reference's 24-bit sample build (decimators.h, SDR_RX_SAMPLE_24BIT):
    int16 I/Q in, {int32, int32} samples out; same call contract as Decimators.decimate()."""
    _prefix = "decim24"

    def __init__(self, log2_decim: int, fcpos: int = FC_CEN, input_bits: int = 12, device: int = 0):
        self._open(device, log2_decim, fcpos, input_bits)
        self.log2 = log2_decim

    def reset(self):
        self._call("reset")

    def decimate(self, buf) -> np.ndarray:
        buf = np.ascontiguousarray(buf, dtype=np.int16)
        out = np.empty(2 * ((buf.size // 2) >> self.log2) + 2, np.int32)
        n = C.c_int32()
        self._call("process", buf.ctypes.data, buf.size, out.ctypes.data, C.byref(n))
        return out[: 2 * n.value]


    def decimate_dev(self, d_iq: int, n_cplx: int, d_out: int) -> int:
        """device pointers (e.g. torch tensor .data_ptr()); asynchronous, sync() waits; returns the samples produced"""
        n = C.c_int64()
        self._call("process_dev", d_iq, n_cplx, d_out, C.byref(n))
        return n.value


class ChannelizerBank24(_Handle, _Sync):
    """N DownChannelizers (downchannelizer.cpp) of the 24-bit sample build on one {int32, int32} stream."""
    _prefix = "chan24_bank"

    def __init__(self, in_rate: int, req_rates, req_fcs, device: int = 0):
        rr = np.ascontiguousarray(req_rates, dtype=np.int32); rf = np.ascontiguousarray(req_fcs, dtype=np.int32)
        self.n_ch = rr.size
        self._open(device, in_rate, self.n_ch, rr.ctypes.data, rf.ctypes.data)

    def reset(self):
        self._call("reset")

    def info(self, ch: int):
        n, r, f = C.c_int32(), C.c_int32(), C.c_int32()
        modes = np.zeros(40, np.uint8)
        self._call("info", ch, C.byref(n), modes.ctypes.data, C.byref(r), C.byref(f))
        return modes[: n.value].copy(), r.value, f.value

    def feed_dev(self, d_iq: int, n_cplx: int):
        self._call("feed_dev", d_iq, n_cplx)

    def out_dev(self, ch: int):
        p, n = C.c_void_p(), C.c_int64()
        self._call("out_dev", ch, C.byref(p), C.byref(n))
        return p.value, n.value

    def feed(self, iq):
        """iq: interleaved int32 I/Q; returns the per-channel outputs of this feed"""
        iq = np.ascontiguousarray(iq, dtype=np.int32)
        self._call("feed", iq.ctypes.data, iq.size // 2)
        outs = []
        for c in range(self.n_ch):
            out = np.empty(iq.size + 2, np.int32)
            n = lib().sdrx_chan24_bank_read(self._h, c, out.ctypes.data, out.size // 2)
            if n < 0:
                _check(int(n), "sdrx_chan24_bank_read")
            outs.append(out[: 2 * n].copy())
        return outs


class IqImbalance(_Handle, _Sync, _SetStream):
    """DSPDeviceSourceEngine::iqCorrections(begin, end, true) (DC + I/Q imbalance, float flavour) for N device streams."""
    _prefix = "iqimb"

    def __init__(self, n_streams: int, device: int = 0):
        self.n = n_streams
        self._open(device, n_streams)

    def reset(self):
        self._call("reset")

    def process(self, per_stream_iq):
        """in place on copies: returns the corrected int16 I/Q per stream"""
        bufs = [_i16(x).copy() for x in per_stream_iq]
        ptrs = (C.c_void_p * self.n)(*[b.ctypes.data for b in bufs])
        ns = (C.c_int64 * self.n)(*[b.size // 2 for b in bufs])
        self._call("process", ptrs, ns)
        return bufs

    def process_dev(self, in_ptrs, out_ptrs, counts):
        """device pointers (4-byte aligned) and complex sample counts per stream; out may equal in; asynchronous on the
        handle's stream"""
        pi = (C.c_void_p * self.n)(*in_ptrs)
        po = (C.c_void_p * self.n)(*out_ptrs)
        ns = (C.c_int64 * self.n)(*counts)
        self._call("process_dev", pi, po, ns)


class SampleSinkFifo(_Handle):
    """sdrbase/dsp/samplesinkfifo.{h,cpp}: write / read / readBegin / readCommit."""
    _prefix = "fifo"

    def __init__(self, size: int):
        self._open(size)

    def set_size(self, size: int):
        self._call("set_size", size)

    size = property(lambda self: lib().sdrx_fifo_size(self._h))
    fill = property(lambda self: lib().sdrx_fifo_fill(self._h))
    dropped = property(lambda self: lib().sdrx_fifo_dropped(self._h))

    def write(self, iq) -> int:
        iq = _i16(iq)
        return lib().sdrx_fifo_write(self._h, iq.ctypes.data, iq.size // 2)

    def write_bytes(self, data: bytes) -> int:
        return lib().sdrx_fifo_write_bytes(self._h, data, len(data))

    def read(self, count: int) -> np.ndarray:
        out = np.empty(max(2 * count, 2), np.int16)
        n = lib().sdrx_fifo_read(self._h, out.ctypes.data, count)
        return out[: 2 * n]

    def read_begin(self, count: int):
        p1, p2, n1, n2 = C.c_void_p(), C.c_void_p(), C.c_uint32(), C.c_uint32()
        tot = lib().sdrx_fifo_read_begin(self._h, count, C.byref(p1), C.byref(n1), C.byref(p2), C.byref(n2))

        def view(p, n):
            if not n:
                return np.empty(0, np.int16)
            return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_int16)), shape=(2 * n,)).copy()

        return tot, view(p1, n1.value), view(p2, n2.value)

    def read_commit(self, count: int) -> int:
        return lib().sdrx_fifo_read_commit(self._h, count)


def measure_hbm_read(device: int = 0, n_bytes: int = 4 << 30, reps: int = 5) -> float:
    """GB/s of a read-only streaming kernel over n_bytes of HBM (best of reps) -- the measured roofline denominator"""
    v = C.c_double()
    _check(lib().sdrx_measure_hbm_read(device, n_bytes, reps, C.byref(v)), "sdrx_measure_hbm_read")
    return v.value
