"""Cases of the ATV demodulator bank (sdrx_atv_*), their synthetic video and the portable oracle.

tests/atv_oracle.cpp is a scalar restatement of ATVDemod::feed, built here with strict IEEE flags and linked to oracle/libsdro.so
for the NCO's table, FM3's discriminator, the Interpolator's taps and the FFT filter; it needs neither the reference tree nor Qt, so it gives the expected output of any
input where the GPU is.

The video is built per line on the sample grid of the channel rate: a sync pulse at level 0, a porch at the black level 0.3, a
ramp from black to white and a short front porch; a field starts with broad-pulse lines (sync level for nine tenths of the line)
that bring the line average under the vsync threshold.  `fields` lists the line counts of the fields in turn (cycled), so that odd
and even counts reach both branches of the interleaved vsync.  `lost` blanks a stretch of the stream to mid grey without sync.
AM puts the level on the envelope (0.1 + 0.9 v of the amplitude), FM on the phase step ((v - 0.5) pi `swing` per sample), both on
a carrier at `f0` Hz that the channel's NCO takes back to 0.

The small shape: 160000 S/s, 64 lines at 25 frames/s -- 100 samples per line, 7 per top, a screen of 82 columns; the line and top
durations are a quarter sample above the whole numbers so that no rounding of the float product decides the integers.

CASES all have that shape (or 40 / 3).  SHAPE_CASES, CUT_STREAMS and random_cases() below put the walk that takes a stretch of a
line at a time (atv_fast_stretch) at other line and top lengths; the oracle's geometry counters (GEO) say what they reach."""
from __future__ import annotations

import ctypes as C
import hashlib
import os
import subprocess
import tempfile

import numpy as np

from tests.wfm_cases import _clip16, _gauss, _uniform_i16, cut  # noqa: F401  (cut is re-exported)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_SRC = os.path.join(ROOT, "tests", "atv_oracle.cpp")
ORACLE_DIR = os.path.join(ROOT, "oracle")
CSRC = os.path.join(ROOT, "sdrangel_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "atv_golden.npz")
RANDOM_GOLDEN = os.path.join(ROOT, "tests", "golden", "atv_random_golden.npz")     # digests: golden_random_cases()

FM1, FM2, FM3, AM, USB, LSB = range(6)
PAL625, PAL525, STD405, SHORT_I, SHORT, HSKIP = range(6)

CFG_FIELDS = (("in_rate", "i"), ("nco_freq", "i"), ("modulation", "i"), ("rf_bw", "f"), ("rf_opp_bw", "f"), ("fft_filtering", "i"),
              ("decimator_enable", "i"), ("fm_deviation", "f"), ("line_duration", "f"), ("top_duration", "f"), ("frames_per_s", "f"),
              ("standard", "i"), ("n_lines", "i"), ("level_synchro_top", "f"), ("level_black", "f"), ("hsync", "i"), ("vsync", "i"),
              ("invert_video", "i"), ("scope", "i"), ("frames_cap", "i"))
STATE_INTS = ("image_index", "synchro_points", "synchro_detected", "vertical_synchro_detected", "col_index", "sample_index", "row_index",
              "line_index", "avg_col_index", "screen_row")
STATE_BITS = ("amp_line_average", "eff_min", "eff_max", "amp_min", "amp_max", "amp_delta")
DESIGN_FIELDS = ("samples_per_line", "samples_per_top", "samples_per_line_signals", "samples_per_hsync", "sync_lines", "black_lines", "eq_lines",
                 "interleaved", "tv_rate", "cols", "rows", "nco_inc")
#: the oracle's branch counters, in the order of atv_scan.hpp's ATV_HIT_ numbers, then the most renders within one line
HITS = ("hcorr_classic", "hcorr_hskip", "minus150", "no_hsync", "row_neg", "row_big", "col_neg", "col_big", "vsync_even", "vsync_odd",
        "half_frame", "half_frame_am", "delta_one", "hskip_render", "null_row", "max_renders_in_line")
#: the oracle's geometry counters of processClassic (ato_geo, the GEO_ enum of tests/atv_oracle.cpp): what a walk that takes 64
#: samples at a time can get wrong, each defined on the reference's own variables
GEO = ("detect_held", "detect_twice_near", "points_from_far", "vsync_tie", "vsync_first_col", "vsync_last_col", "vsync_again", "col_negative",
       "col_past_line", "line_past_frame", "row_stays", "nan_at_check", "detect_at_half")


class Cfg(C.Structure):
    """sdrx_atv_cfg"""
    _fields_ = [(k, C.c_int32 if t == "i" else C.c_float) for k, t in CFG_FIELDS]


class State(C.Structure):
    """sdrx_atv_state_t"""
    _fields_ = [(k, C.c_int32) for k in STATE_INTS] + [(k, C.c_uint32) for k in STATE_BITS] + [("buffer_i", C.c_uint32 * 6), ("buffer_q", C.c_uint32 * 6)]


class Design(C.Structure):
    """sdrx_atv_design_t"""
    _fields_ = [(k, C.c_int32) for k in DESIGN_FIELDS]


def state_words(st) -> list[int]:
    """every field of a state struct (the oracle's or the bank's), in order"""
    return [int(getattr(st, k)) for k in STATE_INTS + STATE_BITS] + [int(v) for v in st.buffer_i] + [int(v) for v in st.buffer_q]


def design_words(d) -> list[int]:
    return [int(getattr(d, k)) for k in DESIGN_FIELDS]


SMALL_RATE, SMALL_LINES, SMALL_SPL, SMALL_SPT = 160000, 64, 100, 7


def cfg(**kw) -> dict:
    """the small shape, FM3, classic Short standard, both syncs on, a scope"""
    d = dict(in_rate=SMALL_RATE, nco_freq=0, modulation=FM3, rf_bw=60000.0, rf_opp_bw=10000.0, fft_filtering=0, decimator_enable=0,
             fm_deviation=1.0, line_duration=(SMALL_SPL + 0.25) / SMALL_RATE, top_duration=(SMALL_SPT + 0.25) / SMALL_RATE, frames_per_s=25.0,
             standard=SHORT, n_lines=SMALL_LINES, level_synchro_top=0.1, level_black=0.3, hsync=1, vsync=1, invert_video=0, scope=1, frames_cap=4)
    d.update(kw)
    return d


def as_struct(k: dict, cls=Cfg):
    return cls(**{name: (int(k[name]) if t == "i" else float(k[name])) for name, t in CFG_FIELDS})


# ---------------------------------------------------------------- the video
def video_levels(n: int, spl: int, spt: int, fields, lead: int = 0, sync_extra: int = 1, broad: int = 2, skip: bool = False) -> np.ndarray:
    """the level (0 sync .. 0.3 black .. 1 white) of n samples: `lead` samples of black, then fields of the listed line counts.
    skip: a field starts with one line whose sync pulse is left out (the HSkip format) instead of `broad` broad-pulse lines"""
    line = np.full(spl, 0.3)
    line[:spt + sync_extra] = 0.0
    pic0, pic1 = 2 * (spt + sync_extra), spl - 3
    line[pic0:pic1] = 0.3 + 0.7 * np.arange(pic1 - pic0) / max(1, pic1 - pic0 - 1)
    wide = np.full(spl, 0.3)
    wide[:(9 * spl) // 10] = 0.0
    out = [np.full(lead, 0.3)]
    have, f = lead, 0
    while have < n:
        k = fields[f % len(fields)]
        f += 1
        head = [np.where(line > 0.0, line, 0.3)] if skip else [wide] * broad
        rows = head + [line * (1.0 if (r % 7) else 0.6) + (0.0 if (r % 7) else 0.12) * (line > 0.3) for r in range(k - len(head))]
        out += rows
        have += k * spl
    return np.concatenate(out)[:n]


def signal(sig: dict, k: dict, n: int, seed: int) -> np.ndarray:
    kind = sig["kind"]
    iq = np.empty(2 * n, np.int16)
    if kind == "zero":
        iq[:] = 0
        return iq
    if kind == "noise":
        iq[0::2], iq[1::2] = _uniform_i16(seed, n, 1), _uniform_i16(seed, n, 2)
        return iq
    if kind == "const":
        iq[0::2], iq[1::2] = sig["i"], sig["q"]
        return iq
    assert kind == "video", kind
    v = video_levels(n, sig.get("spl", SMALL_SPL), sig.get("spt", SMALL_SPT), sig.get("fields", [SMALL_LINES]), sig.get("lead", 0),
                     sig.get("sync_extra", 1), sig.get("broad", 2), sig.get("skip", False))
    for a, b in sig.get("lost", ()):
        v[a:b] = 0.6
    amp = float(sig.get("amp", 9000.0))
    t = np.arange(n, dtype=np.float64)
    ph = 2 * np.pi * sig.get("f0", 0.0) * t / k["in_rate"]
    if k["modulation"] == AM:
        env = amp * (0.1 + 0.9 * v)
    else:
        env = np.full(n, amp)
        ph = ph + np.cumsum((v - 0.5) * np.pi * sig.get("swing", 1.0))
    sigma = float(sig.get("sigma", 0.0))
    re = env * np.cos(ph) + (_gauss(seed, n, 1, sigma) if sigma else 0.0)
    im = env * np.sin(ph) + (_gauss(seed, n, 2, sigma) if sigma else 0.0)
    iq[0::2], iq[1::2] = _clip16(re), _clip16(im)
    for a, b in sig.get("silent", ()):                     # (0, 0) samples: FM1 / FM2 divide by a zero magnitude
        iq[2 * a:2 * b] = 0
    return iq


def inputs(case: dict) -> np.ndarray:
    return signal(case["sig"], case["cfg"], case["n"], case["seed"])


def sha(a: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _ragged(n: int, seed: int, pieces: int) -> list[int]:
    """a cut of n into `pieces` feeds of seeded lengths, a zero-length one among them"""
    r = (_uniform_i16(seed, pieces - 1, 9).astype(np.int64) + 32768) * n // 65536
    edges = sorted(set([0, n] + [int(v) for v in r]))
    out = [b - a for a, b in zip(edges[:-1], edges[1:])]
    return out[:1] + [0] + out[1:]


def _case(name: str, seed: int, n: int, sig: dict, splits=None, **kw) -> dict:
    return {"name": name, "seed": seed, "n": n, "sig": sig, "cfg": cfg(**kw), "splits": splits or _ragged(n, seed, 5)}


N5 = 5 * SMALL_LINES * SMALL_SPL            # five frames: 32000 samples
VIDEO = {"kind": "video", "fields": [SMALL_LINES], "sigma": 60.0}
SKIPPED = {"kind": "video", "fields": [SMALL_LINES], "sigma": 60.0, "skip": True}      # HSkip's own format
FIELDS_I = {"kind": "video", "fields": [31, 32, 33], "sigma": 60.0}             # odd and even fields for the interleaved standards

CASES = [
    # each modulation under classic and under HSkip
    _case("fm1_classic", 1, N5, VIDEO, modulation=FM1),
    _case("fm2_classic", 2, N5, VIDEO, modulation=FM2),
    _case("fm3_classic", 3, N5, VIDEO, modulation=FM3),
    _case("am_classic", 4, N5, VIDEO, modulation=AM),
    _case("fm1_hskip", 5, N5, dict(SKIPPED, lead=37), modulation=FM1, standard=HSKIP),
    _case("fm2_hskip", 6, N5, dict(SKIPPED, lead=11), modulation=FM2, standard=HSKIP),
    _case("fm3_hskip", 7, N5, dict(SKIPPED, lead=53), modulation=FM3, standard=HSKIP),
    _case("am_hskip", 8, N5, dict(SKIPPED, lead=29), modulation=AM, standard=HSKIP),
    _case("fm3_hskip_nohsync", 9, N5, dict(SKIPPED, lead=53), modulation=FM3, standard=HSKIP, hsync=0),
    # the standards: the interleaved ones on fields of odd and even length
    _case("short_interleaved", 10, N5, FIELDS_I, standard=SHORT_I, modulation=FM3),
    _case("std405", 11, N5, FIELDS_I, standard=STD405, modulation=FM1),
    _case("pal525", 12, N5, FIELDS_I, standard=PAL525, modulation=AM),
    _case("pal625_small", 13, N5, FIELDS_I, standard=PAL625, modulation=FM2),
    # 625 lines at 40 samples per line: the row ranges of PAL625, with and without vsync
    _case("pal625_rows", 14, 2 * 625 * 40, {"kind": "video", "spl": 40, "spt": 3, "fields": [312, 313], "sigma": 40.0}, standard=PAL625,
          n_lines=625, in_rate=1000000, line_duration=40.25 / 1000000, top_duration=3.25 / 1000000, modulation=FM3, frames_cap=2),
    _case("pal625_rows_novsync", 15, 2 * 625 * 40, {"kind": "video", "spl": 40, "spt": 3, "fields": [312, 313], "sigma": 40.0}, standard=PAL625,
          n_lines=625, in_rate=1000000, line_duration=40.25 / 1000000, top_duration=3.25 / 1000000, modulation=AM, vsync=0, frames_cap=2),
    # the switches
    _case("nohsync", 16, N5, dict(VIDEO, lead=41), hsync=0, modulation=FM3),
    _case("novsync_am", 17, N5, VIDEO, vsync=0, modulation=AM),
    _case("novsync_nohsync_fm1", 18, N5, dict(VIDEO, lead=13), vsync=0, hsync=0, modulation=FM1),
    _case("inverted", 19, N5, VIDEO, invert_video=1, modulation=FM3),
    _case("inverted_am", 20, N5, VIDEO, invert_video=1, modulation=AM, scope=0),
    _case("deviation_half", 21, N5, dict(VIDEO, swing=0.5), fm_deviation=0.5, modulation=FM1),
    _case("deviation_two_fm2", 22, N5, dict(VIDEO, swing=1.6), fm_deviation=2.0, modulation=FM2),
    _case("deviation_two_fm3", 23, N5, dict(VIDEO, swing=1.6), fm_deviation=2.0, modulation=FM3),
    _case("deviation_half_fm3", 24, N5, dict(VIDEO, swing=0.5), fm_deviation=0.5, modulation=FM3),
    # the oscillator: off, on, and an offset whose increment is 0
    _case("offset_fm3", 25, N5, dict(VIDEO, f0=20000.0), nco_freq=-20000, modulation=FM3),
    _case("offset_am", 26, N5, dict(VIDEO, f0=-31000.0), nco_freq=31000, modulation=AM),
    _case("offset_fm1", 27, N5, dict(VIDEO, f0=12345.0), nco_freq=-12345, modulation=FM1),
    _case("offset_tiny_fm2", 28, N5, VIDEO, nco_freq=20, modulation=FM2),
    # inputs that are no picture
    _case("noise_fm3", 29, 8000, {"kind": "noise"}, modulation=FM3, level_black=0.02, level_synchro_top=-0.2, frames_cap=1),
    _case("noise_fm1", 30, 8000, {"kind": "noise"}, modulation=FM1),
    _case("noise_am_hskip", 31, 8000, {"kind": "noise"}, modulation=AM, standard=HSKIP),
    _case("noise_fm2_novsync", 32, 8000, {"kind": "noise"}, modulation=FM2, vsync=0),
    _case("const_am", 33, 8000, {"kind": "const", "i": 3000, "q": -4000}, modulation=AM),
    _case("const_fm1", 34, 8000, {"kind": "const", "i": 3000, "q": -4000}, modulation=FM1),
    # offset 0 on samples with a zero real part: a mix with the zero-frequency oscillator, whose sine is 6.1e-17, would show in the buffers
    _case("const_i0_fm1_offset0", 51, 3000, {"kind": "const", "i": 0, "q": 5}, modulation=FM1),
    _case("const_q0_fm2_offset0", 52, 3000, {"kind": "const", "i": -7, "q": 0}, modulation=FM2),
    _case("const_fm3_hskip", 35, 8000, {"kind": "const", "i": 0, "q": 5}, modulation=FM3, standard=HSKIP),
    _case("zeros_fm1", 36, 8000, {"kind": "zero"}, modulation=FM1),
    _case("zeros_fm2", 37, 8000, {"kind": "zero"}, modulation=FM2, invert_video=1),
    _case("zeros_fm3", 38, 8000, {"kind": "zero"}, modulation=FM3),
    _case("zeros_am", 39, 8000, {"kind": "zero"}, modulation=AM, vsync=0),
    _case("zeros_offset_fm1", 40, 8000, {"kind": "zero"}, modulation=FM1, nco_freq=5000),
    _case("clipped_am", 41, N5, dict(VIDEO, amp=60000.0), modulation=AM),
    _case("clipped_fm2", 42, N5, dict(VIDEO, amp=60000.0), modulation=FM2),
    _case("silent_stretch_fm1", 43, N5, dict(VIDEO, silent=[(5000, 5003), (9000, 9400)]), modulation=FM1),
    _case("silent_stretch_fm2", 44, N5, dict(SKIPPED, silent=[(5000, 5001), (9000, 9400)]), modulation=FM2, standard=HSKIP),
    _case("sync_lost_fm3", 45, N5, dict(VIDEO, lost=[(9000, 17000)]), modulation=FM3),
    _case("sync_lost_am_hskip", 46, N5, dict(SKIPPED, lost=[(9000, 17000)], lead=29), modulation=AM, standard=HSKIP),
    _case("sync_lost_fm1_interleaved", 47, N5, dict(FIELDS_I, lost=[(9000, 17000)]), modulation=FM1, standard=SHORT_I),
    # the vsync fires, is re-armed by one sample above the level and fires again within the line: more renders than a frames_cap of 1
    _case("rearmed_vsync", 48, N5, VIDEO, splits=[N5 // 2, N5 - N5 // 2], modulation=FM1, frames_cap=1),
    # the decimator: every input emits at phase 0, a 72-tap FIR; off in every case above
    _case("decim_fm1", 53, N5, VIDEO, modulation=FM1, decimator_enable=1),
    _case("decim_fm3_offset", 54, N5, dict(VIDEO, f0=20000.0), modulation=FM3, decimator_enable=1, nco_freq=-20000),
    _case("decim_am_hskip", 55, N5, dict(SKIPPED, lead=29), modulation=AM, standard=HSKIP, decimator_enable=1, rf_bw=90000.0),
    _case("decim_fm2_tiny_feeds", 56, 700, VIDEO, splits=[1] * 80 + [0, 620], modulation=FM2, decimator_enable=1),
    # the FFT filter over more than 2 x 1024 samples: the zero lead (FM1: NaN), the lag of 1023, block refills; FM3 unfiltered
    _case("fft_am", 57, N5, VIDEO, modulation=AM, fft_filtering=1, rf_bw=70000.0, rf_opp_bw=20000.0),
    _case("fft_fm1", 58, N5, VIDEO, modulation=FM1, fft_filtering=1, rf_bw=70000.0, rf_opp_bw=70000.0),
    _case("fft_fm3", 59, N5, VIDEO, modulation=FM3, fft_filtering=1, rf_bw=30000.0, rf_opp_bw=5000.0),
    _case("fft_fm2_edges", 60, 3 * 1024 + 3, VIDEO, splits=[1022, 1, 1, 1, 1023, 1, 1024, 2], modulation=FM2, fft_filtering=1, nco_freq=7000),
    _case("fft_am_short_feeds", 61, 2600, VIDEO, splits=[300] * 8 + [0, 200], modulation=AM, fft_filtering=1, standard=HSKIP),
    _case("fft_zeros_fm1", 62, 2600, {"kind": "zero"}, modulation=FM1, fft_filtering=1),
    # both stages
    _case("decim_fft_fm1", 63, N5, VIDEO, modulation=FM1, fft_filtering=1, decimator_enable=1, rf_bw=75000.0, rf_opp_bw=30000.0),
    _case("decim_fft_fm3", 64, N5, dict(VIDEO, f0=-9000.0), modulation=FM3, fft_filtering=1, decimator_enable=1, nco_freq=9000),
    _case("decim_fft_am", 65, N5, VIDEO, modulation=AM, fft_filtering=1, decimator_enable=1, vsync=0),
    # one feed of everything, and feeds of one sample
    _case("one_feed", 49, N5, VIDEO, splits=[N5], modulation=AM),
    _case("tiny_feeds", 50, 700, VIDEO, splits=[1] * 16 + [0, 684], modulation=FM2),
]
BY_NAME = {c["name"]: c for c in CASES}


# ---------------------------------------------------------------- oracle
def build_oracle() -> C.CDLL:
    so = os.path.join(tempfile.mkdtemp(), "libato.so")
    if not os.path.exists(os.path.join(ORACLE_DIR, "libsdro.so")):
        subprocess.check_call(["make", "-C", ORACLE_DIR, "libsdro.so"])
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-I" + CSRC, ORACLE_SRC, "-o", so,
                           "-L" + ORACLE_DIR, "-lsdro", "-Wl,-rpath," + ORACLE_DIR, "-lm"])
    L = C.CDLL(so)
    L.ato_create.restype = C.c_void_p
    L.ato_create.argtypes = [C.c_void_p]
    L.ato_destroy.argtypes = [C.c_void_p]
    for name, args in (("ato_feed", [C.c_void_p, C.c_void_p, C.c_long]), ("ato_events", [C.c_void_p, C.c_void_p, C.c_long]),
                       ("ato_frame", [C.c_void_p, C.c_long, C.c_void_p]), ("ato_screen", [C.c_void_p, C.c_void_p]),
                       ("ato_scope", [C.c_void_p, C.c_void_p, C.c_long])):
        getattr(L, name).restype = C.c_long
        getattr(L, name).argtypes = args
    L.ato_filters.restype = C.c_int
    L.ato_filters.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    for name in ("ato_state", "ato_design", "ato_hits", "ato_geo"):
        getattr(L, name).restype = None
        getattr(L, name).argtypes = [C.c_void_p, C.c_void_p]
    return L


class OracleAtv:
    def __init__(self, L: C.CDLL, k: dict):
        self.L, self.k = L, k
        s = as_struct(k)
        self.h = L.ato_create(C.byref(s))
        assert self.h, k
        self.design = Design()
        L.ato_design(self.h, C.byref(self.design))

    def feed(self, iq: np.ndarray) -> dict:
        """one feed's outputs: events, the stored frames, the screen, the scope stream and the state's words"""
        iq = np.ascontiguousarray(iq, np.int16)
        n = iq.size // 2
        ne = self.L.ato_feed(self.h, iq.ctypes.data, n)
        events = np.empty(max(ne, 1), np.int32)
        assert self.L.ato_events(self.h, events.ctypes.data, ne) == ne
        rows, cols = self.design.rows, self.design.cols
        frames = []
        for i in range(min(ne, self.k["frames_cap"])):
            f = np.empty((rows, cols), np.uint8)
            assert self.L.ato_frame(self.h, i, f.ctypes.data) == rows * cols
            frames.append(f)
        screen = np.empty((rows, cols), np.uint8)
        self.L.ato_screen(self.h, screen.ctypes.data)
        scope = np.empty(n + 1, np.int16)
        ns = self.L.ato_scope(self.h, scope.ctypes.data, n + 1)
        st = State()
        self.L.ato_state(self.h, C.byref(st))
        return {"events": events[:ne].copy(), "frames": frames, "screen": screen, "scope": scope[:ns].copy(), "state": state_words(st)}

    def filters(self):
        """(the decimator's phase-0 taps, m_DSBFilter's filter and filterOpp as 4096 floats each); empty where the stage is off"""
        taps, f, fo = np.zeros(128, np.float32), np.zeros(4096, np.float32), np.zeros(4096, np.float32)
        nt = self.L.ato_filters(self.h, taps.ctypes.data, taps.size, f.ctypes.data, fo.ctypes.data)
        on = 4096 if self.k["fft_filtering"] else 0
        return taps[:nt].copy(), f[:on].copy(), fo[:on].copy()

    def hits(self) -> dict:
        out = (C.c_int64 * len(HITS))()
        self.L.ato_hits(self.h, out)
        return dict(zip(HITS, (int(v) for v in out)))

    def geo(self) -> dict:
        out = (C.c_int64 * len(GEO))()
        self.L.ato_geo(self.h, out)
        return dict(zip(GEO, (int(v) for v in out)))

    def close(self):
        self.L.ato_destroy(self.h)
        self.h = None


def run_spans(L: C.CDLL, k: dict, spans) -> dict:
    o = OracleAtv(L, k)
    feeds = [o.feed(x) for x in spans]
    res = {"feeds": feeds, "hits": o.hits(), "geo": o.geo(), "design": design_words(o.design)}
    o.close()
    return res


def run_oracle(L: C.CDLL, case: dict, splits=None) -> dict:
    return run_spans(L, case["cfg"], cut(inputs(case), splits or case["splits"]))


def merged(feeds, splits) -> dict:
    """feeds of one stream as one: every event re-based onto the stream, the last screen and state"""
    starts = np.concatenate([[0], np.cumsum(splits)[:-1]])
    ev = [f["events"].astype(np.int64) + int(s) for f, s in zip(feeds, starts)]
    return {"events": np.concatenate(ev) if ev else np.zeros(0, np.int64), "scope": np.concatenate([f["scope"] for f in feeds]),
            "screen": feeds[-1]["screen"], "state": feeds[-1]["state"]}


#: what the cases have to reach, summed over CASES (the issue's list): counter -> least count
COVERAGE = {"hcorr_classic": 1, "hcorr_hskip": 1, "minus150": 1, "no_hsync": 1, "row_neg": 1, "row_big": 1, "col_neg": 1, "col_big": 1,
            "vsync_even": 1, "vsync_odd": 1, "half_frame": 1, "half_frame_am": 1, "delta_one": 1, "hskip_render": 1, "null_row": 1,
            "max_renders_in_line": 2}


def assert_coverage(hits_per_case: list[dict]):
    total = {k: (max if k == "max_renders_in_line" else sum)(h[k] for h in hits_per_case) for k in HITS}
    short = {k: (total[k], v) for k, v in COVERAGE.items() if total[k] < v}
    assert not short, f"branches the cases do not reach (have, need): {short}"
    return total


# ---------------------------------------------------------------- the stretch walk at other shapes (atv_fast_stretch)
#: what SHAPE_CASES' FM classic cases have to reach, summed, on the oracle's geometry counters
GEO_COVERAGE = {k: 1 for k in GEO}
SHAPE_RATE = 1000000
#: samples per line / per top: lines against the 64-sample window, tops that need the carried count, rooms under 8
SHAPES = ((9, 1), (16, 2), (63, 5), (64, 5), (65, 5), (86, 31), (128, 9), (129, 64), (192, 70), (640, 47), (1000, 130), (100, 0),
          (127, 9), (129, 9), (192, 63), (192, 64), (192, 65))


def is_fm_classic(k: dict) -> bool:
    return k["modulation"] != AM and k["standard"] != HSKIP


def shape_cfg(spl: int, spt: int, rate: int = SHAPE_RATE, **kw) -> dict:
    d = dict(in_rate=rate, line_duration=(spl + 0.25) / rate, top_duration=(spt + 0.25) / rate, rf_bw=0.375 * rate, rf_opp_bw=0.0625 * rate, n_lines=16)
    d.update(kw)
    return cfg(**d)


def shape_video(spl: int, spt: int, mod: int, fields, **kw) -> dict:
    return dict({"kind": "video", "spl": spl, "spt": spt, "fields": list(fields), "sigma": 40.0}, **kw)


def _shape(name: str, seed: int, spl: int, spt: int, mod: int, frames: int = 3, sig=None, n=None, splits=None, fields=None, **kw) -> dict:
    """a case at `spl` samples per line and `spt` per top: `frames` frames of video and a third of a line, unless sig or n say otherwise"""
    k = shape_cfg(spl, spt, modulation=mod, **kw)
    sig = sig if sig is not None else shape_video(spl, spt, mod, fields or [k["n_lines"]])
    n = n if n is not None else frames * k["n_lines"] * spl + spl // 3
    return {"name": name, "seed": seed, "n": n, "sig": sig, "cfg": k, "splits": splits or _ragged(n, seed, 5)}


def _shape_cases() -> list[dict]:
    out = []
    for i, (spl, spt) in enumerate(SHAPES):                 # FM1, FM2 and FM3 in turn over the shapes; 16 to 24 lines, 3 or 4 frames
        mod = (FM1, FM2, FM3)[i % 3]
        lines = 16 + 2 * (i % 5)
        frames = 3 + i % 2 if (3 + i % 2) * lines * spl < 50000 else 3
        out.append(_shape(f"shape_{spl}_{spt}_fm{mod + 1}", 100 + i, spl, spt, mod, frames=frames, n_lines=lines))
    C2 = {"kind": "const", "i": 3000, "q": -4000}
    out += [
        # the other two modulations at the shapes nearest the window and at the far count
        _shape("shape_64_5_fm3", 120, 64, 5, FM3), _shape("shape_65_5_fm1", 121, 65, 5, FM1), _shape("shape_129_64_fm3", 122, 129, 64, FM3),
        _shape("shape_192_70_fm1", 123, 192, 70, FM1), _shape("shape_192_64_fm3", 124, 192, 64, FM3), _shape("shape_16_2_fm3", 125, 16, 2, FM3),
        _shape("shape_9_1_fm2", 126, 9, 1, FM2), _shape("shape_100_0_fm2", 127, 100, 0, FM2), _shape("shape_100_1_fm3", 128, 100, 1, FM3),
        # the interleaved standards on odd and even fields
        _shape("shape_short_i_65", 130, 65, 5, FM3, standard=SHORT_I, n_lines=17, fields=[8, 9]),
        _shape("shape_short_i_129", 131, 129, 64, FM2, standard=SHORT_I, n_lines=20, fields=[9, 10, 11]),
        _shape("shape_405_63", 132, 63, 5, FM1, standard=STD405, n_lines=33, fields=[16, 17]),
        _shape("shape_525_86", 133, 86, 31, FM3, standard=PAL525, n_lines=49, fields=[24, 25]),
        _shape("shape_625_128", 134, 128, 9, FM2, standard=PAL625, n_lines=53, fields=[26, 27]),
        # the switches
        _shape("shape_nohsync_65", 140, 65, 5, FM3, hsync=0, lead=23), _shape("shape_nohsync_640", 141, 640, 47, FM2, hsync=0, lead=301),
        _shape("shape_nohsync_9", 142, 9, 1, FM1, hsync=0), _shape("shape_novsync_129", 143, 129, 64, FM3, vsync=0),
        _shape("shape_novsync_nohsync_192", 144, 192, 65, FM1, vsync=0, hsync=0, lead=77), _shape("shape_novsync_16", 145, 16, 2, FM2, vsync=0),
        _shape("shape_inverted_86", 146, 86, 31, FM3, invert_video=1), _shape("shape_inverted_640", 147, 640, 47, FM1, invert_video=1, frames=2),
        _shape("shape_dev_half_128", 148, 128, 9, FM3, fm_deviation=0.5, sig=shape_video(128, 9, FM3, [16], swing=0.5)),
        _shape("shape_dev_two_192", 149, 192, 70, FM3, fm_deviation=2.0, sig=shape_video(192, 70, FM3, [16], swing=1.6)),
        _shape("shape_dev_two_63_fm2", 150, 63, 5, FM2, fm_deviation=2.0, sig=shape_video(63, 5, FM2, [16])),
        # the pulse exactly spt long: the noise on the porch decides whether the detection is held
        _shape("shape_exact_pulse_100", 151, 100, 7, FM3, sig=shape_video(100, 7, FM3, [16], sync_extra=0, sigma=300.0)),
        _shape("shape_exact_pulse_129", 152, 129, 64, FM3, sig=shape_video(129, 64, FM3, [16], sync_extra=0, sigma=300.0)),
        _shape("shape_exact_pulse_640", 153, 640, 47, FM2, sig=shape_video(640, 47, FM2, [16], sync_extra=0, sigma=200.0), frames=2),
        # sync lost for more than four lines before a line 0: the correction puts the column past the line; -150 wins: under 0
        _shape("shape_lost_past_line_65", 154, 65, 5, FM3, vsync=0, sig=shape_video(65, 5, FM3, [16], lost=[(201, 547)])),
        _shape("shape_lost_past_line_129", 155, 129, 9, FM3, vsync=0, sig=shape_video(129, 9, FM3, [16], lost=[(401, 1089)])),
        _shape("shape_lost_vsync_100", 156, 100, 7, FM3, sig=shape_video(100, 7, FM3, [16], lost=[(2656, 3289)]), frames=4),
        # a lead of 40 puts the pulses of the first lines in the left half: the -150 term wins at the first line 0
        _shape("shape_minus150_100", 157, 100, 7, FM3, sig=shape_video(100, 7, FM3, [16], lead=40)),
        _shape("shape_minus150_192", 158, 192, 9, FM2, vsync=0, sig=shape_video(192, 9, FM2, [16], lead=40)),
        # no vsync in the signal for more than a frame: the line index reaches the frame, the row stays
        _shape("shape_no_broad_65", 159, 65, 5, FM3, sig=shape_video(65, 5, FM3, [16], broad=0)),
        _shape("shape_no_broad_i_129", 160, 129, 64, FM2, standard=SHORT_I, sig=shape_video(129, 64, FM2, [16], broad=0)),
        # (0, 0) samples inside the vsync region under FM1: a NaN sum at the check
        _shape("shape_nan_100", 161, 100, 7, FM1, sig=shape_video(100, 7, FM1, [16], silent=[(880, 884), (2490, 2600)])),
        _shape("shape_nan_640", 162, 640, 47, FM1, frames=2, sig=shape_video(640, 47, FM1, [16], silent=[(3000, 3001), (9400, 9500)])),
        _shape("shape_nan_129_fm2", 163, 129, 64, FM2, sig=shape_video(129, 64, FM2, [16], silent=[(1000, 1001), (2150, 2200)])),
        # noise under tops of 1 and 2 samples: detections a few samples apart, and a vsync wherever the sum happens to be
        _shape("shape_noise_100_1", 164, 100, 1, FM3, sig={"kind": "noise"}, n=9000), _shape("shape_noise_100_2", 165, 100, 2, FM1, sig={"kind": "noise"}, n=9000),
        _shape("shape_noise_9_1", 166, 9, 1, FM3, sig={"kind": "noise"}, n=6000, level_black=0.6), _shape("shape_noise_16_2", 167, 16, 2, FM2, sig={"kind": "noise"}, n=6000),
        _shape("shape_noise_65_2", 168, 65, 2, FM3, sig={"kind": "noise"}, n=9000, level_black=0.6, level_synchro_top=0.25),
        _shape("shape_noise_640_47", 169, 640, 47, FM3, sig={"kind": "noise"}, n=9000, level_synchro_top=0.25),
        # the tie: constant I/Q under FM3 is exactly 0.5 from the second sample on; 3 * 86 / 4 = 64 and level_black 0.5 put the level at 16.0,
        # which the sum equals at the first check of a line with 31 per top, passes by 0.5 with 30 and misses by 0.5 with 32
        _shape("shape_tie_86_31", 170, 86, 31, FM3, sig=C2, n=4000, level_black=0.5),
        _shape("shape_tie_86_30", 171, 86, 30, FM3, sig=C2, n=4000, level_black=0.5),
        _shape("shape_tie_86_32", 172, 86, 32, FM3, sig=C2, n=4000, level_black=0.5),
        # other inputs that are no picture
        _shape("shape_zeros_129_fm1", 173, 129, 64, FM1, sig={"kind": "zero"}, n=5000), _shape("shape_const_640_fm2", 174, 640, 47, FM2, sig=C2, n=9000),
        _shape("shape_clipped_192", 175, 192, 64, FM2, sig=shape_video(192, 64, FM2, [16], amp=60000.0)),
        # the old path (AM, HSkip) on the new shapes, and the front stages
        _shape("shape_am_129", 176, 129, 64, AM), _shape("shape_hskip_65", 177, 65, 5, FM3, standard=HSKIP, sig=shape_video(65, 5, FM3, [16], skip=True, lead=20)),
        _shape("shape_decim_86", 178, 86, 31, FM1, decimator_enable=1), _shape("shape_fft_129", 179, 129, 64, FM3, fft_filtering=1),
        _shape("shape_offset_640", 180, 640, 47, FM3, frames=2, nco_freq=-125000, sig=shape_video(640, 47, FM3, [16], f0=125000.0)),
        # the true shape: PAL-625 at 10 MS/s, 64 us lines and 4.7 us tops, fields of 312 and 313 lines, about 700 lines of signal
        _shape("shape_pal625_10ms", 181, 640, 47, FM1, rate=10000000, n_lines=625, standard=PAL625, frames_cap=2, n=700 * 640,
               sig=shape_video(640, 47, FM1, [312, 313], sigma=60.0)),
    ]
    names = [c["name"] for c in out]
    assert len(set(names)) == len(names)
    return out


SHAPE_CASES = _shape_cases()
SHAPE_BY_NAME = {c["name"]: c for c in SHAPE_CASES}

# ---------------------------------------------------------------- every cut of four short streams
CUT_CHANNELS = 131                      # channel i gets the first i samples in the first feed and the rest in the second
CUT_TAIL = (1, 7, 8, 9, 63, 64, 65)     # then every channel these, in turn: the stretch is tried from a span of 8 on
_T = sum(CUT_TAIL)
CUT_STREAMS = [
    _shape("cut_100_7", 190, 100, 7, FM3, n=13 + 6 * 100 + _T, splits=[13 + 6 * 100 + _T], sig=shape_video(100, 7, FM3, [5], broad=1, lead=13, sigma=60.0)),
    _shape("cut_129_64", 191, 129, 64, FM2, n=7 * 129 + _T, splits=[7 * 129 + _T], sig=shape_video(129, 64, FM2, [6], broad=1, sigma=60.0)),
    _shape("cut_86_31_tie", 192, 86, 31, FM3, n=6 * 86 + _T, splits=[6 * 86 + _T], sig={"kind": "const", "i": 3000, "q": -4000}, level_black=0.5),
    _shape("cut_65_5_nohsync", 193, 65, 5, FM1, n=29 + 6 * 65 + _T, splits=[29 + 6 * 65 + _T], hsync=0, sig=shape_video(65, 5, FM1, [4], broad=1, lead=29, sigma=60.0)),
]


def cut_spans(case: dict, i: int) -> list[int]:
    """channel i's feeds of a cut stream: i samples, the rest of the body, then the tail's pieces"""
    body = case["n"] - _T
    assert 0 <= i <= body
    return [i, body - i] + list(CUT_TAIL)


# ---------------------------------------------------------------- random configurations
RANDOM_SEED = 20261021
RANDOM_RATES = (160000, 1000000, 2000000, 10000000)
#: the fewest lines each standard's screen needs one row for (lines - black lines >= 1), by ATVStd
LEAST_LINES = {PAL625: 49, PAL525: 45, STD405: 29, SHORT_I: 5, SHORT: 5, HSKIP: 2}


def _f32(v) -> float:
    return float(np.float32(v))


def random_case(rng, i: int) -> dict:
    std = int(rng.choice([PAL625, PAL525, STD405, SHORT_I, SHORT, HSKIP], p=[0.1, 0.1, 0.1, 0.25, 0.35, 0.1]))
    mod = int(rng.choice([FM1, FM2, FM3, AM], p=[0.3, 0.3, 0.3, 0.1]))
    spl = int(rng.integers(9, 701))
    spt = int(rng.integers(0, spl // 3 + 1))
    least = LEAST_LINES[std]
    n_lines = int(rng.integers(least, max(40, least + 8) + 1))           # to 40, or eight past the least where that is above 40
    rate = int(rng.choice(RANDOM_RATES))
    dev = float(rng.choice([1.0, 1.0, 0.5, 2.0]))
    half = rate // 2
    nco = int(rng.choice([0, 0, int(rng.integers(-half // 2, half // 2)), int(rng.integers(-half // 2, half // 2)), half - 1, 1 - half, half, -half]))
    k = shape_cfg(spl, spt, rate, modulation=mod, standard=std, n_lines=n_lines, fm_deviation=dev, nco_freq=nco,
                  hsync=int(rng.random() < 0.8), vsync=int(rng.random() < 0.8), invert_video=int(rng.random() < 0.2),
                  level_synchro_top=_f32(rng.uniform(-0.2, 0.25)), level_black=_f32(rng.uniform(0.02, 0.6)),
                  decimator_enable=int(rng.random() < 0.2), fft_filtering=int(rng.random() < 0.2),
                  rf_bw=_f32(rate * rng.uniform(0.3, 0.6)), rf_opp_bw=_f32(rate * rng.uniform(0.0, 0.3)),
                  scope=int(rng.random() < 0.5), frames_cap=int(rng.integers(1, 4)))
    n = min(20000, int(rng.integers(2, 5)) * n_lines * spl + int(rng.integers(0, spl)))
    kind = str(rng.choice(["video", "video", "video", "lossy", "lossy", "noise", "const", "zero", "clipped"]))
    if kind in ("video", "lossy", "clipped"):
        h = n_lines // 2
        fields = [h, n_lines - h] if std in (PAL625, PAL525, STD405, SHORT_I) else [n_lines]
        swing = min(dev, 1.6) if mod == FM3 else 1.0        # FM1 and FM2 answer the sine of the step
        sig = shape_video(spl, spt, mod, fields, swing=swing, sigma=float(rng.choice([0.0, 40.0, 300.0])), lead=int(rng.integers(0, spl)),
                          sync_extra=int(rng.integers(0, 2)), skip=std == HSKIP, f0=float(-nco) if abs(nco) < half // 2 else 0.0)
        if kind == "lossy":
            a = int(rng.integers(0, max(1, n - spl)))
            sig["lost"] = [(a, min(n, a + int(rng.integers(spl, 6 * spl + 1))))]
        if kind == "clipped":
            sig["amp"] = 60000.0
    elif kind == "const":
        sig = {"kind": "const", "i": int(rng.integers(-9000, 9001)), "q": int(rng.choice([0, int(rng.integers(-9000, 9001))]))}
    else:
        sig = {"kind": kind}
    seed = 1000 + i
    return {"name": f"random_{i:03d}", "seed": seed, "n": n, "sig": sig, "cfg": k, "splits": _ragged(n, seed, int(rng.integers(2, 6)))}


def random_cases(count: int = 100) -> list[dict]:
    """the first `count` random cases, drawn in order from one generator"""
    rng = np.random.default_rng(RANDOM_SEED)
    return [random_case(rng, i) for i in range(count)]


def golden_random_cases() -> list[dict]:
    """what tests/golden/atv_random_golden.npz records: the shape cases, the cut streams fed whole, the random cases"""
    return SHAPE_CASES + CUT_STREAMS + random_cases()


def load_random_golden() -> dict:
    """atv_random_golden.npz by case name, each entry as make_golden_atv.pack_digests packs a single run"""
    g = np.load(RANDOM_GOLDEN)
    out, f0, e0, k0 = {}, 0, 0, 0
    for i, name in enumerate(g["names"].tolist()):
        f1 = f0 + int(g["feeds"][i])
        e1, k1 = e0 + int(g["event_counts"][f0:f1].sum()), k0 + int(g["frame_counts"][f0:f1].sum())
        out[name] = {"in_sha256": g["in_sha256"][i], "design": g["design"][i], "event_counts": g["event_counts"][f0:f1], "events": g["events"][e0:e1],
                     "state": g["state"][f0:f1], "frame_counts": g["frame_counts"][f0:f1], "frames_sha256": g["frames_sha256"][k0:k1],
                     "screens_sha256": g["screens_sha256"][f0:f1], "scope_sha256": g["scope_sha256"][f0:f1]}
        f0, e0, k0 = f1, e1, k1
    return out


def assert_random_shares(cases):
    """the draw stays with the stretch: half of it FM under a classic standard, a tenth with a top of a stretch or more"""
    fm = sum(1 for c in cases if is_fm_classic(c["cfg"]))
    far = sum(1 for c in cases if int(c["cfg"]["top_duration"] * c["cfg"]["in_rate"]) >= 64)
    assert len(cases) == 100 and fm >= 50 and far >= 10, (len(cases), fm, far)
    return fm, far


def assert_geo_coverage(geo_per_case: list[dict]):
    total = {k: sum(g[k] for g in geo_per_case) for k in GEO}
    short = {k: (total[k], v) for k, v in GEO_COVERAGE.items() if total[k] < v}
    assert not short, f"geometry the FM classic shape cases do not reach (have, need): {short}"
    return total
