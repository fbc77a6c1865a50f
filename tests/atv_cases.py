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
durations are a quarter sample above the whole numbers so that no rounding of the float product decides the integers."""
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
    for name in ("ato_state", "ato_design", "ato_hits"):
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

    def close(self):
        self.L.ato_destroy(self.h)
        self.h = None


def run_spans(L: C.CDLL, k: dict, spans) -> dict:
    o = OracleAtv(L, k)
    feeds = [o.feed(x) for x in spans]
    res = {"feeds": feeds, "hits": o.hits(), "design": design_words(o.design)}
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
