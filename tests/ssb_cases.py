"""Cases of the SSB / DSB demodulator bank (sdrx_ssb_*) and the ctypes face of tests/ssb_oracle.c, shared by
tests/test_ssb_oracle.py (CPU) and tests/test_ssb_gpu.py.

A case is a demodulator configuration, a signal at the channel rate and the lengths of the feeds it is cut into:
    cfg = dict(in_rate, nco_freq, audio_rate, rf_bandwidth, low_cutoff, volume, span_log2, audio_binaural, audio_flip, dsb,
               audio_mute, agc, agc_clamping, agc_time_log2, agc_power_threshold, agc_threshold_gate)
    sig = {"kind": ...}   see signal()
    reach = probe counters of the oracle that the case must leave non-zero: the branch it is named after

The generator is the portable one of tests/wfm_cases.py and tests/am_cases.py (splitmix64 counters, integer phase
accumulators): a tone beside the carrier whose amplitude follows a list of runs."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from tests.am_cases import _amp_runs
from tests.wfm_cases import _clip16, _fm_phase, _gauss, _splitmix, _uniform_i16, cut  # noqa: F401  (cut is re-exported)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_SRC = os.path.join(ROOT, "tests", "ssb_oracle.c")
ORACLE_DIR = os.path.join(ROOT, "oracle")

FIELDS = ("in_rate", "nco_freq", "audio_rate", "rf_bandwidth", "low_cutoff", "volume", "span_log2", "audio_binaural", "audio_flip", "dsb",
          "audio_mute", "agc", "agc_clamping", "agc_time_log2", "agc_power_threshold", "agc_threshold_gate")
#: SSBDemodSettings::resetToDefaults.  The default m_agc = false gives silence (include/sdrx.h): the cases that are to carry audio
#: switch the AGC on, `agc_off` is the literal default
DEFAULT = dict(nco_freq=0, rf_bandwidth=3000.0, low_cutoff=300.0, volume=3.0, span_log2=3, audio_binaural=0, audio_flip=0, dsb=0,
               audio_mute=0, agc=0, agc_clamping=0, agc_time_log2=7, agc_power_threshold=-40, agc_threshold_gate=4)
PROBES = ("resets", "gate_full", "count_full", "up_to_down", "down_to_up", "down_to_up_early", "clamped", "dl_wraps", "nan_writes", "groups",
          "step_up_full", "step_down_zero")


# ---------------------------------------------------------------- oracle
def build_oracle() -> C.CDLL:
    so = os.path.join(tempfile.mkdtemp(), "libssbo.so")
    if not os.path.exists(os.path.join(ORACLE_DIR, "libsdro.so")):
        subprocess.check_call(["make", "-C", ORACLE_DIR, "libsdro.so"])
    subprocess.check_call(["cc", "-std=gnu11", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", ORACLE_SRC, "-o", so,
                           "-L" + ORACLE_DIR, "-lsdro", "-Wl,-rpath," + ORACLE_DIR, "-lm"])
    L = C.CDLL(so)
    L.ssbo_create.restype = C.c_void_p
    L.ssbo_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float] + [C.c_int] * 10
    L.ssbo_destroy.argtypes = [C.c_void_p]
    L.ssbo_feed.restype = C.c_long
    L.ssbo_feed.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_void_p, C.c_long, C.c_void_p, C.c_long, C.POINTER(C.c_long)]
    L.ssbo_levels.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_long)]
    L.ssbo_audio_active.restype = C.c_int
    L.ssbo_audio_active.argtypes = [C.c_void_p]
    L.ssbo_state.argtypes = [C.c_void_p, C.c_void_p]
    L.ssbo_probe.argtypes = [C.c_void_p, C.c_void_p]
    L.ssbo_design.restype = C.c_int
    L.ssbo_design.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                              C.POINTER(C.c_double), C.POINTER(C.c_float)]
    return L


class OracleSsb:
    def __init__(self, L: C.CDLL, cfg: dict):
        self.L = L
        self.cfg = cfg
        k = [cfg[f] for f in FIELDS]
        self.h = L.ssbo_create(int(k[0]), int(k[1]), int(k[2]), float(k[3]), float(k[4]), float(k[5]), *[int(v) for v in k[6:]])
        assert self.h

    def feed(self, iq: np.ndarray):
        """(audio [n, 2] of l, r; spectrum Samples [m, 2] of re, im)"""
        iq = np.ascontiguousarray(iq, np.int16)
        n = iq.size // 2
        cap = n + 2048                            # at most one sideband sample per input, plus what the filter held back
        audio, spec = np.empty((cap, 2), np.int16), np.empty((cap, 2), np.int16)
        ns = C.c_long()
        k = self.L.ssbo_feed(self.h, iq.ctypes.data, n, audio.ctypes.data, cap, spec.ctypes.data, cap, C.byref(ns))
        assert k <= cap and ns.value <= cap
        return audio[:k].copy(), spec[: ns.value].copy()

    def levels(self):
        m, s, p, n = C.c_double(), C.c_double(), C.c_double(), C.c_long()
        self.L.ssbo_levels(self.h, C.byref(m), C.byref(s), C.byref(p), C.byref(n))
        return m.value, s.value, p.value, n.value

    def audio_active(self) -> bool:
        return bool(self.L.ssbo_audio_active(self.h))

    def state(self) -> tuple:
        out = np.zeros(10, np.float64)
        self.L.ssbo_state(self.h, out.ctypes.data)
        return tuple(out.tolist())

    def probe(self) -> dict:
        out = np.zeros(len(PROBES), np.int64)
        self.L.ssbo_probe(self.h, out.ctypes.data)
        return dict(zip(PROBES, (int(v) for v in out)))

    def design(self):
        taps, filt = np.zeros(16 * 256, np.float32), np.zeros(4096, np.float32)
        inc, hn, gate, thr, vol = C.c_int(), C.c_int(), C.c_int(), C.c_double(), C.c_float()
        nt = self.L.ssbo_design(self.h, taps.ctypes.data, filt.ctypes.data, C.byref(inc), C.byref(hn), C.byref(gate), C.byref(thr), C.byref(vol))
        return nt, taps[: 16 * nt].copy(), filt, inc.value, hn.value, gate.value, thr.value, vol.value

    def close(self):
        if self.h:
            self.L.ssbo_destroy(self.h)
            self.h = None

    __del__ = close


# ---------------------------------------------------------------- portable signals
def signal(sig: dict, n: int, rate: int, seed: int) -> np.ndarray:
    kind = sig["kind"]
    iq = np.empty(2 * n, np.int16)
    if kind == "zero":
        iq[:] = 0
    elif kind == "noise_full":                         # full-scale uniform I and Q
        iq[0::2] = _uniform_i16(seed, n, 1)
        iq[1::2] = _uniform_i16(seed, n, 2)
    elif kind == "tone":                               # a tone at f0 with a slow wobble, amplitude in runs
        ph = _fm_phase(n, rate, sig.get("f0", 0.0), sig.get("dev", 200.0), sig.get("fa", 3.0))
        amp = _amp_runs(n, sig["runs"], sig["amps"]) if "runs" in sig else np.full(n, float(sig.get("amp", 8000.0)))
        sg = float(sig.get("noise", 20.0))
        iq[0::2] = _clip16(amp * np.cos(ph) + _gauss(seed, n, 3, sg))
        iq[1::2] = _clip16(amp * np.sin(ph) + _gauss(seed, n, 4, sg))
    else:
        raise ValueError(kind)
    return iq


# ---------------------------------------------------------------- cases
def _ragged(n: int, seed: int) -> list[int]:
    """feed lengths adding up to n: empty and one-sample feeds, feeds that emit no block of 512, one block, three blocks
    (1536 outputs: a 1024-sample scan trip and a 64-term psum trip end mid-feed), then short and long spans"""
    z = _splitmix(seed, 4096, 9)
    out, left, k = [], n, 0
    head = [1, 0, 300, 700, 0, 1, 2000, 100, 640]
    while left > 0:
        if k < len(head):
            m = head[k]
        else:
            r = int(z[k] % np.uint64(4))
            m = int(z[k + 1000] % np.uint64([3, 400, 3000, 40000][r])) + (0 if r == 0 else 1)
        m = min(m, left)
        out.append(m); left -= m; k += 1
    return out


def _cfg(in_rate, audio_rate, **kw):
    d = dict(DEFAULT); d.update(kw)
    d["in_rate"], d["audio_rate"] = in_rate, audio_rate
    assert set(d) == set(FIELDS)
    return d


def hn_of(cfg) -> int:
    return (cfg["audio_rate"] // 1000) << cfg["agc_time_log2"]


def gate_of(cfg) -> int:
    return (cfg["audio_rate"] // 1000) * cfg["agc_threshold_gate"]


#: input runs at 60 kS/s (x 0.8 at the audio rate), strong and weak in turn, around the gate of 4 ms = 192 audio samples and
#: hn = 6144: after a silence longer than hn + L the AGC is down; strong bursts of 80 and 120 audio samples never fill the gate
#: and leave it down, the burst of 320 fills it and resets m_count
GATE_RUNS = [9000, 20000, 100, 3000, 150, 3000, 400, 2500, 12000, 12000, 200, 1000, 9000]
#: hn = 6144, L = 3072 at the audio rate: a gap of 9600 inputs = 7680 audio samples passes hn and is cut mid-descent; the gap
#: of 16000 = 12800 reaches the bottom (hn + L = 9216)
DOWN_RUNS = [20000, 9600, 15000, 16000, 20000]
#: hn = 16, L = 8 at 8 kS/s, in = audio rate
SHORT_RUNS = [3000, 20, 500, 21, 700, 30, 900, 10, 1500, 200, 4000, 12, 6000]
_EDGES = [1, 0, 511, 1, 512, 513, 1536, 2, 3, 5, 7, 255, 256, 257, 1023, 1025, 4099, 0, 1]


def make_cases() -> list[dict]:
    cases = []

    def add(name, cfg, sig, n, reach, splits=None, seed=None):
        seed = len(cases) + 1 if seed is None else seed
        cases.append({"name": name, "cfg": cfg, "sig": sig, "n": n, "seed": seed, "reach": reach, "splits": splits or _ragged(n, seed)})

    tone = lambda f0, **kw: dict({"kind": "tone", "f0": f0, "amp": 8000.0}, **kw)
    on = dict(agc=1)
    add("default_usb", _cfg(60000, 48000, nco_freq=-3000, **on), tone(4000.0), 60000, ["groups", "resets", "gate_full", "step_up_full"])
    add("lsb", _cfg(60000, 48000, nco_freq=-3000, rf_bandwidth=-3000.0, low_cutoff=-300.0, **on), tone(2000.0), 40000, ["groups", "resets"])
    add("dsb", _cfg(60000, 48000, nco_freq=-3000, dsb=1, **on), tone(4000.0), 40000, ["groups", "resets"])
    add("binaural", _cfg(60000, 48000, nco_freq=-3000, audio_binaural=1, **on), tone(4000.0), 30000, ["groups", "resets"])
    add("binaural_flip", _cfg(60000, 48000, nco_freq=-3000, audio_binaural=1, audio_flip=1, **on), tone(4000.0), 30000, ["groups", "resets"], seed=4)   # binaural's signal
    add("mute", _cfg(60000, 48000, nco_freq=-3000, audio_mute=1, **on), tone(4000.0), 30000, ["groups", "resets"])
    add("agc_off", _cfg(60000, 48000, nco_freq=-3000), tone(4000.0), 30000, ["groups"])
    add("threshold_disabled", _cfg(60000, 48000, nco_freq=-3000, agc_power_threshold=100, **on), tone(4000.0), 30000, ["groups"])
    add("gate", _cfg(60000, 48000, nco_freq=-3000, **on), tone(4000.0, runs=GATE_RUNS, amps=[8000.0, 30.0]), sum(GATE_RUNS),
        ["resets", "gate_full", "count_full", "up_to_down", "down_to_up"])
    add("clamping", _cfg(60000, 48000, nco_freq=-3000, agc_clamping=1, **on), tone(4000.0, runs=[12000, 9000, 12000, 7000], amps=[8000.0, 150.0]),
        40000, ["clamped", "resets"])
    add("step_down_and_back", _cfg(60000, 48000, nco_freq=-3000, agc_threshold_gate=0, **on), tone(4000.0, runs=DOWN_RUNS, amps=[8000.0, 30.0]),
        sum(DOWN_RUNS), ["count_full", "up_to_down", "down_to_up", "down_to_up_early", "step_down_zero", "step_up_full"])
    add("short_history", _cfg(8000, 8000, nco_freq=-1000, rf_bandwidth=2400.0, agc_time_log2=1, agc_threshold_gate=1, **on),
        tone(2000.0, runs=SHORT_RUNS, amps=[8000.0, 30.0]), sum(SHORT_RUNS),
        ["count_full", "up_to_down", "down_to_up", "step_down_zero", "step_up_full", "gate_full"])
    # hn = 98304 > the 96000 entries of the delay line: readBack clamps; more than 96000 audio samples: the line wraps
    add("long_history", _cfg(48000, 48000, nco_freq=-3000, agc_time_log2=11, **on), tone(4000.0), 120000, ["dl_wraps", "resets"], seed=13)
    add("span1", _cfg(60000, 48000, nco_freq=-3000, span_log2=1, **on), tone(4000.0), 20000, ["groups"])
    add("span8", _cfg(60000, 48000, nco_freq=-3000, span_log2=8, **on), tone(4000.0), 20000, ["groups"])
    add("resample_60k_48k", _cfg(60000, 48000, nco_freq=1700, **on), {"kind": "noise_full"}, 30000, ["groups", "resets"])
    add("resample_96k_8k", _cfg(96000, 8000, nco_freq=-12000, rf_bandwidth=2400.0, agc_time_log2=5, **on), tone(13000.0), 90000, ["groups", "resets"])
    add("zero", _cfg(60000, 48000, **on), {"kind": "zero"}, 20000, ["nan_writes", "groups"])
    # 700 inputs at 60 kS/s give 560 resampler outputs: exactly one block of 512
    add("first_block_only", _cfg(60000, 48000, nco_freq=-3000, **on), tone(4000.0), 700, ["groups"], splits=[300, 0, 399, 1])
    add("splits_edges", _cfg(48000, 48000, nco_freq=-3000, **on), tone(4000.0), 30000, ["groups", "resets"], splits=_EDGES + [30000 - sum(_EDGES)])
    for c in cases:
        assert sum(c["splits"]) == c["n"], c["name"]
    return cases


CASES = make_cases()


def inputs(case: dict) -> np.ndarray:
    return signal(case["sig"], case["n"], case["cfg"]["in_rate"], case["seed"])


def run_oracle(L: C.CDLL, case: dict, splits=None) -> dict:
    o = OracleSsb(L, case["cfg"])
    feeds = [o.feed(x) for x in cut(inputs(case), splits or case["splits"])]
    m, s, p, n = o.levels()
    res = {"audio": [f[0] for f in feeds], "spec": [f[1] for f in feeds], "magsq": m, "sum": s, "peak": p, "count": n,
           "active": o.audio_active(), "state": o.state(), "probe": o.probe(), "design": o.design()}
    o.close()
    return res


# ---------------------------------------------------------------- random cases
def random_case(rng, i) -> dict:
    """one random configuration, signal and split list; the order of the rng calls is part of the case set"""
    rates = [(60000, 48000), (62500, 48000), (48000, 48000), (96000, 44100), (120000, 48000), (48000, 8000), (50000, 44100), (48000, 32000),
             (16000, 1000), (192000, 192000)]
    in_rate, audio = rates[int(rng.integers(len(rates)))]
    kind = str(rng.choice(["tone", "burst", "noise_full", "zero", "tone", "burst"]))
    band = float(rng.choice([3000.0, 2400.0, 1500.0, 50.0, 5000.0])) * (audio / 48000.0 if audio < 16000 else 1.0)
    lsb = rng.random() < 0.3
    f0 = float(rng.integers(-in_rate // 8, in_rate // 8))
    sig = {"kind": "tone" if kind == "burst" else kind, "f0": f0 + (-1.0 if lsb else 1.0) * band / 3, "amp": float(rng.integers(50, 20000)),
           "noise": float(rng.integers(0, 50))}
    time_log2 = int(rng.choice([0, 1, 3, 5, 7, 7, 9]))
    hn = (audio // 1000) << time_log2
    if hn < 2:
        time_log2 = 1
    if kind == "burst":
        hn = (audio // 1000) << time_log2
        sig["runs"] = [int(v) for v in rng.integers(1, max(2, min(3 * hn * in_rate // audio, in_rate // 3)), size=8)]
        sig["amps"] = [float(rng.integers(3000, 16000)), float(rng.integers(1, 200))]
    n = int(rng.integers(2000, 60000))
    cfg = _cfg(in_rate, audio, nco_freq=-int(f0), rf_bandwidth=-band if lsb else band, low_cutoff=(-1.0 if lsb else 1.0) * float(rng.choice([300.0, 0.0, 100.0])),
                  volume=float(rng.choice([0.5, 3.0, 10.0])), span_log2=int(rng.integers(1, 9)), audio_binaural=int(rng.random() < 0.3),
                  audio_flip=int(rng.random() < 0.5), dsb=int(rng.random() < 0.2), audio_mute=int(rng.random() < 0.1), agc=int(rng.random() < 0.85),
                  agc_clamping=int(rng.random() < 0.4), agc_time_log2=time_log2, agc_power_threshold=int(rng.choice([-40, -40, -20, -60, -100, 100, 0])),
                  agc_threshold_gate=int(rng.choice([0, 1, 4, 4, 20])))
    splits, left = [], n
    while left > 0:
        m = min(left, int(rng.choice([0, 1, 2, 511, 513, int(rng.integers(1, 3000)), int(rng.integers(1, 30000))])))
        splits.append(m); left -= m
    return {"name": f"random{i}", "cfg": cfg, "sig": sig, "n": n, "seed": 1000 + i, "splits": splits, "reach": []}


#: the seed of random_cases(): the cases the `ref` test of tests/test_ssb_oracle.py proves against the reference
RANDOM_SEED = 20261017


def random_cases(count: int = 100) -> list[dict]:
    """the first `count` random cases, drawn in order from one generator"""
    rng = np.random.default_rng(RANDOM_SEED)
    return [random_case(rng, i) for i in range(count)]
