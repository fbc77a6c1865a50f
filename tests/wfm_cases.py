"""Cases of the wideband-FM demodulator bank (sdrx_wfm_*) and the ctypes face of tests/wfm_oracle.c, shared by
tests/test_wfm_oracle.py (CPU), tests/test_wfm_gpu.py and the golden recorder tests/golden/make_golden_wfm.py.

A case is a demodulator configuration, a signal at the channel rate and the lengths of the feeds it is cut into:
    cfg = (in_rate, nco_freq, audio_rate, rf_bandwidth, af_bandwidth, volume, squelch_db, audio_mute)
    sig = {"kind": ...}   see signal()

The generator is portable on purpose: uniform and near-Gaussian noise come from a counter-based splitmix64 in uint64
arithmetic, phases from a 32-bit integer accumulator; nothing depends on a library's random stream."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_SRC = os.path.join(ROOT, "tests", "wfm_oracle.c")
ORACLE_DIR = os.path.join(ROOT, "oracle")

DEFAULT = dict(rf=80000.0, af=15000.0, vol=2.0, sq=-60.0, mute=0)


def required_bw(rf_bw: int) -> int:
    """WFMDemod::requiredBW (wfmdemod.h:142-149)"""
    return 48000 if rf_bw <= 48000 else (3 * rf_bw) // 2


# ---------------------------------------------------------------- oracle
def build_oracle() -> C.CDLL:
    so = os.path.join(tempfile.mkdtemp(), "libwfo.so")
    if not os.path.exists(os.path.join(ORACLE_DIR, "libsdro.so")):
        subprocess.check_call(["make", "-C", ORACLE_DIR, "libsdro.so"])
    subprocess.check_call(["cc", "-std=gnu11", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", ORACLE_SRC, "-o", so,
                           "-L" + ORACLE_DIR, "-lsdro", "-Wl,-rpath," + ORACLE_DIR, "-lm"])
    L = C.CDLL(so)
    L.wfo_create.restype = C.c_void_p
    L.wfo_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int]
    L.wfo_destroy.argtypes = [C.c_void_p]
    L.wfo_feed.restype = C.c_long
    L.wfo_feed.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_void_p, C.c_long]
    L.wfo_levels.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_long)]
    L.wfo_squelch_open.restype = C.c_int
    L.wfo_squelch_open.argtypes = [C.c_void_p]
    L.wfo_squelch_state.restype = C.c_int
    L.wfo_squelch_state.argtypes = [C.c_void_p]
    L.wfo_count_ge.restype = C.c_long
    L.wfo_count_ge.argtypes = [C.c_void_p]
    L.wfo_design.restype = C.c_int
    L.wfo_design.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_float)]
    return L


class OracleWfm:
    def __init__(self, L: C.CDLL, cfg):
        self.L = L
        self.cfg = cfg
        self.h = L.wfo_create(int(cfg[0]), int(cfg[1]), int(cfg[2]), float(cfg[3]), float(cfg[4]), float(cfg[5]), float(cfg[6]), int(cfg[7]))
        assert self.h

    def feed(self, iq: np.ndarray) -> np.ndarray:
        iq = np.ascontiguousarray(iq, np.int16)
        n = iq.size // 2
        cap = n + 1024                          # pending (< 512) + new, at most one audio sample per input
        out = np.empty(cap, np.int16)
        k = self.L.wfo_feed(self.h, iq.ctypes.data, n, out.ctypes.data, cap)
        assert k <= cap
        return out[:k].copy()

    def levels(self):
        s, p, n = C.c_double(), C.c_double(), C.c_long()
        self.L.wfo_levels(self.h, C.byref(s), C.byref(p), C.byref(n))
        return s.value, p.value, n.value

    def squelch_open(self) -> bool:
        return bool(self.L.wfo_squelch_open(self.h))

    def squelch_state(self) -> int:
        return self.L.wfo_squelch_state(self.h)

    def count_ge(self) -> int:
        return self.L.wfo_count_ge(self.h)

    def design(self):
        taps = np.zeros(16 * 128, np.float32)
        filt = np.zeros(2048, np.float32)
        inc, lvl = C.c_int(), C.c_float()
        nt = self.L.wfo_design(self.h, taps.ctypes.data, filt.ctypes.data, C.byref(inc), C.byref(lvl))
        return nt, taps[: 16 * nt].copy(), filt, inc.value, lvl.value

    def close(self):
        if self.h:
            self.L.wfo_destroy(self.h)
            self.h = None

    __del__ = close


# ---------------------------------------------------------------- portable signals
_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def _splitmix(seed: int, n: int, stream: int = 0) -> np.ndarray:
    """n uint64 values: splitmix64 of the counters (seed, stream, i)"""
    with np.errstate(over="ignore"):
        z = (np.arange(n, dtype=np.uint64) + np.uint64((seed * 0x632BE59BD9B4E019 + stream * 0xD1342543DE82EF95) & 0xFFFFFFFFFFFFFFFF)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return z


def _uniform_i16(seed: int, n: int, stream: int) -> np.ndarray:
    return ((_splitmix(seed, n, stream) >> np.uint64(48)).astype(np.int64) - 32768).astype(np.int16)


def _gauss(seed: int, n: int, stream: int, sigma: float) -> np.ndarray:
    """near-Gaussian (sum of four 16-bit uniforms), integer arithmetic up to the final scale"""
    z = _splitmix(seed, n, stream)
    s = np.zeros(n, np.int64)
    for k in range(4):
        s += ((z >> np.uint64(16 * k)) & np.uint64(0xFFFF)).astype(np.int64)
    return (s - 2 * 65535).astype(np.float64) * (sigma / 37837.0)       # std of the sum: 65536 * sqrt(4 / 12)


def _fm_phase(n: int, rate: int, f0: float, dev: float, f_audio: float) -> np.ndarray:
    """phase in turns * 2^32 (uint32 accumulator) of a carrier at f0 frequency-modulated by a tone"""
    t = np.arange(n, dtype=np.float64)
    f = f0 + dev * np.sin(2 * np.pi * f_audio * t / rate)
    inc = np.round(f / rate * 4294967296.0).astype(np.int64)
    return (np.cumsum(inc) & 0xFFFFFFFF).astype(np.float64) * (2 * np.pi / 4294967296.0)


def _clip16(x: np.ndarray) -> np.ndarray:
    return np.clip(np.round(x), -32768, 32767).astype(np.int16)


def signal(sig: dict, n: int, rate: int, seed: int) -> np.ndarray:
    kind = sig["kind"]
    iq = np.empty(2 * n, np.int16)
    if kind == "zero":
        iq[:] = 0
    elif kind == "noise_full":                         # full-scale uniform I and Q
        iq[0::2] = _uniform_i16(seed, n, 1)
        iq[1::2] = _uniform_i16(seed, n, 2)
    elif kind == "const":                              # constant sample (level-edge case)
        iq[0::2] = sig["i"]
        iq[1::2] = sig["q"]
    elif kind in ("fm", "burst"):
        ph = _fm_phase(n, rate, sig.get("f0", 0.0), sig.get("dev", 50000.0), sig.get("fa", 1000.0))
        if kind == "fm":
            amp = np.full(n, float(sig.get("amp", 8000.0)))
        else:                                          # amplitude alternating hi / lo over the listed stretches (cycled)
            amp = np.empty(n)
            pos, k, hi = 0, 0, True
            runs = sig["runs"]
            while pos < n:
                r = runs[k % len(runs)]
                amp[pos:pos + r] = sig["hi"] if hi else sig["lo"]
                pos += r; k += 1; hi = not hi
        sg = float(sig.get("noise", 20.0))
        iq[0::2] = _clip16(amp * np.cos(ph) + _gauss(seed, n, 3, sg))
        iq[1::2] = _clip16(amp * np.sin(ph) + _gauss(seed, n, 4, sg))
    else:
        raise ValueError(kind)
    return iq


# ---------------------------------------------------------------- cases
def _ragged(n: int, seed: int) -> list[int]:
    """feed lengths adding up to n: sub-block feeds, block edges and long spans"""
    z = _splitmix(seed, 4096, 9)
    out, left, k = [], n, 0
    head = [1, 511, 512, 513, 700]
    while left > 0:
        if k < len(head):
            m = head[k]
        else:
            r = int(z[k] % np.uint64(3))
            m = int(z[k + 1000] % np.uint64([400, 3000, 40000][r])) + 1
        m = min(m, left)
        out.append(m); left -= m; k += 1
    return out


def _cfg(in_rate, audio_rate, nco_freq=0, **kw):
    d = dict(DEFAULT); d.update(kw)
    return (in_rate, nco_freq, audio_rate, d["rf"], d["af"], d["vol"], d["sq"], d["mute"])


def make_cases() -> list[dict]:
    cases = []

    def add(name, cfg, sig, n, splits=None, seed=None):
        seed = len(cases) + 1 if seed is None else seed
        cases.append({"name": name, "cfg": cfg, "sig": sig, "n": n, "seed": seed, "splits": splits or _ragged(n, seed)})

    fm = lambda f0, dev=50000.0, fa=1000.0, amp=8000.0: {"kind": "fm", "f0": f0, "dev": dev, "fa": fa, "amp": amp}
    add("default_240k", _cfg(240000, 48000, nco_freq=-20000), fm(20000.0), 120000)
    add("default_120k", _cfg(120000, 48000, nco_freq=7000), fm(-7000.0, dev=30000.0), 90000)
    add("nbfm_48k_step1", _cfg(48000, 48000, rf=12500.0, af=3000.0), fm(0.0, dev=2500.0, fa=400.0), 40000)
    add("nondyadic_250k", _cfg(250000, 48000, nco_freq=31000), fm(-31000.0), 110000)
    add("r384k_to_44k1", _cfg(384000, 44100, nco_freq=-50000), fm(50000.0, dev=75000.0), 150000)
    add("wide_rf250k_384k", _cfg(384000, 48000, rf=250000.0), fm(0.0, dev=75000.0, fa=3000.0), 150000)
    # squelch bursts: open above rfBW / 20 samples, saturation at rfBW / 10.  Stretches shorter and longer than both, not
    # multiples of 512: the counter saturates at 0 and at the cap, opens and closes inside blocks, prevArg survives closures
    add("burst_48k", _cfg(48000, 48000, rf=12500.0, af=3000.0, sq=-30.0),
        {"kind": "burst", "dev": 2500.0, "fa": 400.0, "hi": 12000.0, "lo": 60.0, "noise": 5.0,
         "runs": [300, 200, 700, 100, 2000, 3000, 650, 640, 1300, 90, 5000, 4000]}, 70000)
    add("burst_240k_fraccap", _cfg(240000, 48000, rf=80005.0, sq=-30.0),            # rfBW / 10 = 8000.5: a non-integer cap
        {"kind": "burst", "dev": 50000.0, "fa": 1000.0, "hi": 12000.0, "lo": 60.0, "noise": 5.0,
         "runs": [3000, 1000, 5000, 700, 20000, 30000, 4100, 3900, 9000, 12000]}, 200000)
    # magsq within a few ulp of the level: a constant sample turned slowly by the NCO (increment 1), so that the filtered power
    # is constant up to rounding and straddles m_squelchLevel = pow(10, -0.6) sample by sample; (i, q) found by search on the
    # oracle (tests/test_wfm_oracle.py::test_level_edge_case_straddles_the_level keeps it honest)
    add("level_edge", _cfg(48000, 48000, nco_freq=12, rf=12500.0, af=3000.0, sq=-6.0), {"kind": "const", "i": EDGE_IQ[0], "q": EDGE_IQ[1]}, 60000)
    add("audio_mute", _cfg(240000, 48000, mute=1), fm(0.0), 60000)
    add("vol10_fullscale_noise", _cfg(240000, 48000, vol=10.0), {"kind": "noise_full"}, 60000)
    add("all_zero", _cfg(240000, 48000), {"kind": "zero"}, 50000)
    add("splits_edges", _cfg(240000, 48000, nco_freq=12345), fm(-12345.0), 100000,
        splits=_EDGES + [100000 - sum(_EDGES)])
    add("one_long_feed", _cfg(240000, 48000, nco_freq=12345), fm(-12345.0), 100000, splits=[100000], seed=13)
    for c in cases:
        assert sum(c["splits"]) == c["n"], c["name"]
    return cases


_EDGES = [1, 511, 512, 513, 2, 3, 5, 7, 11, 13, 509, 521, 1021, 1031, 4099, 10007, 0, 1]

#: the level-edge sample (see make_cases)
EDGE_IQ = (10077, 12971)

CASES = make_cases()


def dyadic_step(cfg) -> bool:
    """whether sdrx_wfm_create gives the channel the closed-form resampler schedule: the float step in_rate / audio_rate times 2^q
    is an integer below 2^20 for some q <= 10 (sdrangel_amd/csrc/sdrx_wfm.hip)"""
    step = np.float32(cfg[0]) / np.float32(cfg[2])
    return any(float(step) * (1 << q) == np.floor(float(step) * (1 << q)) < (1 << 20) for q in range(11))


#: the named cases that SDRX_WFM_SERIAL_SCHEDULE=1 moves from the closed form to the serial walk
DYADIC_CASES = [c for c in CASES if dyadic_step(c["cfg"])]


def inputs(case: dict) -> np.ndarray:
    return signal(case["sig"], case["n"], case["cfg"][0], case["seed"])


def cut(iq: np.ndarray, splits) -> list[np.ndarray]:
    out, pos = [], 0
    for m in splits:
        out.append(iq[2 * pos: 2 * (pos + m)])
        pos += m
    assert 2 * pos == iq.size
    return out


def run_oracle(L: C.CDLL, case: dict, splits=None) -> dict:
    o = OracleWfm(L, case["cfg"])
    feeds = [o.feed(x) for x in cut(inputs(case), splits or case["splits"])]
    s, p, n = o.levels()
    res = {"feeds": feeds, "sum": s, "peak": p, "count": n, "open": o.squelch_open(), "state": o.squelch_state(), "ge": o.count_ge()}
    o.close()
    return res


# ---------------------------------------------------------------- random cases
def random_case(rng, i) -> dict:
    """one random configuration, signal and split list; the order of the rng calls is part of the case set"""
    rates = [(240000, 48000), (120000, 48000), (48000, 48000), (250000, 48000), (384000, 44100), (384000, 48000), (96000, 8000),
             (200000, 44100), (48000, 32000)]
    in_rate, audio = rates[int(rng.integers(len(rates)))]
    rf = float(rng.choice([12500.0, 12345.0, 40000.0, 80000.0, 80005.0, 120000.0, 250000.0]))
    rf = min(rf, in_rate * 0.9)
    kind = str(rng.choice(["fm", "burst", "noise_full", "zero", "fm"]))
    f0 = float(rng.integers(-in_rate // 8, in_rate // 8))
    sig = {"kind": kind, "f0": f0, "dev": rf * 0.4, "fa": float(rng.integers(100, 5000)), "amp": float(rng.integers(50, 20000)),
           "hi": 12000.0, "lo": float(rng.integers(1, 200)), "noise": float(rng.integers(0, 50)),
           "runs": [int(v) for v in rng.integers(1, int(rf / 5), size=8)]}
    cfg = (in_rate, -int(f0), audio, rf, float(rng.choice([3000.0, 15000.0, 20000.0])), float(rng.choice([0.5, 2.0, 10.0])),
           float(rng.choice([-60.0, -30.0, -25.5, -10.0])), int(rng.random() < 0.1))
    n = int(rng.integers(2000, 60000))
    splits, left = [], n
    while left > 0:
        m = min(left, int(rng.choice([1, 511, 512, 513, int(rng.integers(1, 3000)), int(rng.integers(1, 30000))])))
        splits.append(m); left -= m
    return {"name": f"random{i}", "cfg": cfg, "sig": sig, "n": n, "seed": 1000 + i, "splits": splits}


#: the seed of random_cases(): the cases the `ref` test of tests/test_wfm_oracle.py proves against the reference
RANDOM_SEED = 20261017


def random_cases(count: int = 100) -> list[dict]:
    """the first `count` random cases, drawn in order from one generator"""
    rng = np.random.default_rng(RANDOM_SEED)
    return [random_case(rng, i) for i in range(count)]
