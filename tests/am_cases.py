"""Cases of the AM demodulator bank (sdrx_am_*) and the ctypes face of tests/am_oracle.c, shared by tests/test_am_oracle.py
(CPU), tests/test_am_gpu.py and the golden recorder tests/golden/make_golden_am.py.

A case is a demodulator configuration, a signal at the channel rate and the lengths of the feeds it is cut into:
    cfg = (in_rate, nco_freq, audio_rate, rf_bandwidth, volume, squelch_db, audio_mute, bandpass_enable)
    sig = {"kind": ...}   see signal()

The generator is the portable one of tests/wfm_cases.py (splitmix64 counters, integer phase accumulators) with an `am` kind:
a carrier at f0, tone-modulated with a given depth, whose amplitude follows a list of runs."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from tests.wfm_cases import _clip16, _gauss, _splitmix, _uniform_i16, cut  # noqa: F401  (cut is re-exported)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_SRC = os.path.join(ROOT, "tests", "am_oracle.c")
ORACLE_DIR = os.path.join(ROOT, "oracle")

DEFAULT = dict(rf=5000.0, vol=2.0, sq=-40.0, mute=0, bp=0)
PROBES = ("transitions", "below_changes", "count_zero", "count_cap", "fed", "open_root_zero", "first_open", "unwritten_reads", "open",
          "fed_after_closure")


# ---------------------------------------------------------------- oracle
def build_oracle() -> C.CDLL:
    so = os.path.join(tempfile.mkdtemp(), "libamo.so")
    if not os.path.exists(os.path.join(ORACLE_DIR, "libsdro.so")):
        subprocess.check_call(["make", "-C", ORACLE_DIR, "libsdro.so"])
    subprocess.check_call(["cc", "-std=gnu11", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", ORACLE_SRC, "-o", so,
                           "-L" + ORACLE_DIR, "-lsdro", "-Wl,-rpath," + ORACLE_DIR, "-lm"])
    L = C.CDLL(so)
    L.amo_create.restype = C.c_void_p
    L.amo_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_int, C.c_int]
    L.amo_destroy.argtypes = [C.c_void_p]
    L.amo_feed.restype = C.c_long
    L.amo_feed.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_void_p, C.c_long]
    L.amo_levels.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_long)]
    L.amo_squelch_open.restype = C.c_int
    L.amo_squelch_open.argtypes = [C.c_void_p]
    L.amo_squelch_count.restype = C.c_int
    L.amo_squelch_count.argtypes = [C.c_void_p]
    L.amo_probe.argtypes = [C.c_void_p, C.c_void_p]
    L.amo_design.restype = C.c_int
    L.amo_design.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_float)]
    return L


class OracleAm:
    def __init__(self, L: C.CDLL, cfg):
        self.L = L
        self.cfg = cfg
        self.h = L.amo_create(int(cfg[0]), int(cfg[1]), int(cfg[2]), float(cfg[3]), float(cfg[4]), float(cfg[5]), int(cfg[6]), int(cfg[7]))
        assert self.h

    def feed(self, iq: np.ndarray) -> np.ndarray:
        iq = np.ascontiguousarray(iq, np.int16)
        n = iq.size // 2
        cap = n + 16                            # at most one audio sample per input
        out = np.empty(cap, np.int16)
        k = self.L.amo_feed(self.h, iq.ctypes.data, n, out.ctypes.data, cap)
        assert k <= cap
        return out[:k].copy()

    def levels(self):
        m, s, p, n = C.c_double(), C.c_double(), C.c_double(), C.c_long()
        self.L.amo_levels(self.h, C.byref(m), C.byref(s), C.byref(p), C.byref(n))
        return m.value, s.value, p.value, n.value

    def squelch_open(self) -> bool:
        return bool(self.L.amo_squelch_open(self.h))

    def squelch_count(self) -> int:
        return self.L.amo_squelch_count(self.h)

    def probe(self) -> dict:
        out = np.zeros(len(PROBES), np.int64)
        self.L.amo_probe(self.h, out.ctypes.data)
        return dict(zip(PROBES, (int(v) for v in out)))

    def design(self):
        taps = np.zeros(16 * 128, np.float32)
        bp = np.zeros(151, np.float32)
        inc, lvl = C.c_int(), C.c_float()
        nt = self.L.amo_design(self.h, taps.ctypes.data, bp.ctypes.data, C.byref(inc), C.byref(lvl))
        return nt, taps[: 16 * nt].copy(), bp, inc.value, lvl.value

    def close(self):
        if self.h:
            self.L.amo_destroy(self.h)
            self.h = None

    __del__ = close


# ---------------------------------------------------------------- portable signals
def _amp_runs(n: int, runs, amps) -> np.ndarray:
    """amplitude amps[k % len] over runs[k % len] samples, cycled"""
    amp = np.empty(n)
    pos, k = 0, 0
    while pos < n:
        r = runs[k % len(runs)]
        amp[pos:pos + r] = amps[k % len(amps)]
        pos += r; k += 1
    return amp


def signal(sig: dict, n: int, rate: int, seed: int) -> np.ndarray:
    kind = sig["kind"]
    iq = np.empty(2 * n, np.int16)
    if kind == "zero":
        iq[:] = 0
    elif kind == "noise_full":                         # full-scale uniform I and Q
        iq[0::2] = _uniform_i16(seed, n, 1)
        iq[1::2] = _uniform_i16(seed, n, 2)
    elif kind == "const":                              # constant sample
        iq[0::2] = sig["i"]
        iq[1::2] = sig["q"]
    elif kind == "am":
        t = np.arange(n, dtype=np.float64)
        inc = int(round(sig.get("f0", 0.0) / rate * 4294967296.0))
        ph = ((np.arange(1, n + 1, dtype=np.int64) * inc) & 0xFFFFFFFF).astype(np.float64) * (2 * np.pi / 4294967296.0)
        amp = _amp_runs(n, sig["runs"], sig["amps"]) if "runs" in sig else np.full(n, float(sig.get("amp", 8000.0)))
        env = amp * (1.0 + float(sig.get("depth", 0.5)) * np.sin(2 * np.pi * float(sig.get("fa", 1000.0)) * t / rate))
        sg = float(sig.get("noise", 20.0))
        iq[0::2] = _clip16(env * np.cos(ph) + _gauss(seed, n, 3, sg))
        iq[1::2] = _clip16(env * np.sin(ph) + _gauss(seed, n, 4, sg))
        if "zero_at" in sig:                           # a stretch of exact zeros
            a, m = sig["zero_at"]
            iq[2 * a: 2 * (a + m)] = 0
    else:
        raise ValueError(kind)
    return iq


# ---------------------------------------------------------------- cases
def _ragged(n: int, seed: int) -> list[int]:
    """feed lengths adding up to n: empty, one- and two-sample feeds, the moving average's length, short and long spans"""
    z = _splitmix(seed, 4096, 9)
    out, left, k = [], n, 0
    head = [1, 0, 2, 15, 16, 17, 0, 1, 700]
    while left > 0:
        if k < len(head):
            m = head[k]
        else:
            r = int(z[k] % np.uint64(4))
            m = int(z[k + 1000] % np.uint64([3, 400, 3000, 40000][r])) + (0 if r == 0 else 1)
        m = min(m, left)
        out.append(m); left -= m; k += 1
    return out


def _cfg(in_rate, audio_rate, nco_freq=0, **kw):
    d = dict(DEFAULT); d.update(kw)
    return (in_rate, nco_freq, audio_rate, d["rf"], d["vol"], d["sq"], d["mute"], d["bp"])


BURST_RUNS = [9000, 2000, 30000, 7000, 4000, 3500, 50000, 20000]
#: the level-edge sample and squelch (see make_cases)
EDGE_IQ = (9703, 13007)
EDGE_DB = -6.10400677
_EDGES = [1, 15, 16, 17, 2, 3, 5, 7, 11, 13, 255, 256, 257, 1023, 1025, 4099, 10007, 0, 1]


def make_cases() -> list[dict]:
    cases = []

    def add(name, cfg, sig, n, splits=None, seed=None):
        seed = len(cases) + 1 if seed is None else seed
        cases.append({"name": name, "cfg": cfg, "sig": sig, "n": n, "seed": seed, "splits": splits or _ragged(n, seed)})

    am = lambda f0, **kw: dict({"kind": "am", "f0": f0, "depth": 0.5, "fa": 1000.0, "amp": 8000.0}, **kw)
    add("default_airband", _cfg(60000, 48000, nco_freq=-3000), am(3000.0), 90000)
    add("nondyadic_62500", _cfg(62500, 48000, nco_freq=1700), am(-1700.0, fa=700.0), 80000)           # serial resampler schedule
    add("step1_48k", _cfg(48000, 48000), am(0.0, fa=400.0), 60000)
    add("r96k_to_44k1", _cfg(96000, 44100, nco_freq=-12000), am(12000.0, depth=0.8), 120000)          # D 2205, H 4410, rate / 24 = 1837
    add("rf8330", _cfg(60000, 48000, nco_freq=5000, rf=8330.0), am(-5000.0, fa=2500.0), 60000)
    # squelch bursts: the amplitude alternates between 8000 and 30 (below the -40 dB level) over stretches shorter and longer
    # than the opening count (rate / 20) and the counter's cap (rate / 10)
    burst = am(3000.0, runs=BURST_RUNS, amps=[8000.0, 30.0], noise=20.0)
    add("burst", _cfg(60000, 48000, nco_freq=-3000), burst, sum(BURST_RUNS))
    add("burst_bandpass", _cfg(60000, 48000, nco_freq=-3000, bp=1), burst, sum(BURST_RUNS), seed=6)
    add("wrap_vol10", _cfg(60000, 48000, nco_freq=-3000, vol=10.0, sq=-50.0), am(3000.0, runs=[60000, 40000], amps=[300.0, 12000.0]), 100000)
    add("zero_gap", _cfg(60000, 48000, nco_freq=-3000), am(3000.0, noise=0.0, zero_at=(40000, 120)), 70000)
    # m_magsq within a few ulp of the level: a constant sample turned slowly by the NCO, the squelch found by search on the
    # oracle (tests/test_am_oracle.py::test_level_edge_case_straddles_the_level keeps it honest)
    add("level_edge", _cfg(48000, 48000, nco_freq=12, sq=EDGE_DB), {"kind": "const", "i": EDGE_IQ[0], "q": EDGE_IQ[1]}, 60000)
    add("earliest_open", _cfg(48000, 48000, sq=-100.0), {"kind": "const", "i": 30000, "q": 30000}, 60000)
    add("audio_mute", _cfg(60000, 48000, nco_freq=-3000, mute=1), am(3000.0), 60000)
    add("all_zero", _cfg(60000, 48000), {"kind": "zero"}, 60000)
    add("fullscale_noise", _cfg(60000, 48000, bp=1), {"kind": "noise_full"}, 60000)
    add("splits_edges", _cfg(60000, 48000, nco_freq=-2345, bp=1), am(2345.0), 100000, splits=_EDGES + [100000 - sum(_EDGES)])
    add("one_long_feed", _cfg(60000, 48000, nco_freq=-2345, bp=1), am(2345.0), 100000, splits=[100000], seed=15)
    for c in cases:
        assert sum(c["splits"]) == c["n"], c["name"]
    return cases


CASES = make_cases()


def inputs(case: dict) -> np.ndarray:
    return signal(case["sig"], case["n"], case["cfg"][0], case["seed"])


def run_oracle(L: C.CDLL, case: dict, splits=None) -> dict:
    o = OracleAm(L, case["cfg"])
    feeds = [o.feed(x) for x in cut(inputs(case), splits or case["splits"])]
    m, s, p, n = o.levels()
    res = {"feeds": feeds, "magsq": m, "sum": s, "peak": p, "count": n, "open": o.squelch_open(), "state": o.squelch_count(), "probe": o.probe()}
    o.close()
    return res


# ---------------------------------------------------------------- random cases
def random_case(rng, i) -> dict:
    """one random configuration, signal and split list; the order of the rng calls is part of the case set"""
    rates = [(60000, 48000), (62500, 48000), (48000, 48000), (96000, 44100), (120000, 48000), (75000, 48000), (48000, 8000), (50000, 44100),
             (48000, 32000), (16000, 1000)]
    in_rate, audio = rates[int(rng.integers(len(rates)))]
    rf = float(rng.choice([5000.0, 8330.0, 3000.0, 10000.0, 12345.0]))
    kind = str(rng.choice(["am", "burst", "noise_full", "zero", "am", "gap"]))
    f0 = float(rng.integers(-in_rate // 8, in_rate // 8))
    sig = {"kind": "am" if kind in ("burst", "gap") else kind, "f0": f0, "depth": float(rng.choice([0.0, 0.3, 0.9])), "fa": float(rng.integers(100, 3000)),
           "amp": float(rng.integers(50, 20000)), "noise": float(rng.integers(0, 50))}
    if kind == "burst":
        sig["runs"] = [int(v) for v in rng.integers(1, in_rate // 4, size=8)]
        sig["amps"] = [float(rng.integers(3000, 16000)), float(rng.integers(1, 200))]
    n = int(rng.integers(2000, 60000))
    if kind == "gap":
        sig["noise"] = 0.0
        sig["zero_at"] = (int(rng.integers(0, n)), int(rng.integers(1, 400)))
    cfg = (in_rate, -int(f0), audio, rf, float(rng.choice([0.5, 2.0, 10.0])), float(rng.choice([-100.0, -60.0, -40.0, -25.5, -10.0])),
           int(rng.random() < 0.1), int(rng.random() < 0.5))
    splits, left = [], n
    while left > 0:
        m = min(left, int(rng.choice([0, 1, 2, 16, 17, int(rng.integers(1, 3000)), int(rng.integers(1, 30000))])))
        splits.append(m); left -= m
    return {"name": f"random{i}", "cfg": cfg, "sig": sig, "n": n, "seed": 1000 + i, "splits": splits}


#: the seed of random_cases(): the cases the `ref` test of tests/test_am_oracle.py proves against the reference
RANDOM_SEED = 20261017


def random_cases(count: int = 100) -> list[dict]:
    """the first `count` random cases, drawn in order from one generator"""
    rng = np.random.default_rng(RANDOM_SEED)
    return [random_case(rng, i) for i in range(count)]
