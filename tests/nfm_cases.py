"""Cases of the NFM demodulator bank (sdrx_nfm_*) and the ctypes face of tests/nfm_oracle.c, shared by tests/test_nfm_oracle.py
(CPU), tests/test_nfm_gpu.py and the golden recorder tests/golden/make_golden_nfm.py.

A case is a demodulator configuration, a signal at the channel rate and the lengths of the feeds it is cut into:
    cfg = (in_rate, nco_freq, audio_rate, rf_bandwidth, af_bandwidth, fm_deviation, volume, squelch, squelch_gate, audio_mute)
    sig = {"kind": ...}   see signal()

The generator is the portable one of tests/wfm_cases.py (splitmix64 counters, integer phase accumulators) with an `nfm` kind:
a carrier at f0, frequency-modulated by a tone, whose amplitude follows a list of runs."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from tests.am_cases import _amp_runs
from tests.wfm_cases import _clip16, _fm_phase, _gauss, _splitmix, _uniform_i16, cut  # noqa: F401  (cut is re-exported)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_SRC = os.path.join(ROOT, "tests", "nfm_oracle.c")
ORACLE_DIR = os.path.join(ROOT, "oracle")

#: NFMDemodSettings::resetToDefaults, with the squelch at -30 dB
DEFAULT = dict(rf=12500.0, af=3000.0, fmdev=2000, vol=2.0, sq=-300.0, gate=5, mute=0)
PROBES = ("transitions", "below_changes", "count_zero", "count_cap", "open", "clamped_reads", "wraps", "zero_ci")


# ---------------------------------------------------------------- oracle
def build_oracle() -> C.CDLL:
    so = os.path.join(tempfile.mkdtemp(), "libnfmo.so")
    if not os.path.exists(os.path.join(ORACLE_DIR, "libsdro.so")):
        subprocess.check_call(["make", "-C", ORACLE_DIR, "libsdro.so"])
    subprocess.check_call(["cc", "-std=gnu11", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", ORACLE_SRC, "-o", so,
                           "-L" + ORACLE_DIR, "-lsdro", "-Wl,-rpath," + ORACLE_DIR, "-lm"])
    L = C.CDLL(so)
    L.nfmo_create.restype = C.c_void_p
    L.nfmo_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, C.c_float, C.c_float, C.c_int, C.c_int]
    L.nfmo_destroy.argtypes = [C.c_void_p]
    L.nfmo_feed.restype = C.c_long
    L.nfmo_feed.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_void_p, C.c_long]
    L.nfmo_levels.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_long)]
    L.nfmo_squelch_open.restype = C.c_int
    L.nfmo_squelch_open.argtypes = [C.c_void_p]
    L.nfmo_squelch_count.restype = C.c_int
    L.nfmo_squelch_count.argtypes = [C.c_void_p]
    L.nfmo_probe.argtypes = [C.c_void_p, C.c_void_p]
    L.nfmo_design.restype = C.c_int
    L.nfmo_design.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_int)]
    return L


class OracleNfm:
    def __init__(self, L: C.CDLL, cfg):
        self.L = L
        self.cfg = cfg
        self.h = L.nfmo_create(int(cfg[0]), int(cfg[1]), int(cfg[2]), float(cfg[3]), float(cfg[4]), int(cfg[5]), float(cfg[6]), float(cfg[7]),
                               int(cfg[8]), int(cfg[9]))
        assert self.h

    def feed(self, iq: np.ndarray) -> np.ndarray:
        iq = np.ascontiguousarray(iq, np.int16)
        n = iq.size // 2
        cap = n + 16                            # at most one audio sample per input
        out = np.empty(cap, np.int16)
        k = self.L.nfmo_feed(self.h, iq.ctypes.data, n, out.ctypes.data, cap)
        assert k <= cap
        return out[:k].copy()

    def levels(self):
        m, s, p, n = C.c_double(), C.c_double(), C.c_double(), C.c_long()
        self.L.nfmo_levels(self.h, C.byref(m), C.byref(s), C.byref(p), C.byref(n))
        return m.value, s.value, p.value, n.value

    def squelch_open(self) -> bool:
        return bool(self.L.nfmo_squelch_open(self.h))

    def squelch_count(self) -> int:
        return self.L.nfmo_squelch_count(self.h)

    def probe(self) -> dict:
        out = np.zeros(len(PROBES), np.int64)
        self.L.nfmo_probe(self.h, out.ctypes.data)
        return dict(zip(PROBES, (int(v) for v in out)))

    def design(self):
        taps = np.zeros(16 * 128, np.float32)
        bp = np.zeros(151, np.float32)
        inc, lvl, gate = C.c_int(), C.c_float(), C.c_int()
        nt = self.L.nfmo_design(self.h, taps.ctypes.data, bp.ctypes.data, C.byref(inc), C.byref(lvl), C.byref(gate))
        return nt, taps[: 16 * nt].copy(), bp, inc.value, lvl.value, gate.value

    def close(self):
        if self.h:
            self.L.nfmo_destroy(self.h)
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
    elif kind == "const":                              # constant sample
        iq[0::2] = sig["i"]
        iq[1::2] = sig["q"]
    elif kind == "nfm":
        ph = _fm_phase(n, rate, sig.get("f0", 0.0), sig.get("dev", 2000.0), sig.get("fa", 1000.0))
        amp = _amp_runs(n, sig["runs"], sig["amps"]) if "runs" in sig else np.full(n, float(sig.get("amp", 8000.0)))
        sg = float(sig.get("noise", 20.0))
        iq[0::2] = _clip16(amp * np.cos(ph) + _gauss(seed, n, 3, sg))
        iq[1::2] = _clip16(amp * np.sin(ph) + _gauss(seed, n, 4, sg))
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
    head = [1, 0, 2, 31, 32, 33, 0, 1, 700]
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
    return (in_rate, nco_freq, audio_rate, d["rf"], d["af"], d["fmdev"], d["vol"], d["sq"], d["gate"], d["mute"])


def gate_samples(cfg) -> int:
    """m_squelchGate"""
    return (cfg[2] // 100) * cfg[8]


#: input runs (60 kS/s in, 48 kS/s audio: x 0.8) around gate 2400 / cap 4800 ...
BURST_RUNS_5 = [9000, 2000, 30000, 7000, 4000, 3500, 40000, 20000]
#: ... and around gate 480 / cap 960
BURST_RUNS_1 = [3000, 400, 9000, 700, 1000, 5000, 300, 900, 20000, 1100, 30000, 500]
#: the level-edge sample and squelch (see make_cases)
EDGE_IQ = (9703, 13007)
EDGE_SQ = -61.0399169921875
_EDGES = [1, 31, 32, 33, 2, 3, 5, 7, 11, 13, 255, 256, 257, 1023, 1025, 4099, 10007, 0, 1]


def make_cases() -> list[dict]:
    cases = []

    def add(name, cfg, sig, n, splits=None, seed=None):
        seed = len(cases) + 1 if seed is None else seed
        cases.append({"name": name, "cfg": cfg, "sig": sig, "n": n, "seed": seed, "splits": splits or _ragged(n, seed)})

    fm = lambda f0, **kw: dict({"kind": "nfm", "f0": f0, "dev": 2000.0, "fa": 1000.0, "amp": 8000.0}, **kw)
    add("default_60k", _cfg(60000, 48000, nco_freq=-3000), fm(3000.0), 90000)
    add("nondyadic_62500", _cfg(62500, 48000, nco_freq=1700), fm(-1700.0, fa=700.0), 80000)          # serial resampler schedule
    add("step1_48k", _cfg(48000, 48000), fm(0.0, fa=400.0), 60000)
    add("r96k_to_44k1", _cfg(96000, 44100, nco_freq=-12000), fm(12000.0, dev=2500.0), 120000)        # gate 2205, compensation != 1
    # squelch bursts: the amplitude alternates between 8000 and 30 (below the -30 dB level) over stretches shorter and longer
    # than the opening count (gate) and the counter's cap (2 * gate)
    add("burst_gate5", _cfg(60000, 48000, nco_freq=-3000), fm(3000.0, runs=BURST_RUNS_5, amps=[8000.0, 30.0]), sum(BURST_RUNS_5))
    add("burst_gate1", _cfg(60000, 48000, nco_freq=-3000, gate=1), fm(3000.0, runs=BURST_RUNS_1, amps=[8000.0, 30.0]), sum(BURST_RUNS_1))
    # gate 28 800 > the 24 000 entries of the delay line: readBack clamps
    add("gate60_clamped", _cfg(60000, 48000, nco_freq=-3000, gate=60), fm(3000.0), 120000)
    # (qint16) of a product outside the int16 range: 16 * dev / fm_deviation * volume = 64 000
    add("wrap_vol10", _cfg(60000, 48000, nco_freq=-3000, vol=10.0, fmdev=10), fm(3000.0, dev=4000.0), 60000)
    add("zero_gap", _cfg(60000, 48000, nco_freq=-3000), fm(3000.0, noise=0.0, zero_at=(40000, 200)), 70000)
    # the moving average within a few ulp of the level: a constant sample turned slowly by the NCO, the squelch found by search
    # on the oracle (tests/test_nfm_oracle.py::test_level_edge_case_straddles_the_level keeps it honest)
    add("level_edge", _cfg(48000, 48000, nco_freq=12, sq=EDGE_SQ, gate=1), {"kind": "const", "i": EDGE_IQ[0], "q": EDGE_IQ[1]}, 60000)
    add("audio_mute", _cfg(60000, 48000, nco_freq=-3000, mute=1), fm(3000.0), 60000)
    add("all_zero", _cfg(60000, 48000), {"kind": "zero"}, 60000)
    add("fullscale_noise", _cfg(60000, 48000), {"kind": "noise_full"}, 60000)
    add("wide_25k", _cfg(96000, 48000, nco_freq=7000, rf=25000.0, af=6000.0, fmdev=5000, sq=-450.0, gate=3), fm(-7000.0, dev=5000.0, fa=2500.0), 90000)
    add("splits_edges", _cfg(60000, 48000, nco_freq=-2345), fm(2345.0), 100000, splits=_EDGES + [100000 - sum(_EDGES)])
    add("one_long_feed", _cfg(60000, 48000, nco_freq=-2345), fm(2345.0), 100000, splits=[100000], seed=15)
    for c in cases:
        assert sum(c["splits"]) == c["n"], c["name"]
    return cases


CASES = make_cases()


def inputs(case: dict) -> np.ndarray:
    return signal(case["sig"], case["n"], case["cfg"][0], case["seed"])


def run_oracle(L: C.CDLL, case: dict, splits=None) -> dict:
    o = OracleNfm(L, case["cfg"])
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
    kind = str(rng.choice(["nfm", "burst", "noise_full", "zero", "nfm", "gap"]))
    f0 = float(rng.integers(-in_rate // 8, in_rate // 8))
    sig = {"kind": "nfm" if kind in ("burst", "gap") else kind, "f0": f0, "dev": float(rng.choice([500.0, 2000.0, 4000.0])), "fa": float(rng.integers(100, 3000)),
           "amp": float(rng.integers(50, 20000)), "noise": float(rng.integers(0, 50))}
    if kind == "burst":
        sig["runs"] = [int(v) for v in rng.integers(1, in_rate // 4, size=8)]
        sig["amps"] = [float(rng.integers(3000, 16000)), float(rng.integers(1, 200))]
    n = int(rng.integers(2000, 60000))
    if kind == "gap":
        sig["noise"] = 0.0
        sig["zero_at"] = (int(rng.integers(0, n)), int(rng.integers(1, 400)))
    cfg = (in_rate, -int(f0), audio, float(rng.choice([5000.0, 8330.0, 12500.0, 25000.0])), float(rng.choice([3000.0, 2400.0, 301.0, 6000.0])),
           int(rng.choice([2000, 5000, 10, 1234])), float(rng.choice([0.5, 2.0, 10.0])), float(rng.choice([-1000.0, -600.0, -400.0, -255.5, -100.0])),
           int(rng.choice([0, 1, 1, 2, 5, 5, 17, 60])), int(rng.random() < 0.1))
    splits, left = [], n
    while left > 0:
        m = min(left, int(rng.choice([0, 1, 2, 32, 33, int(rng.integers(1, 3000)), int(rng.integers(1, 30000))])))
        splits.append(m); left -= m
    return {"name": f"random{i}", "cfg": cfg, "sig": sig, "n": n, "seed": 1000 + i, "splits": splits}


#: the seed of random_cases(): the cases the `ref` test of tests/test_nfm_oracle.py proves against the reference
RANDOM_SEED = 20261017


def random_cases(count: int = 100) -> list[dict]:
    """the first `count` random cases, drawn in order from one generator"""
    rng = np.random.default_rng(RANDOM_SEED)
    return [random_case(rng, i) for i in range(count)]
