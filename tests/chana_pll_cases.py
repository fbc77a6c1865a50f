"""Cases of the ChannelAnalyzer bank with its PLL / FLL (sdrx_chanapll_*) and the ctypes face of tests/chana_pll_oracle.c, shared by
tests/test_chana_pll_oracle.py (CPU), tests/test_chana_pll_gpu.py and tests/golden/make_golden_chana_pll.py.

A case is tests/chana_cases.py's (configuration, signal, feed lengths) with three more configuration fields (pll, fll, psk_order)
and two more kinds of signal: a tone that steps to another frequency at sample `at` (sig has step2), and a constant (sig has
const).  All run at in_rate 48000 unless the Interpolator is what they are about; the tone sits at in_rate / 16 = 3000 Hz, so
nco_freq decides the offset the loop sees.  Sizes are those of tests/chana_cases.py."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from tests import chana_cases as cc
from tests import synth
from tests.wfm_cases import cut  # noqa: F401  (re-exported)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_SRC = os.path.join(ROOT, "tests", "chana_pll_oracle.c")
FIELDS = cc.FIELDS + ("pll", "fll", "psk_order")
SIGNAL, PLLOUT, AUTOCORR = 0, 1, 2
PROBES = ("sat_hi", "sat_lo", "turns_many", "lock_up", "lock_down", "big_arg", "arg_zero", "steps")


# ---------------------------------------------------------------- oracle
def build_oracle() -> C.CDLL:
    so = os.path.join(tempfile.mkdtemp(), "libchapo.so")
    subprocess.check_call(["cc", "-std=gnu11", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-fno-builtin", ORACLE_SRC, "-o", so, "-lm"])
    L = C.CDLL(so)
    L.chapo_create.restype = C.c_void_p
    L.chapo_create.argtypes = [C.c_int] * 14
    L.chapo_destroy.argtypes = [C.c_void_p]
    L.chapo_feed.restype = C.c_long
    L.chapo_feed.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_void_p, C.c_long]
    L.chapo_state.argtypes = [C.c_void_p, C.c_void_p]
    L.chapo_probe.argtypes = [C.c_void_p, C.c_void_p]
    return L


class OraclePll:
    def __init__(self, L: C.CDLL, cfg: dict):
        self.L = L
        self.h = L.chapo_create(*[int(cfg[f]) for f in FIELDS])
        assert self.h

    def feed(self, iq: np.ndarray) -> np.ndarray:
        iq = np.ascontiguousarray(iq, np.int16)
        n = iq.size // 2
        cap = n + 2048
        out = np.empty((cap, 2), np.int16)
        k = self.L.chapo_feed(self.h, iq.ctypes.data, n, out.ctypes.data, cap)
        assert k <= cap
        return out[:k].copy()

    def state(self) -> tuple:
        """(isPllLocked, bits of getPllFrequency, getPllDeltaPhase, getPllPhase, m_magsq)"""
        out = np.zeros(5, np.float64)
        self.L.chapo_state(self.h, out.ctypes.data)
        return int(out[0]), int(out[1]), int(out[2]), int(out[3]), float(out[4])

    def probe(self) -> dict:
        out = np.zeros(8, np.int64)
        self.L.chapo_probe(self.h, out.ctypes.data)
        return dict(zip(PROBES, (int(v) for v in out)))

    def close(self):
        if self.h:
            self.L.chapo_destroy(self.h)
            self.h = None

    __del__ = close


# ---------------------------------------------------------------- cases
def _cfg(in_rate, **kw):
    d = dict(cc.DEFAULT, pll=0, fll=0, psk_order=1); d.update(kw)
    d["in_rate"] = in_rate
    assert set(d) == set(FIELDS)
    return d


#: feed lengths 0, 1, 1023, 1024, 4097 and 3000: around the filter's blocks of 512 / 1024 and the 64 steps the walk stages at a time
_EDGES = [1, 0, 1023, 1024, 3000, 4097]


def make_cases() -> list[dict]:
    cases = []

    def add(name, cfg, sig, n, splits=None, seed=None):
        seed = len(cases) + 101 if seed is None else seed
        cases.append({"name": name, "cfg": cfg, "sig": sig, "n": n, "seed": seed, "splits": splits or cc._splits(n, _EDGES)})

    clean = dict(amp=30, tone=8000, step=1)                  # a tone at +3000 Hz, little noise
    noisy = dict(amp=6000, tone=3000, step=1)
    n6 = 6 * 1024 + 300
    halves = [512] * 12 + [300]                              # the state after every 512 inputs: locked, then not
    stepped = dict(clean, step2=15, at=3 * 1024 + 200)       # ... then at -3000 Hz, outside the filter behind nco_freq: noise is left
    # order 1: the loop sees +50 Hz and follows it; the phase estimate passes 2 pi again and again
    add("pll_above_usb", _cfg(48000, nco_freq=-2950, ssb=1, pll=1), clean, n6, splits=halves)
    add("pll_lock_lost_dsb", _cfg(48000, nco_freq=-2950, pll=1), stepped, n6, splits=halves)
    add("pll_below_lsb", _cfg(48000, nco_freq=2950, ssb=1, bandwidth=-5000, pll=1), dict(clean, step=15), n6)      # -50 Hz, and the swap
    add("pll_rrc", _cfg(48000, nco_freq=-3010, rrc=1, bandwidth=6000, pll=1), clean, n6)
    # PSK orders: the multiplied phase error wraps more than once under noise; the lock counter goes up on the tone, down after the step
    add("psk2_span3", _cfg(48000, nco_freq=-2998, span_log2=3, pll=1, psk_order=2), dict(stepped, at=4 * 1024), 3 * n6, splits=cc._splits(3 * n6, _EDGES))
    add("psk4_noisy", _cfg(48000, nco_freq=-2990, pll=1, psk_order=4), noisy, n6)
    add("psk16_lsb", _cfg(48000, nco_freq=3002, ssb=1, bandwidth=-5000, pll=1, psk_order=16), dict(noisy, step=15), n6)
    # 256 samples per group: the loops run at 187 S/s, m_lockTime is 1
    add("pll_span8", _cfg(48000, nco_freq=-3000, ssb=1, span_log2=8, pll=1), clean, 6 * 512 + 100, splits=[1, 511, 100, 412, 300, 300, 600, 512, 436])
    add("pll_down_96k_37k", _cfg(96000, down_sample=1, down_sample_rate=37000, ssb=1, nco_freq=-5990, span_log2=2, pll=1, psk_order=2), clean, 8000,
        splits=cc._splits(8000, [1, 0, 700, 3, 2000, 1300]))
    # the three input types
    add("in1_pll", _cfg(48000, nco_freq=-2950, pll=1, input_type=PLLOUT), clean, n6)
    add("in1_unfed", _cfg(48000, input_type=PLLOUT), clean, 2 * 1024 + 100)
    add("in1_fll_only_lsb", _cfg(48000, ssb=1, bandwidth=-5000, fll=1, input_type=PLLOUT), clean, 2 * 1024 + 100)
    nc = 2 * 4096 + 100
    add("corr_pll", _cfg(48000, nco_freq=-2950, pll=1, input_type=AUTOCORR), dict(amp=3, tone=20, step=1), nc + 1024,
        splits=cc._splits(nc + 1024, [1, 4095, 1, 4096, 0, 4097]))
    # FreqLockComplex: its phase is never wrapped and passes 120 within a few hundred samples at 3000 Hz
    add("fll_pll", _cfg(48000, pll=1, fll=1, bandwidth=8000), clean, n6)
    add("fll_pll_in1_lsb", _cfg(48000, ssb=1, bandwidth=-8000, pll=1, fll=1, input_type=PLLOUT), dict(clean, step=15), n6)
    add("fll_only", _cfg(48000, fll=1), clean, 2 * 1024 + 100)
    # arg(0), and the most negative input
    add("silence_pll", _cfg(48000, pll=1, psk_order=4), dict(amp=0, tone=0, step=1), 3 * 1024 + 100)
    add("silence_fll", _cfg(48000, pll=1, fll=1), dict(amp=0, tone=0, step=1), 3 * 1024 + 100)
    add("minus_32768", _cfg(48000, pll=1), dict(const=-32768), n6)
    add("minus_32768_fll", _cfg(48000, nco_freq=-700, pll=1, fll=1), dict(const=-32768), n6)
    for c in cases:
        assert sum(c["splits"]) == c["n"], c["name"]
    return cases


CASES = make_cases()


def inputs(case: dict) -> np.ndarray:
    s, n = case["sig"], case["n"]
    if "const" in s:
        return np.full(2 * n, s["const"], np.int16)
    x = synth.mix(n, case["seed"], s["amp"], s["tone"], s["step"])
    if "step2" in s:
        y = synth.mix(n, case["seed"] + 1000, s["amp"], s["tone"], s["step2"])
        x = np.concatenate([x[: 2 * s["at"]], y[2 * s["at"]:]])
    return x


def run_oracle(L: C.CDLL, cfg: dict, feeds) -> dict:
    """feeds: the input arrays, one per feed.  Samples and state after every feed, and the probes"""
    o = OraclePll(L, cfg)
    out, states = [], []
    for x in feeds:
        out.append(o.feed(x))
        states.append(o.state())
    res = {"out": out, "states": states, "probe": o.probe()}
    o.close()
    return res


def random_cfg(rng) -> dict:
    """a configuration the object allows, PLL / FLL / input type in every combination"""
    down = int(rng.integers(0, 4) == 0)
    in_rate = int(rng.choice([48000, 50000, 96000, 12345]))
    ssb, rrc = int(rng.integers(0, 2)), int(rng.integers(0, 2))
    return _cfg(in_rate, nco_freq=int(rng.integers(-in_rate // 8, in_rate // 8)), down_sample=down,
                down_sample_rate=int(rng.integers(in_rate // 4, in_rate + 1)) if down else int(rng.integers(0, 2)) * 24000,
                bandwidth=int(rng.choice([-1, 1])) * int(rng.integers(50, in_rate // 4)), low_cutoff=int(rng.integers(0, 600)),
                span_log2=int(rng.choice([0, 0, 1, 2, 3, 5, 8])), ssb=ssb, rrc=rrc, rrc_rolloff=int(rng.integers(0, 101)),
                input_type=int(rng.choice([SIGNAL, SIGNAL, PLLOUT, AUTOCORR])), pll=int(rng.integers(0, 4) != 0), fll=int(rng.integers(0, 3) == 0),
                psk_order=int(rng.choice([1, 1, 2, 3, 4, 8, 16, 31])))


def random_signal(rng, n: int) -> np.ndarray:
    amp, tone = int(rng.choice([0, 3, 300, 20000])), int(rng.choice([0, 20, 8000, 30000]))
    return synth.mix(n, int(rng.integers(1, 1 << 20)), amp, tone, int(rng.choice([1, 15])))
