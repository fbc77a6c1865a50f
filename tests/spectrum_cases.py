"""Cases of the spectrum sink (sdrx_spectrum_*) and the ctypes face of tests/spectrum_oracle.c, shared by
tests/test_spectrum_oracle.py (CPU) and tests/test_spectrum_gpu.py.

A case is a start configuration and a list of steps:
    ("feed", n_cplx, positive_only, signal)   signal: "noise" (full-scale uniform), "tone", "min" (all -32768), "zero"
    ("configure", cfg)                         handleConfigure mid-stream
cfg = (fft_size, overlap_percent, avg_nb, avg_mode, window, linear)."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_SRC = os.path.join(ROOT, "tests", "spectrum_oracle.c")

BH, RECT = 1, 5
NONE, MOVING, FIXED = 0, 1, 2


def build_oracle() -> C.CDLL:
    so = os.path.join(tempfile.mkdtemp(), "libspo.so")
    subprocess.check_call(["cc", "-std=gnu11", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", ORACLE_SRC, "-o", so, "-lm"])
    L = C.CDLL(so)
    L.spo_create.restype = C.c_void_p
    L.spo_create.argtypes = [C.c_float]
    L.spo_destroy.argtypes = [C.c_void_p]
    L.spo_configure.restype = C.c_int
    L.spo_configure.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_uint, C.c_int, C.c_int, C.c_int]
    L.spo_feed.restype = C.c_long
    L.spo_feed.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_int, C.c_void_p, C.c_long]
    L.spo_window.restype = C.c_int
    L.spo_window.argtypes = [C.c_void_p, C.c_void_p]
    L.spo_set_log2_double.argtypes = [C.c_void_p, C.c_int]
    return L


class OracleSpectrum:
    def __init__(self, L: C.CDLL, cfg, scalef: float = 32768.0, log2_double: bool = False):
        self.L = L
        self.h = L.spo_create(scalef)
        L.spo_set_log2_double(self.h, int(log2_double))
        self.n = 1024
        self.configure(cfg)

    def configure(self, cfg):
        if self.L.spo_configure(self.h, *[int(v) for v in cfg]) != 0:
            raise ValueError(f"rejected configuration {cfg}")
        self.n = min(max(int(cfg[0]), 64), 4096)
        self.s = self.n - 2 * (self.n * min(max(int(cfg[1]), 0), 100) // 100)     # fresh samples per frame

    def feed(self, iq: np.ndarray, positive_only: bool) -> np.ndarray:
        iq = np.ascontiguousarray(iq, np.int16)
        n = iq.size // 2
        cap = n // self.s + 2                  # a feed completes at most n / S + 1 frames
        out = np.empty((cap, self.n), np.float32)
        k = self.L.spo_feed(self.h, iq.ctypes.data, n, int(positive_only), out.ctypes.data, cap)
        assert k <= cap
        return out[:k].copy()

    def window(self) -> np.ndarray:
        out = np.empty(4096, np.float32)
        n = self.L.spo_window(self.h, out.ctypes.data)
        return out[:n].copy()

    def close(self):
        if self.h:
            self.L.spo_destroy(self.h)
            self.h = None

    __del__ = close


def signal(kind: str, n: int, rng: np.random.Generator) -> np.ndarray:
    if kind == "noise":
        return rng.integers(-32768, 32768, size=2 * n, dtype=np.int64).astype(np.int16)
    if kind == "min":
        return np.full(2 * n, -32768, np.int16)
    if kind == "zero":
        return np.zeros(2 * n, np.int16)
    if kind == "tone":
        t = np.arange(n)
        ph = 2 * np.pi * 0.1234 * t
        iq = np.empty(2 * n, np.int16)
        iq[0::2] = np.round(20000 * np.cos(ph) + rng.normal(0, 30, n)).astype(np.int16)
        iq[1::2] = np.round(20000 * np.sin(ph) + rng.normal(0, 30, n)).astype(np.int16)
        return iq
    raise ValueError(kind)


def _feeds(n_fft: int, total_frames: float, po=False, sig="noise", seed=0):
    """ragged feed lengths adding up to about total_frames * n_fft samples: 1, N-1, N+1, sub-frame runs and big spans"""
    rng = np.random.default_rng(seed)
    steps = [("feed", 1, po, sig), ("feed", n_fft - 1, po, sig), ("feed", n_fft + 1, po, sig)]
    left = int(total_frames * n_fft)
    while left > 0:
        k = int(rng.choice([rng.integers(1, max(2, n_fft // 3)), rng.integers(n_fft // 2, 3 * n_fft), rng.integers(5 * n_fft, 12 * n_fft)]))
        k = min(k, left)
        steps.append(("feed", k, po, sig))
        left -= k
    return steps


def make_cases() -> list[dict]:
    cases = []
    for w in range(6):
        cases.append({"name": f"win{w}", "cfg": (1024, 0, 0, NONE, w, 0), "steps": _feeds(1024, 6, seed=w)})
    for n in (64, 256, 1024, 2048, 4096):
        for ov in (0, 10, 25, 49):
            cases.append({"name": f"n{n}_ov{ov}", "cfg": (n, ov, 0, NONE, BH, 0), "steps": _feeds(n, 8, seed=n + ov)})
    for mode in (MOVING, FIXED):
        for nb in (1, 3, 10):
            for lin in (0, 1):
                for po in (False, True):
                    cases.append({"name": f"avg{mode}_nb{nb}_lin{lin}_po{int(po)}", "cfg": (256, 25, nb, mode, BH, lin),
                                  "steps": _feeds(256, 40, po=po, seed=100 * mode + 10 * nb + 2 * lin + po)})
    for lin in (0, 1):
        for po in (False, True):
            cases.append({"name": f"none_lin{lin}_po{int(po)}", "cfg": (512, 10, 0, NONE, 3, lin), "steps": _feeds(512, 10, po=po, seed=7 + lin + po)})
    # positive_only toggling between feeds while averaging (the upper bins' state is left alone)
    st = _feeds(128, 12, po=False, seed=31)
    st = [(s[0], s[1], bool(i % 2), s[3]) for i, s in enumerate(st)]
    cases.append({"name": "moving_po_toggle", "cfg": (128, 10, 3, MOVING, 4, 0), "steps": st})
    cases.append({"name": "fixed_po_toggle", "cfg": (128, 10, 3, FIXED, 4, 0), "steps": st})
    # stale data: 4096/0 % -> 1024/25 % with a partial frame pending across the configure, then more changes
    steps = [("feed", 4096 * 3 + 1500, False, "tone"), ("configure", (1024, 25, 0, NONE, BH, 0))]
    steps += _feeds(1024, 10, sig="tone", seed=5)
    steps += [("feed", 700, False, "noise"), ("configure", (2048, 49, 3, MOVING, 2, 0))] + _feeds(2048, 6, seed=6)
    steps += [("feed", 100, False, "noise"), ("configure", (64, 40, 10, FIXED, 0, 1))] + _feeds(64, 40, seed=8)
    cases.append({"name": "reconfigure_stale", "cfg": (4096, 0, 0, NONE, BH, 0), "steps": steps})
    steps = [("feed", 3000, False, "noise"), ("configure", (256, 25, 0, NONE, RECT, 1))] + _feeds(256, 10, seed=9)
    steps += [("configure", (4096, 30, 0, NONE, BH, 0))] + _feeds(4096, 4, seed=10)
    cases.append({"name": "reconfigure_grow", "cfg": (1024, 10, 0, NONE, BH, 0), "steps": steps})
    for sig in ("min", "zero"):
        for lin in (0, 1):
            cases.append({"name": f"{sig}_lin{lin}", "cfg": (1024, 25, 3, MOVING if lin else NONE, BH, lin), "steps": _feeds(1024, 6, sig=sig, seed=11)})
            cases.append({"name": f"{sig}_fixed_lin{lin}", "cfg": (256, 0, 3, FIXED, RECT, lin), "steps": _feeds(256, 8, sig=sig, seed=12)})
    return cases


CASES = make_cases()


def inputs(case: dict, seed: int = 1234):
    """the int16 span of every feed step (None for configure steps)"""
    rng = np.random.default_rng(seed)
    return [signal(s[3], s[1], rng) if s[0] == "feed" else None for s in case["steps"]]


def run_oracle(L: C.CDLL, case: dict, log2_double: bool = False):
    """per step: frames emitted by a feed (array (k, N)), or the window table after a configure"""
    o = OracleSpectrum(L, case["cfg"], log2_double=log2_double)
    res = [("window", o.window())]
    for s, iq in zip(case["steps"], inputs(case)):
        if s[0] == "feed":
            res.append(("frames", o.feed(iq, s[2])))
        else:
            o.configure(s[1])
            res.append(("window", o.window()))
    o.close()
    return res


def ulp_diff(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """distance in float32 ulps (equal infinities: 0; NaN or unequal infinities: huge)"""
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    ia = a.view(np.int32).astype(np.int64)
    ib = b.view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia)
    ib = np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    d = np.abs(ia - ib)
    d = np.where(a == b, 0, d)
    d = np.where(np.isinf(a) | np.isinf(b), np.where(a == b, 0, 1 << 40), d)
    return d
