"""Cases of the ChannelAnalyzer bank (sdrx_chana_*) and the ctypes face of tests/chana_oracle.c, shared by
tests/test_chana_oracle.py (CPU) and tests/test_chana_gpu.py.

A case is an analyzer configuration, a signal at the channel rate and the lengths of the feeds it is cut into:
    cfg = dict(in_rate, nco_freq, down_sample, down_sample_rate, bandwidth, low_cutoff, span_log2, ssb, rrc, rrc_rolloff, input_type)
    sig = dict(amp, tone, step)     tests/synth.mix: uniform noise of +-amp plus a tone of amplitude `tone` at step * rate / 16

Each case is the smallest shape at which its path can go wrong: a signal case is a few blocks of 1024 filtered samples, an
autocorrelation case two blocks of 4096 calls and a tail that ends inside the third."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from tests import synth
from tests.wfm_cases import cut  # noqa: F401  (re-exported)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_SRC = os.path.join(ROOT, "tests", "chana_oracle.c")

FIELDS = ("in_rate", "nco_freq", "down_sample", "down_sample_rate", "bandwidth", "low_cutoff", "span_log2", "ssb", "rrc", "rrc_rolloff", "input_type")
#: ChannelAnalyzerSettings::resetToDefaults
DEFAULT = dict(nco_freq=0, down_sample=0, down_sample_rate=0, bandwidth=5000, low_cutoff=300, span_log2=0, ssb=0, rrc=0, rrc_rolloff=35, input_type=0)
SIGNAL, AUTOCORR = 0, 2


# ---------------------------------------------------------------- oracle
def build_oracle() -> C.CDLL:
    so = os.path.join(tempfile.mkdtemp(), "libchao.so")
    subprocess.check_call(["cc", "-std=gnu11", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", ORACLE_SRC, "-o", so, "-lm"])
    L = C.CDLL(so)
    L.chao_create.restype = C.c_void_p
    L.chao_create.argtypes = [C.c_int] * 11
    L.chao_destroy.argtypes = [C.c_void_p]
    L.chao_feed.restype = C.c_long
    L.chao_feed.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_void_p, C.c_long]
    L.chao_magsq.restype = C.c_double
    L.chao_magsq.argtypes = [C.c_void_p]
    L.chao_seek.argtypes = [C.c_void_p, C.c_uint64]
    L.chao_state.argtypes = [C.c_void_p, C.c_void_p]
    L.chao_design.restype = C.c_int
    L.chao_design.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_float)]
    return L


class OracleChana:
    def __init__(self, L: C.CDLL, cfg: dict):
        self.L = L
        self.cfg = cfg
        self.h = L.chao_create(*[int(cfg[f]) for f in FIELDS])
        assert self.h

    def feed(self, iq: np.ndarray) -> np.ndarray:
        """the Samples of this feed, [m, 2] of re, im"""
        iq = np.ascontiguousarray(iq, np.int16)
        n = iq.size // 2
        cap = n + 2048                            # at most one filtered sample per input, plus what the filter held back
        out = np.empty((cap, 2), np.int16)
        k = self.L.chao_feed(self.h, iq.ctypes.data, n, out.ctypes.data, cap)
        assert k <= cap
        return out[:k].copy()

    def magsq(self) -> float:
        return self.L.chao_magsq(self.h)

    def seek(self, filtered_samples: int):
        self.L.chao_seek(self.h, filtered_samples)

    def state(self) -> tuple:
        """(m_undersampleCount's low 32 bits, fftcorr's inptrA, blocks it completed, filtered samples)"""
        out = np.zeros(4, np.float64)
        self.L.chao_state(self.h, out.ctypes.data)
        return tuple(int(v) for v in out)

    def design(self):
        taps, filt = np.zeros(16 * 256, np.float32), np.zeros(4096, np.float32)
        inc = C.c_float()
        nt = self.L.chao_design(self.h, taps.ctypes.data, filt.ctypes.data, C.byref(inc))
        return nt, taps[: 16 * nt].copy(), filt, inc.value

    def close(self):
        if self.h:
            self.L.chao_destroy(self.h)
            self.h = None

    __del__ = close


# ---------------------------------------------------------------- cases
def _cfg(in_rate, **kw):
    d = dict(DEFAULT); d.update(kw)
    d["in_rate"] = in_rate
    assert set(d) == set(FIELDS)
    return d


#: feed lengths around the filter's blocks of 512 and 1024 and fftcorr's of 4096: empty and one-sample feeds included
_EDGES = [1, 0, 511, 1, 512, 513, 2, 1023, 1025, 0, 1]


def _splits(n, head=_EDGES):
    out, left = [], n
    for m in head:
        m = min(m, left)
        out.append(m); left -= m
    if left:
        out.append(left)
    return out


def make_cases() -> list[dict]:
    cases = []

    def add(name, cfg, sig, n, splits=None, seed=None):
        seed = len(cases) + 1 if seed is None else seed
        cases.append({"name": name, "cfg": cfg, "sig": sig, "n": n, "seed": seed, "splits": splits or _splits(n)})

    up = dict(amp=300, tone=8000, step=1)          # a tone at +rate/16 over noise
    down = dict(amp=300, tone=8000, step=15)       # at -rate/16
    n4 = 4 * 1024 + 300                            # four blocks of 1024 (eight of 512) and a held-back rest
    add("dsb_default", _cfg(48000), up, n4)
    add("usb", _cfg(48000, nco_freq=-1000, ssb=1), up, n4)
    add("lsb_swap", _cfg(48000, nco_freq=1000, ssb=1, bandwidth=-5000), down, n4)
    add("dsb_negative_bandwidth", _cfg(48000, bandwidth=-5000), up, n4, seed=1)        # dsb_default's signal: no swap, the same Samples
    add("band_reject", _cfg(48000, ssb=1, bandwidth=2000, low_cutoff=6000), up, n4)
    add("band_clamp", _cfg(48000, ssb=1, bandwidth=-60, low_cutoff=-20), down, n4)
    add("nco_fractional", _cfg(50000, nco_freq=-1234, ssb=1), up, n4)                  # NCOF's increment is no integer: the float phase rounds
    add("nco_negative", _cfg(50000, nco_freq=4321), up, n4)
    for a in (0, 35, 100):
        add(f"rrc_{a}", _cfg(48000, rrc=1, rrc_rolloff=a, bandwidth=6000), up, n4)
    add("span0", _cfg(48000, ssb=1, span_log2=0), up, n4)
    add("span1", _cfg(48000, ssb=1, span_log2=1), up, n4)
    add("span3", _cfg(48000, span_log2=3), up, n4)
    # 256 samples per group, blocks of 512: a group stays open across feeds that emit nothing
    add("span8", _cfg(48000, ssb=1, span_log2=8), up, 6 * 512 + 100, splits=[1, 511, 100, 412, 300, 300, 600, 512, 436])
    add("down_48k_12k", _cfg(48000, down_sample=1, down_sample_rate=12000, bandwidth=2500, span_log2=1), up, 4 * 4 * 1024 + 500)
    add("down_96k_37k", _cfg(96000, down_sample=1, down_sample_rate=37000, ssb=1, nco_freq=-5000, span_log2=2), dict(amp=300, tone=8000, step=1),
        8000, splits=_splits(8000, [1, 0, 700, 3, 2000, 1300]))
    add("down_step1", _cfg(48000, down_sample=1, down_sample_rate=48000), up, n4, seed=1)      # beside dsb_default: same rate, they differ
    add("down_rrc_negative", _cfg(48000, down_sample=1, down_sample_rate=24000, rrc=1, bandwidth=-3000, rrc_rolloff=50), up, 2 * 2 * 1024 + 100)
    # autocorrelation: 2 * 4096 calls and ~100 more
    quiet = dict(amp=3, tone=20, step=1)
    loud = dict(amp=20000, tone=12000, step=1)
    nc = 2 * 4096 + 100
    acs = [1, 4095, 1, 4096, 0, 4097]              # the calls that complete a block fall on a feed's last, first and inner samples
    add("corr_dsb_quiet", _cfg(48000, input_type=AUTOCORR), quiet, nc + 1024, splits=_splits(nc + 1024, acs))
    add("corr_usb_quiet", _cfg(48000, ssb=1, input_type=AUTOCORR), quiet, nc + 512)
    add("corr_lsb_quiet", _cfg(48000, ssb=1, bandwidth=-5000, input_type=AUTOCORR), dict(amp=3, tone=20, step=15), nc + 512, splits=_splits(nc + 512, acs))
    add("corr_dsb_loud", _cfg(48000, input_type=AUTOCORR), loud, nc + 1024)
    add("corr_lsb_loud", _cfg(48000, ssb=1, bandwidth=-5000, input_type=AUTOCORR), dict(amp=20000, tone=12000, step=15), nc + 512, splits=_splits(nc + 512, acs))
    add("corr_span2", _cfg(48000, ssb=1, span_log2=2, input_type=AUTOCORR), quiet, 4 * nc + 512, splits=_splits(4 * nc + 512, [4 * 4096, 3, 4 * 4096 - 3, 1]))
    add("corr_rrc_down", _cfg(96000, down_sample=1, down_sample_rate=48000, rrc=1, rrc_rolloff=35, input_type=AUTOCORR), quiet, 2 * nc + 2048)
    for c in cases:
        assert sum(c["splits"]) == c["n"], c["name"]
    return cases


CASES = make_cases()


def inputs(case: dict) -> np.ndarray:
    s = case["sig"]
    return synth.mix(case["n"], case["seed"], s["amp"], s["tone"], s["step"])


def run_oracle(L: C.CDLL, case: dict, splits=None) -> dict:
    o = OracleChana(L, case["cfg"])
    feeds = [o.feed(x) for x in cut(inputs(case), splits or case["splits"])]
    res = {"out": feeds, "magsq": o.magsq(), "state": o.state(), "design": o.design()}
    o.close()
    return res
