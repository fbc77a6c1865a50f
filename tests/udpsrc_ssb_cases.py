"""Cases of the UDPSrc bank's SSB formats 4 .. 7 (sdrx_udpsrc_create_ex with SDRX_UDPSRC_SSB_FORMATS) and the ctypes face of
tests/udpsrc_ssb_oracle.c, shared by tests/test_udpsrc_ssb_oracle.py (CPU), tests/test_udpsrc_ssb_gpu.py and the golden recorder
tests/golden/make_golden_udpsrc_ssb.py.  The cfg tuple, the signals and `cut` are tests/udpsrc_cases.py's.

Shapes: 48000 in; 8000, 11025.5 and 48000 out; at most about 4000 resampled samples per case, i.e. up to 15 blocks of 256.
For these formats m_squelchGate is rate * 0.05 (400 samples at 8000) whatever squelch_gate says, and squelch_gate only sets
the release (80 samples per unit at 8000)."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from tests import udpsrc_cases as uc
from tests.udpsrc_cases import cut, signal  # noqa: F401  (re-exported)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_SRC = os.path.join(ROOT, "tests", "udpsrc_ssb_oracle.c")

LSB, USB, LSB_MONO, USB_MONO = 4, 5, 6, 7
FORMATS = (LSB, USB, LSB_MONO, USB_MONO)
#: numpy base type and components of one payload element
PAYLOAD = {LSB: (np.int16, 2), USB: (np.int16, 2), LSB_MONO: (np.int16, 1), USB_MONO: (np.int16, 1)}
PROBES = ("blocks", "blocks_open", "flips_in_block", "nan_blocks", "wraps", "past_int32")
H = 256


def elem_bytes(fmt: int) -> int:
    t, k = PAYLOAD[fmt]
    return np.dtype(t).itemsize * k


def as_elements(fmt: int, raw: bytes) -> np.ndarray:
    t, k = PAYLOAD[fmt]
    a = np.frombuffer(raw, t)
    return a.reshape(-1, 2).copy() if k == 2 else a.copy()


# ---------------------------------------------------------------- oracle
def build_oracle() -> C.CDLL:
    so = os.path.join(tempfile.mkdtemp(), "libudso.so")
    subprocess.check_call(["cc", "-std=gnu11", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-w", ORACLE_SRC, "-o", so, "-lm"])
    L = C.CDLL(so)
    L.udso_create.restype = C.c_void_p
    L.udso_create.argtypes = [C.c_int, C.c_int, C.c_float, C.c_int, C.c_float, C.c_int, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int]
    L.udso_destroy.argtypes = [C.c_void_p]
    L.udso_feed.restype = C.c_long
    L.udso_feed.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_void_p, C.c_long, C.c_void_p, C.POINTER(C.c_long)]
    L.udso_state.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_void_p]
    L.udso_last_open.restype = C.c_long
    L.udso_last_open.argtypes = [C.c_void_p, C.c_void_p, C.c_long]
    L.udso_filter.argtypes = [C.c_void_p, C.c_void_p]
    L.udso_design.argtypes = [C.c_void_p, C.c_void_p]
    L.udso_probe.argtypes = [C.c_void_p, C.c_void_p]
    return L


class OracleSsb:
    def __init__(self, L: C.CDLL, cfg):
        self.L, self.cfg, self.fmt = L, cfg, int(cfg[3])
        self.h = L.udso_create(int(cfg[0]), int(cfg[1]), float(cfg[2]), int(cfg[3]), float(cfg[4]), int(cfg[5]), float(cfg[6]), int(cfg[7]),
                               int(cfg[8]), int(cfg[9]), int(cfg[10]))
        assert self.h

    def feed(self, iq: np.ndarray):
        """(payload elements, spectrum Samples [k, 2]) of one feed"""
        iq = np.ascontiguousarray(iq, np.int16)
        n = iq.size // 2
        cap = 2 * n + H + 16                    # every input can give a raw element and takes part in one block
        out = np.zeros(cap * elem_bytes(self.fmt), np.uint8)
        spec = np.empty((n + 16, 2), np.int16)
        npay = C.c_long()
        k = self.L.udso_feed(self.h, iq.ctypes.data, n, out.ctypes.data, cap, spec.ctypes.data, C.byref(npay))
        assert npay.value <= cap
        return as_elements(self.fmt, out[: npay.value * elem_bytes(self.fmt)].tobytes()), spec[:k].copy()

    def last_open(self) -> np.ndarray:
        out = np.zeros(1 << 16, np.uint8)
        n = self.L.udso_last_open(self.h, out.ctypes.data, out.size)
        return out[:n].astype(bool)

    def state(self) -> dict:
        m = C.c_double()
        st = np.zeros(7, np.int64)
        self.L.udso_state(self.h, C.byref(m), st.ctypes.data)
        return {"in_magsq": m.value, "open": bool(st[0]), "open_count": int(st[1]), "close_count": int(st[2]), "resampled": int(st[3]),
                "pending": int(st[4]), "blocks": int(st[5]), "total": int(st[6])}

    def filter(self) -> np.ndarray:
        out = np.zeros(1024, np.float32)
        self.L.udso_filter(self.h, out.ctypes.data)
        return out

    def design(self) -> dict:
        v = np.zeros(2, np.int32)
        self.L.udso_design(self.h, v.ctypes.data)
        return {"gate": int(v[0]), "release": int(v[1])}

    def probe(self) -> dict:
        out = np.zeros(len(PROBES), np.int64)
        self.L.udso_probe(self.h, out.ctypes.data)
        return dict(zip(PROBES, (int(v) for v in out)))

    def close(self):
        if self.h:
            self.L.udso_destroy(self.h)
            self.h = None

    __del__ = close


# ---------------------------------------------------------------- cases
DEFAULT = dict(fmt=LSB, rf=5000.0, fmdev=2500, gain=1.0, sqdb=-60, gate=1, enabled=1, agc=0)


def _cfg(rate, nco_freq=0, in_rate=48000, **kw):
    d = dict(DEFAULT); d.update(kw)
    return (in_rate, nco_freq, float(rate), d["fmt"], d["rf"], d["fmdev"], d["gain"], d["sqdb"], d["gate"], d["enabled"], d["agc"])


#: input runs at 48000 in / 8000 out around the gate of 400 and a release of 80 output samples: the squelch opens near output
#: sample 400 + the average's lag, closes near 750 + 80, opens near 1000 + 400 and closes near 2000 + 80: none at a multiple of 256
BURST_RUNS = [4500, 1500, 6000, 3000]
#: feeds of 48000 -> 8000 (6 inputs per output, the first output with the sixth input) that yield 0, 1, 0 (a zero-length feed),
#: 255, 256, 257 and 3 x 256 resampled samples, then 5 inputs that yield none and the rest
YIELD_SPLITS = [5, 1, 0, 6 * 255, 6 * 256, 6 * 257, 6 * 768, 5]
YIELDS = [0, 1, 0, 255, 256, 257, 768, 0]
#: format 4 across feed boundaries that fall mid-block: 100, 300, 156 (which completes block 2 exactly), 1, 255, 700 outputs
INTERLEAVE_SPLITS = [600, 1800, 936, 6, 1530, 4200]


def make_cases() -> list[dict]:
    cases = []

    def add(name, cfg, sig, n, splits=None, seed=None):
        seed = len(cases) + 101 if seed is None else seed
        if splits is not None and sum(splits) < n:
            splits = list(splits) + [n - sum(splits)]
        cases.append({"name": name, "cfg": cfg, "sig": sig, "n": n, "seed": seed, "splits": splits or uc._nc._ragged(n, seed)})

    fm = lambda f0, **kw: dict({"kind": "nfm", "f0": f0, "dev": 2000.0, "fa": 700.0, "amp": 8000.0}, **kw)
    am = lambda f0, **kw: dict({"kind": "am", "f0": f0, "fa": 700.0, "amp": 8000.0}, **kw)
    on_off = [8000.0, 3.0]
    burst = lambda f0: fm(f0, runs=BURST_RUNS, amps=on_off)
    nb = sum(BURST_RUNS)
    # each format over a squelch that flips inside blocks in both directions (item 8), AGC off and on
    add("lsb_burst", _cfg(8000, nco_freq=-1000, fmt=LSB), burst(400.0), nb)
    add("usb_burst", _cfg(8000, nco_freq=-1000, fmt=USB), burst(1600.0), nb)
    add("lsbmono_burst_gate0", _cfg(8000, fmt=LSB_MONO, gate=0), burst(-900.0), nb)               # release 0 behind a gate of 400 (item 7)
    add("usbmono_burst", _cfg(8000, fmt=USB_MONO, gate=2), burst(700.0), nb)
    agc_runs = [4000, 4000, 4000, 1000, 3000, 300, 3700]
    agc_sig = lambda **kw: am(500.0, runs=agc_runs, amps=[8000.0, 40.0], **kw)
    add("lsb_agc_cross", _cfg(8000, fmt=LSB, sqdb=-20, agc=1, enabled=0), agc_sig(), sum(agc_runs))
    add("usb_agc_squelched", _cfg(8000, fmt=USB, sqdb=-30, agc=1), am(900.0, runs=[6000, 5000, 500, 4000, 4500], amps=[8000.0, 20.0]), 20000)
    add("lsbmono_agc", _cfg(11025.5, fmt=LSB_MONO, sqdb=-20, agc=1, enabled=0, gain=0.5), agc_sig(fa=400.0), sum(agc_runs))
    add("usbmono_agc_float_rate", _cfg(11025.5, fmt=USB_MONO, agc=1, gate=5), burst(1200.0), nb)
    # settings far from the 12500 / 48000 the filter was designed for: the design must not move (item 1)
    add("usb_wild_settings", _cfg(48000, fmt=USB, rf=1300.0, gate=1), fm(2000.0, runs=[1500, 500, 2000], amps=on_off), 4000)
    add("lsbmono_wild_settings", _cfg(8000, fmt=LSB_MONO, rf=100.0, enabled=0), fm(-300.0), 9000)
    # format 4's interleave across feed boundaries mid-block (item 9)
    add("lsb_interleave", _cfg(8000, fmt=LSB, enabled=0, gain=2.0), fm(-1200.0), sum(INTERLEAVE_SPLITS), splits=INTERLEAVE_SPLITS)
    # conversions: a gain that wraps int16, one past int32 (item 10)
    # (a deviation of 100 Hz keeps the carrier inside the filter's 1 kHz at this rate, so the sideband has the full amplitude)
    add("lsb_gain_wraps", _cfg(8000, fmt=LSB, gain=10.0, enabled=0), fm(-500.0, amp=9000.0, dev=100.0), 9000)
    add("usbmono_gain_wraps", _cfg(8000, fmt=USB_MONO, gain=-7.5, enabled=0), fm(500.0, amp=12000.0, dev=100.0), 9000)
    add("usb_gain_past_int32", _cfg(8000, fmt=USB, gain=1.0e6, enabled=0), fm(500.0, amp=12000.0, dev=100.0), 6000)
    add("lsbmono_gain_past_int32", _cfg(8000, fmt=LSB_MONO, gain=-3.0e6, enabled=0), fm(-500.0, amp=12000.0, dev=100.0), 6000)
    # silence with the AGC on: NaN blocks, payload 0 (item 11); and with it off
    # (squelch_gate 17 keeps MagAGC's factor at inf for 1360 samples, well past the 400 after which the disabled squelch opens)
    add("usb_agc_silence", _cfg(8000, fmt=USB, agc=1, enabled=0, gate=17), {"kind": "zero"}, 9000)
    add("lsb_agc_silence", _cfg(8000, fmt=LSB, agc=1, enabled=0, gate=17), {"kind": "zero"}, 9000)
    add("lsbmono_silence", _cfg(8000, fmt=LSB_MONO, enabled=0), {"kind": "zero"}, 6000)
    # feeds yielding 0, 1, 255, 256, 257 and 3 x 256 resampled samples and a zero-length feed
    ny = sum(YIELD_SPLITS) + 1201
    add("lsb_feed_yields", _cfg(8000, fmt=LSB, enabled=0), fm(-800.0), ny, splits=YIELD_SPLITS)
    add("usbmono_feed_yields", _cfg(8000, fmt=USB_MONO, enabled=0), fm(800.0), ny, splits=YIELD_SPLITS)
    add("fullscale_noise_usb", _cfg(8000, fmt=USB, gate=1), {"kind": "noise_full"}, 9000)
    for c in cases:
        assert sum(c["splits"]) == c["n"], c["name"]
        assert c["n"] / (c["cfg"][0] / c["cfg"][2]) <= 4700, c["name"]
    return cases


CASES = make_cases()
BY = {c["name"]: c for c in CASES}


def inputs(case: dict) -> np.ndarray:
    return signal(case["sig"], case["n"], case["cfg"][0], case["seed"])


def run_oracle(L: C.CDLL, case: dict, splits=None) -> dict:
    """the case through the oracle: per feed the payload, the spectrum, the open flags and the state after it"""
    o = OracleSsb(L, case["cfg"])
    feeds, specs, masks, states = [], [], [], []
    for x in cut(inputs(case), splits or case["splits"]):
        p, s = o.feed(x)
        feeds.append(p); specs.append(s); masks.append(o.last_open()); states.append(o.state())
    res = dict(o.state(), feeds=feeds, specs=specs, masks=masks, states=states, probe=o.probe(), filter=o.filter(), design=o.design())
    o.close()
    return res


# ---------------------------------------------------------------- random cases
RANDOM_SEED = 20261020
RATES = (8000.0, 11025.5, 48000.0)


def random_case(rng, i) -> dict:
    """one random configuration, signal and split list; the order of the rng calls is part of the case set"""
    in_rate, rate = 48000, float(rng.choice(RATES))
    fmt = int(rng.choice(FORMATS))
    kind = str(rng.choice(["nfm", "am", "burst", "burst", "noise_full", "zero"]))
    f0 = float(rng.integers(-3000, 3000))
    sig = {"kind": "am" if kind == "am" else ("nfm" if kind in ("nfm", "burst") else kind), "f0": f0, "dev": float(rng.choice([500.0, 2000.0])),
           "fa": float(rng.integers(100, 3000)), "amp": float(rng.integers(2, 20000)), "noise": float(rng.integers(0, 50))}
    if kind == "burst":
        sig["runs"] = [int(v) for v in rng.integers(1, in_rate // 8, size=8)]
        sig["amps"] = [float(rng.integers(300, 16000)), float(rng.integers(1, 30))]
    n = int(rng.integers(500, int(4000 * in_rate / rate)))
    cfg = (in_rate, -int(f0), rate, fmt, float(rng.choice([1300.0, 5000.0, 12500.0])), 2500, float(rng.choice([0.5, 1.0, 7.0, -3.0, 4.0e5])),
           int(rng.choice([-100, -60, -40, -20])), int(rng.choice([0, 0, 1, 2, 5, 17])), int(rng.random() < 0.7), int(rng.random() < 0.5))
    splits, left = [], n
    while left > 0:
        m = min(left, int(rng.choice([0, 1, 2, 32, 33, int(rng.integers(1, 300)), int(rng.integers(1, 8000))])))
        splits.append(m); left -= m
    return {"name": f"random{i}", "cfg": cfg, "sig": sig, "n": n, "seed": 3000 + i, "splits": splits}


def random_cases(count: int = 50) -> list[dict]:
    rng = np.random.default_rng(RANDOM_SEED)
    return [random_case(rng, i) for i in range(count)]
