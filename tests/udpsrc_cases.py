"""Cases of the UDPSrc bank (sdrx_udpsrc_*) and the ctypes face of tests/udpsrc_oracle.c, shared by tests/test_udpsrc_oracle.py
(CPU), tests/test_udpsrc_gpu.py and the golden recorder tests/golden/make_golden_udpsrc.py.

A case is a channel configuration, a signal at the channel rate and the lengths of the feeds it is cut into:
    cfg = (in_rate, nco_freq, output_sample_rate, sample_format, rf_bandwidth, fm_deviation, gain, squelch_db, squelch_gate, squelch_enabled, agc)
    sig = {"kind": ...}   see signal()

The shapes are the smallest that reach every carry: 48000 in, 8000 out in most cases (windows of 80 and 40 samples, a gate of
400 output samples = 2400 inputs at squelch_gate 5), 6000 .. 20000 inputs per case.  The generator is the portable one of
tests/wfm_cases.py / tests/nfm_cases.py with an `am` kind: a carrier at f0, amplitude-modulated by a tone, whose amplitude
follows a list of runs."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from tests import nfm_cases as _nc
from tests.am_cases import _amp_runs
from tests.wfm_cases import _clip16, _fm_phase, _gauss, cut  # noqa: F401  (cut is re-exported)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_SRC = os.path.join(ROOT, "tests", "udpsrc_oracle.c")

IQ16, IQ24, NFM, NFM_MONO, AM_MONO, AM_NODC_MONO, AM_BPF_MONO = 0, 1, 2, 3, 8, 9, 10
FORMATS = (IQ16, IQ24, NFM, NFM_MONO, AM_MONO, AM_NODC_MONO, AM_BPF_MONO)
#: numpy base type and components of one payload sample
PAYLOAD = {IQ16: (np.int16, 2), IQ24: (np.int32, 2), NFM: (np.int16, 2), NFM_MONO: (np.int16, 1), AM_MONO: (np.int16, 1),
           AM_NODC_MONO: (np.int16, 1), AM_BPF_MONO: (np.int16, 1)}
#: UDPSrcSettings::resetToDefaults, at 8000 S/s with a squelch gate
DEFAULT = dict(fmt=IQ16, rf=5000.0, fmdev=2500, gain=1.0, sqdb=-60, gate=5, enabled=1, agc=0)
PROBES = ("transitions", "open", "above_changes", "conv_wraps", "zero_ci", "release_hits", "gate_hits", "closed_above", "agc_up_ramp",
          "agc_down_ramp", "agc_mode_changes", "agc_cut")


def elem_bytes(fmt: int) -> int:
    t, k = PAYLOAD[fmt]
    return np.dtype(t).itemsize * k


def as_samples(fmt: int, raw: bytes) -> np.ndarray:
    """payload bytes as [n, 2] or [n] integers"""
    t, k = PAYLOAD[fmt]
    a = np.frombuffer(raw, t)
    return a.reshape(-1, 2).copy() if k == 2 else a.copy()


# ---------------------------------------------------------------- oracle
def build_oracle() -> C.CDLL:
    so = os.path.join(tempfile.mkdtemp(), "libudpo.so")
    subprocess.check_call(["cc", "-std=gnu11", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-w", ORACLE_SRC, "-o", so, "-lm"])
    L = C.CDLL(so)
    L.udpo_create.restype = C.c_void_p
    L.udpo_create.argtypes = [C.c_int, C.c_int, C.c_float, C.c_int, C.c_float, C.c_int, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int]
    L.udpo_destroy.argtypes = [C.c_void_p]
    L.udpo_feed.restype = C.c_long
    L.udpo_feed.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_void_p, C.c_void_p, C.c_long]
    L.udpo_state.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_void_p]
    L.udpo_probe.argtypes = [C.c_void_p, C.c_void_p]
    L.udpo_last_open.restype = C.c_long
    L.udpo_last_open.argtypes = [C.c_void_p, C.c_void_p, C.c_long]
    L.udpo_design.restype = C.c_int
    L.udpo_design.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int),
                              C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_void_p, C.POINTER(C.c_double)]
    return L


class OracleUdp:
    def __init__(self, L: C.CDLL, cfg):
        self.L = L
        self.cfg = cfg
        self.fmt = int(cfg[3])
        self.h = L.udpo_create(int(cfg[0]), int(cfg[1]), float(cfg[2]), int(cfg[3]), float(cfg[4]), int(cfg[5]), float(cfg[6]), int(cfg[7]),
                               int(cfg[8]), int(cfg[9]), int(cfg[10]) if len(cfg) > 10 else 0)
        assert self.h

    def feed(self, iq: np.ndarray):
        """(payload samples, spectrum Samples [n, 2]) of one feed"""
        iq = np.ascontiguousarray(iq, np.int16)
        n = iq.size // 2
        cap = n + 16                            # at most one output sample per input
        out = np.empty(cap * elem_bytes(self.fmt), np.uint8)
        spec = np.empty((cap, 2), np.int16)
        k = self.L.udpo_feed(self.h, iq.ctypes.data, n, out.ctypes.data, spec.ctypes.data, cap)
        assert k <= cap
        return as_samples(self.fmt, out[: k * elem_bytes(self.fmt)].tobytes()), spec[:k].copy()

    def last_open(self) -> np.ndarray:
        """m_squelchOpen for every sample of the last feed"""
        out = np.zeros(1 << 20, np.uint8)
        n = self.L.udpo_last_open(self.h, out.ctypes.data, out.size)
        return out[:n].astype(bool)

    def state(self) -> dict:
        m = C.c_double()
        st = np.zeros(4, np.int64)
        self.L.udpo_state(self.h, C.byref(m), st.ctypes.data)
        return {"in_magsq": m.value, "open": bool(st[0]), "open_count": int(st[1]), "close_count": int(st[2]), "total": int(st[3])}

    def probe(self) -> dict:
        out = np.zeros(len(PROBES), np.int64)
        self.L.udpo_probe(self.h, out.ctypes.data)
        return dict(zip(PROBES, (int(v) for v in out)))

    def design(self) -> dict:
        taps, bp, win, agc = np.zeros(16 * 128, np.float32), np.zeros(151, np.float32), np.zeros(3, np.int32), np.zeros(4, np.int32)
        thr = C.c_double()
        inc, gate, rel, lvl, fms, step = C.c_int(), C.c_int(), C.c_int(), C.c_double(), C.c_float(), C.c_float()
        nt = self.L.udpo_design(self.h, taps.ctypes.data, bp.ctypes.data, C.byref(inc), win.ctypes.data, C.byref(gate), C.byref(rel), C.byref(lvl),
                                C.byref(fms), C.byref(step), agc.ctypes.data, C.byref(thr))
        return {"agc": agc.tolist(), "agc_threshold": thr.value, "ntaps": nt, "taps": taps[: 16 * nt].copy(), "bandpass": bp, "nco_inc": inc.value, "windows": win.tolist(), "gate": gate.value,
                "release": rel.value, "level": lvl.value, "fm_scaling": fms.value, "step": step.value}

    def close(self):
        if self.h:
            self.L.udpo_destroy(self.h)
            self.h = None

    __del__ = close


# ---------------------------------------------------------------- portable signals
def signal(sig: dict, n: int, rate: int, seed: int) -> np.ndarray:
    if sig["kind"] != "am":
        return _nc.signal(sig, n, rate, seed)
    iq = np.empty(2 * n, np.int16)
    ph = _fm_phase(n, rate, sig.get("f0", 0.0), 0.0, 1000.0)
    amp = _amp_runs(n, sig["runs"], sig["amps"]) if "runs" in sig else np.full(n, float(sig.get("amp", 8000.0)))
    t = np.arange(n, dtype=np.float64)
    env = amp * (1.0 + float(sig.get("m", 0.5)) * np.sin(2 * np.pi * float(sig.get("fa", 700.0)) * t / rate))
    sg = float(sig.get("noise", 2.0))
    iq[0::2] = _clip16(env * np.cos(ph) + _gauss(seed, n, 3, sg))
    iq[1::2] = _clip16(env * np.sin(ph) + _gauss(seed, n, 4, sg))
    return iq


# ---------------------------------------------------------------- cases
def _cfg(in_rate, rate, nco_freq=0, **kw):
    d = dict(DEFAULT); d.update(kw)
    return (in_rate, nco_freq, float(rate), d["fmt"], d["rf"], d["fmdev"], d["gain"], d["sqdb"], d["gate"], d["enabled"], d["agc"])


def gate_samples(cfg) -> int:
    """m_squelchGate = m_squelchRelease"""
    return int(np.float32(np.float32(cfg[2]) * np.float32(cfg[8])) / np.float32(100))


#: input runs at 48000 in / 8000 out (x 1/6) around a gate of 400 output samples: the squelch opens twice and closes twice, one
#: burst (1500 inputs = 250 outputs) is shorter than the gate, one gap (500 inputs) shorter than the release
BURST_RUNS_5 = [4000, 3500, 1500, 1000, 5000, 500, 1500, 3000]
#: ... around a gate of 80 output samples = 480 inputs
BURST_RUNS_1 = [1000, 800, 300, 200, 1500, 700, 100, 100, 2000, 900, 400, 2000, 600, 1400]
#: ... and for the stateless gate 0
BURST_RUNS_0 = [700, 300, 50, 50, 1000, 900, 7, 13, 1500, 1480]
#: iq16_release_boundary: the number of inputs after which m_squelchCloseCount has just reached 0 with the squelch still open,
#: found on the oracle (tests/test_udpsrc_oracle.py::test_release_runs_out_at_a_feed_boundary keeps it honest); the output that
#: closes the squelch comes with the sixth input after it
RELEASE_BOUNDARY_SPLIT = 7926
_EDGES = [1, 31, 32, 33, 2, 3, 5, 7, 11, 13, 255, 256, 257, 1023, 1025, 4099, 0, 1]


def make_cases() -> list[dict]:
    cases = []

    def add(name, cfg, sig, n, splits=None, seed=None):
        seed = len(cases) + 1 if seed is None else seed
        cases.append({"name": name, "cfg": cfg, "sig": sig, "n": n, "seed": seed, "splits": splits or _nc._ragged(n, seed)})

    fm = lambda f0, **kw: dict({"kind": "nfm", "f0": f0, "dev": 2000.0, "fa": 700.0, "amp": 8000.0}, **kw)
    am = lambda f0, **kw: dict({"kind": "am", "f0": f0, "fa": 700.0, "amp": 8000.0}, **kw)
    on_off = [8000.0, 3.0]                                 # above and below the -60 dB squelch (amplitude 32.8)
    # squelch bursts, one per gate setting
    add("iq16_burst_gate5", _cfg(48000, 8000, nco_freq=-1000), fm(1000.0, runs=BURST_RUNS_5, amps=on_off), sum(BURST_RUNS_5))
    add("iq16_burst_gate1", _cfg(48000, 8000, nco_freq=-1000, gate=1), fm(1000.0, runs=BURST_RUNS_1, amps=on_off), sum(BURST_RUNS_1))
    add("iq16_burst_gate0", _cfg(48000, 8000, nco_freq=-1000, gate=0), fm(1000.0, runs=BURST_RUNS_0, amps=on_off), sum(BURST_RUNS_0))
    add("iq16_short_burst", _cfg(48000, 8000), fm(0.0, runs=[1000, 1800, 7200], amps=[3.0, 8000.0, 3.0]), 10000)
    add("iq16_release_boundary", _cfg(48000, 8000), fm(0.0, runs=[5000, 5000], amps=on_off), 10000,
        splits=[2000, 33, RELEASE_BOUNDARY_SPLIT - 2033, 6, 10000 - RELEASE_BOUNDARY_SPLIT - 6])
    add("iq16_squelch_off", _cfg(48000, 8000, enabled=0, gate=1), fm(0.0, amp=3.0, noise=1.0), 6000)
    add("iq16_overflow_gain", _cfg(48000, 8000, gain=10.0, gate=1), fm(500.0, amp=9000.0), 6000)
    add("iq24_burst", _cfg(48000, 8000, fmt=IQ24, gate=1), fm(-700.0, runs=BURST_RUNS_1, amps=on_off), sum(BURST_RUNS_1))
    add("iq24_overflow_gain", _cfg(48000, 8000, fmt=IQ24, gain=-7.5, gate=0), fm(500.0, amp=12000.0), 6000)
    # discriminator on open samples only: fm_scaling * gain = 1.6 and 0.8 * 2 (below 8), then 9.6 (overflowing)
    add("nfm_burst", _cfg(48000, 8000, fmt=NFM, gate=1, nco_freq=-1000), fm(1000.0, dev=1500.0, runs=BURST_RUNS_1, amps=on_off), sum(BURST_RUNS_1))
    add("nfmmono_burst_gate5", _cfg(48000, 8000, fmt=NFM_MONO, fmdev=5000, gain=2.0), fm(0.0, dev=2500.0, runs=BURST_RUNS_5, amps=on_off), sum(BURST_RUNS_5))
    add("nfm_overflow_9p6", _cfg(48000, 48000, fmt=NFM, rf=12500.0, gate=0), fm(0.0, dev=2500.0), 8000)
    add("nfmmono_zero_input", _cfg(48000, 8000, fmt=NFM_MONO, enabled=0, gate=0), {"kind": "zero"}, 6000)
    # AM formats
    add("am_burst", _cfg(48000, 8000, fmt=AM_MONO, gate=1, nco_freq=300), am(-300.0, runs=BURST_RUNS_1, amps=on_off), sum(BURST_RUNS_1))
    add("am_overflow_gain", _cfg(48000, 8000, fmt=AM_MONO, gain=6.0, gate=0), am(0.0, amp=9000.0), 6000)
    add("amnodc_burst", _cfg(48000, 8000, fmt=AM_NODC_MONO, gate=1), am(0.0, runs=BURST_RUNS_1, amps=on_off), sum(BURST_RUNS_1))
    add("ambpf_burst", _cfg(48000, 8000, fmt=AM_BPF_MONO, gate=1), am(0.0, runs=BURST_RUNS_1, amps=on_off), sum(BURST_RUNS_1))
    # fewer open samples in a feed than the 40-sample window / the 300 ring entries, then more: feeds of 60 inputs = 10 outputs
    small = [60] * 50 + [600] * 5 + [3000, 4000]
    add("amnodc_small_feeds", _cfg(48000, 8000, fmt=AM_NODC_MONO, gate=0, gain=3.0), am(200.0), sum(small), splits=small)
    add("ambpf_small_feeds", _cfg(48000, 8000, fmt=AM_BPF_MONO, gate=0, gain=3.0), am(200.0, fa=1000.0), sum(small), splits=small)
    add("amnodc_zero_open", _cfg(48000, 8000, fmt=AM_NODC_MONO, enabled=0, gate=0), {"kind": "zero"}, 6000)
    add("ambpf_all_zero", _cfg(48000, 8000, fmt=AM_BPF_MONO), {"kind": "zero"}, 6000)
    # MagAGC on for the AM formats: the threshold is powerFromdB(squelch_db) * 2^23 on the RAW power, amplitude 2.9 at -60 dB, so
    # at -60 dB nothing here ever goes below it.  At -20 dB it is amplitude 290: the runs alternate between 8000 and 40 -- above
    # the squelch (32.8 on the averaged power) on both levels, across the AGC threshold in both directions -- over stretches
    # longer and shorter than the AGC gate (400 outputs), the step-down delay (80 or 400) and the step length (400)
    agc_runs = [4000, 4000, 4000, 1000, 3000, 300, 3700]
    agc_sig = lambda **kw: am(0.0, runs=agc_runs, amps=[8000.0, 40.0], **kw)
    add("am_agc_cross", _cfg(48000, 8000, fmt=AM_MONO, sqdb=-20, gate=1, agc=1, enabled=0), agc_sig(), sum(agc_runs))
    add("amnodc_agc_cross", _cfg(48000, 8000, fmt=AM_NODC_MONO, sqdb=-20, gate=5, agc=1, enabled=0), agc_sig(fa=400.0), sum(agc_runs))
    add("ambpf_agc_cross", _cfg(48000, 8000, fmt=AM_BPF_MONO, sqdb=-20, gate=0, agc=1, enabled=0, gain=0.5), agc_sig(fa=1000.0), sum(agc_runs))
    # the squelch enabled at the same level: the channel closes while the AGC ramps down, and opens behind its gate
    add("am_agc_squelched", _cfg(48000, 8000, fmt=AM_MONO, sqdb=-30, gate=1, agc=1), am(0.0, runs=[6000, 5000, 500, 4000, 4500], amps=[8000.0, 20.0]), 20000)
    add("ambpf_agc_default", _cfg(48000, 8000, fmt=AM_BPF_MONO, agc=1, gate=1), am(0.0, runs=BURST_RUNS_1, amps=on_off), sum(BURST_RUNS_1))
    add("amnodc_agc_zero_input", _cfg(48000, 8000, fmt=AM_NODC_MONO, agc=1, enabled=0, gate=0), {"kind": "zero"}, 6000)
    add("am_agc_nondyadic_62500", _cfg(62500, 48000, fmt=AM_MONO, rf=12500.0, sqdb=-20, gate=1, agc=1, enabled=0),
        am(0.0, runs=[6000, 7000, 7000], amps=[8000.0, 40.0]), 20000)
    # other rates: step 1, a non-dyadic step (the serial resampler schedule), 96000 -> 44100, a rate that is no integer
    add("iq16_step1_48k", _cfg(48000, 48000, rf=12500.0, gate=1), fm(0.0, runs=[3000, 2000, 3000], amps=on_off), 8000)
    add("am_nondyadic_62500", _cfg(62500, 48000, fmt=AM_MONO, rf=12500.0, gate=1, nco_freq=1700), am(-1700.0, runs=[4000, 2000, 4000], amps=on_off), 10000)
    add("ambpf_r96k_to_44k1", _cfg(96000, 44100, fmt=AM_BPF_MONO, rf=10000.0, gate=1, nco_freq=-12000), am(12000.0, runs=[6000, 3000, 5000], amps=on_off), 14000)
    add("nfm_float_rate", _cfg(48000, 11025.5, fmt=NFM, fmdev=2500, gate=2), fm(0.0, dev=2000.0, runs=[5000, 3000, 4000], amps=on_off), 12000)
    add("fullscale_noise", _cfg(48000, 8000, fmt=AM_NODC_MONO, gate=1), {"kind": "noise_full"}, 6000)
    add("splits_edges", _cfg(48000, 8000, fmt=AM_BPF_MONO, gate=1, nco_freq=-345), am(345.0), 12000, splits=_EDGES + [12000 - sum(_EDGES)], seed=27)
    add("one_long_feed", _cfg(48000, 8000, fmt=AM_BPF_MONO, gate=1, nco_freq=-345), am(345.0), 12000, splits=[12000], seed=27)
    for c in cases:
        assert sum(c["splits"]) == c["n"], c["name"]
        assert 6000 <= c["n"] <= 20000, c["name"]
    return cases


CASES = make_cases()


def inputs(case: dict) -> np.ndarray:
    return signal(case["sig"], case["n"], case["cfg"][0], case["seed"])


def run_oracle(L: C.CDLL, case: dict, splits=None) -> dict:
    o = OracleUdp(L, case["cfg"])
    feeds, specs, opens, masks = [], [], [], []
    for x in cut(inputs(case), splits or case["splits"]):
        p, s = o.feed(x)
        feeds.append(p); specs.append(s); opens.append(o.state()["open"]); masks.append(o.last_open())
    res = dict(o.state(), feeds=feeds, specs=specs, opens=opens, masks=masks, probe=o.probe())
    o.close()
    return res


# ---------------------------------------------------------------- random cases
def random_case(rng, i) -> dict:
    """one random configuration, signal and split list; the order of the rng calls is part of the case set"""
    rates = [(48000, 8000.0), (48000, 48000.0), (62500, 48000.0), (96000, 44100.0), (48000, 11025.5), (60000, 48000.0), (50000, 44100.0),
             (48000, 32000.0), (16000, 1000.0), (48000, 7999.25)]
    in_rate, rate = rates[int(rng.integers(len(rates)))]
    fmt = int(rng.choice(FORMATS))
    kind = str(rng.choice(["nfm", "am", "burst", "noise_full", "zero", "burst"]))
    f0 = float(rng.integers(-in_rate // 8, in_rate // 8))
    base = "am" if (kind in ("am", "burst") and fmt >= 8) else ("nfm" if kind in ("nfm", "am", "burst") else kind)
    sig = {"kind": base, "f0": f0, "dev": float(rng.choice([500.0, 2000.0])), "fa": float(rng.integers(100, 3000)),
           "amp": float(rng.integers(2, 20000)), "noise": float(rng.integers(0, 50))}
    if kind == "burst":
        sig["runs"] = [int(v) for v in rng.integers(1, in_rate // 8, size=8)]
        sig["amps"] = [float(rng.integers(300, 16000)), float(rng.integers(1, 30))]
    n = int(rng.integers(500, 20000))
    cfg = (in_rate, -int(f0), rate, fmt, float(rng.choice([1300.0, 5000.0, 12500.0])), int(rng.choice([2500, 5000, 100])),
           float(rng.choice([0.5, 1.0, 7.0, -3.0])), int(rng.choice([-100, -60, -40, -20])), int(rng.choice([0, 0, 1, 2, 5, 17])), int(rng.random() < 0.8), int(rng.random() < 0.5))
    if cfg[10] and fmt >= 8 and kind == "burst":             # the raw power on both sides of the AGC threshold (amplitude 290 at -20 dB)
        cfg = cfg[:7] + (int(rng.choice([-20, -10])),) + cfg[8:]
        sig["amps"] = [float(rng.integers(3000, 16000)), float(rng.integers(1, 100))]
    splits, left = [], n
    while left > 0:
        m = min(left, int(rng.choice([0, 1, 2, 32, 33, int(rng.integers(1, 300)), int(rng.integers(1, 8000))])))
        splits.append(m); left -= m
    return {"name": f"random{i}", "cfg": cfg, "sig": sig, "n": n, "seed": 2000 + i, "splits": splits}


#: the seed of random_cases(): the cases the `ref` test of tests/test_udpsrc_oracle.py proves against the reference
RANDOM_SEED = 20261018


def random_cases(count: int = 100) -> list[dict]:
    """the first `count` random cases, drawn in order from one generator"""
    rng = np.random.default_rng(RANDOM_SEED)
    return [random_case(rng, i) for i in range(count)]
