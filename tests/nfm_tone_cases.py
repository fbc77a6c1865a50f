"""Cases of the NFM demodulator bank with CTCSS and the AF squelch (sdrx_nfm_create_ex) and the ctypes face of tests/nfm_tone_oracle.c, shared by
tests/test_nfm_tone_oracle.py (CPU), tests/test_nfm_tone_gpu.py and the golden recorder tests/golden/make_golden_nfm_tone.py.

A case is tests/nfm_cases.py's with three more configuration fields and a `tone` signal:
    cfg = (in_rate, nco_freq, audio_rate, rf_bandwidth, af_bandwidth, fm_deviation, volume, squelch, squelch_gate, audio_mute,
           ctcss_on, ctcss_index, delta_squelch)
    sig = {"kind": "tone", "tones": [(input samples, Hz or 0), ...], "tdev": Hz, ...}     a carrier modulated by an audio tone
          and, run by run, by a sub-audible one

Most cases run at an audio rate of 8000: the detector's block is N = 500 of its samples, one audio sample in eight, so 4000
open audio samples; the detector rate is 1000."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from tests import nfm_cases as nc
from tests.am_cases import _amp_runs
from tests.wfm_cases import _clip16, _gauss, cut  # noqa: F401  (cut is re-exported)

ROOT = nc.ROOT
ORACLE_SRC = os.path.join(ROOT, "tests", "nfm_tone_oracle.c")
PROBES = ("blocks", "detections", "chg_block", "chg_close", "mismatch", "det_samples")
AF_PROBES = ("af_block_ends", "af_max_zero", "af_second_eval", "af_zero_events", "af_zeroed_reads", "af_other_copy")
#: the 32 EIA tones; ctcss_index i names TONES[i - 1]
TONES = (67.0, 71.9, 74.4, 77.0, 79.7, 82.5, 85.4, 88.5, 91.5, 94.8, 97.4, 100.0, 103.5, 107.2, 110.9, 114.8, 118.8, 123.0, 127.3, 131.8,
         136.5, 141.3, 146.2, 151.4, 156.7, 162.2, 167.9, 173.8, 179.9, 186.2, 192.8, 203.5)


# ---------------------------------------------------------------- oracle
def build_oracle() -> C.CDLL:
    so = os.path.join(tempfile.mkdtemp(), "libnfmto.so")
    if not os.path.exists(os.path.join(nc.ORACLE_DIR, "libsdro.so")):
        subprocess.check_call(["make", "-C", nc.ORACLE_DIR, "libsdro.so"])
    subprocess.check_call(["cc", "-std=gnu11", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", ORACLE_SRC, "-o", so,
                           "-L" + nc.ORACLE_DIR, "-lsdro", "-Wl,-rpath," + nc.ORACLE_DIR, "-lm"])
    L = C.CDLL(so)
    L.nfmto_create.restype = C.c_void_p
    L.nfmto_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, C.c_float, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    L.nfmto_af.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.c_void_p, C.POINTER(C.c_int)]
    L.nfmto_af_probe.argtypes = [C.c_void_p, C.c_void_p]
    L.nfmto_level.restype = C.c_float
    L.nfmto_level.argtypes = [C.c_void_p]
    L.nfmto_destroy.argtypes = [C.c_void_p]
    L.nfmto_feed.restype = C.c_long
    L.nfmto_feed.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_void_p, C.c_long]
    L.nfmto_events.restype = C.c_long
    L.nfmto_events.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_long]
    L.nfmto_ctcss.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_long)]
    L.nfmto_powers.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_long)]
    L.nfmto_design.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p, C.c_void_p]
    L.nfmto_probe.argtypes = [C.c_void_p, C.c_void_p]
    L.nfmto_af_design.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.POINTER(C.c_double)]
    L.nfmto_base.restype = C.c_void_p
    L.nfmto_base.argtypes = [C.c_void_p]
    L.nfmo_levels.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_long)]
    L.nfmo_squelch_open.restype = C.c_int
    L.nfmo_squelch_open.argtypes = [C.c_void_p]
    L.nfmo_squelch_count.restype = C.c_int
    L.nfmo_squelch_count.argtypes = [C.c_void_p]
    L.nfmo_probe.argtypes = [C.c_void_p, C.c_void_p]
    return L


class OracleNfmTone:
    def __init__(self, L: C.CDLL, cfg):
        self.L = L
        self.cfg = cfg
        self.h = L.nfmto_create(int(cfg[0]), int(cfg[1]), int(cfg[2]), float(cfg[3]), float(cfg[4]), int(cfg[5]), float(cfg[6]), float(cfg[7]),
                                int(cfg[8]), int(cfg[9]), int(cfg[10]), int(cfg[11]), int(cfg[12]) if len(cfg) > 12 else 0)
        assert self.h
        self.base = L.nfmto_base(self.h)

    def feed(self, iq: np.ndarray) -> np.ndarray:
        iq = np.ascontiguousarray(iq, np.int16)
        n = iq.size // 2
        cap = n + 16                            # at most one audio sample per input
        out = np.empty(cap, np.int16)
        k = self.L.nfmto_feed(self.h, iq.ctypes.data, n, out.ctypes.data, cap)
        assert k <= cap
        return out[:k].copy()

    def events(self):
        """(audio sample positions in the last feed, new m_ctcssIndex values)"""
        n = self.L.nfmto_events(self.h, None, None, 0)
        at, idx = np.zeros(max(n, 1), np.int64), np.zeros(max(n, 1), np.int32)
        self.L.nfmto_events(self.h, at.ctypes.data, idx.ctypes.data, n)
        return at[:n].copy(), idx[:n].copy()

    def ctcss(self):
        i, n = C.c_int(), C.c_long()
        self.L.nfmto_ctcss(self.h, C.byref(i), C.byref(n))
        return i.value, n.value

    def powers(self):
        p = np.zeros(32, np.float32)
        d, m, n = C.c_int(), C.c_int(), C.c_long()
        self.L.nfmto_powers(self.h, p.ctypes.data, C.byref(d), C.byref(m), C.byref(n))
        return p, bool(d.value), m.value, n.value

    def design(self):
        n, r = C.c_int(), C.c_int()
        coef, lp = np.zeros(32, np.float32), np.zeros(151, np.float32)
        self.L.nfmto_design(self.h, C.byref(n), C.byref(r), coef.ctypes.data, lp.ctypes.data)
        return n.value, r.value, coef, lp

    def af(self):
        """(m_afSquelchOpen, the two moving-average sums, AFSquelch::m_squelchCount)"""
        o, k = C.c_int(), C.c_int()
        sums = np.zeros(2, np.float64)
        self.L.nfmto_af(self.h, C.byref(o), sums.ctypes.data, C.byref(k))
        return bool(o.value), sums, k.value

    def level(self) -> float:
        return self.L.nfmto_level(self.h)

    def af_design(self):
        """(AF block length N, tones[2], coef[2], threshold)"""
        n, th = C.c_int(), C.c_double()
        tones, coef = np.zeros(2, np.float64), np.zeros(2, np.float64)
        self.L.nfmto_af_design(self.h, C.byref(n), tones.ctypes.data, coef.ctypes.data, C.byref(th))
        return n.value, tones, coef, th.value

    def levels(self):
        m, s, p, n = C.c_double(), C.c_double(), C.c_double(), C.c_long()
        self.L.nfmo_levels(self.base, C.byref(m), C.byref(s), C.byref(p), C.byref(n))
        return m.value, s.value, p.value, n.value

    def probe(self) -> dict:
        out = np.zeros(len(PROBES), np.int64)
        self.L.nfmto_probe(self.h, out.ctypes.data)
        d = dict(zip(PROBES, (int(v) for v in out)))
        out = np.zeros(len(nc.PROBES), np.int64)
        self.L.nfmo_probe(self.base, out.ctypes.data)
        d.update(zip(nc.PROBES, (int(v) for v in out)))
        out = np.zeros(len(AF_PROBES), np.int64)
        self.L.nfmto_af_probe(self.h, out.ctypes.data)
        d.update(zip(AF_PROBES, (int(v) for v in out)))
        return d

    def close(self):
        if self.h:
            self.L.nfmto_destroy(self.h)
            self.h = None

    __del__ = close


# ---------------------------------------------------------------- signals
def signal(sig: dict, n: int, rate: int, seed: int) -> np.ndarray:
    if sig["kind"] != "tone":
        return nc.signal(sig, n, rate, seed)
    t = np.arange(n, dtype=np.float64)
    ft = np.zeros(n)
    pos = 0
    for m, hz in sig["tones"]:
        ft[pos: pos + m] = hz
        pos += m
    assert pos >= n, "the tone runs must cover the signal"
    # the sub-audible tone keeps its phase across runs of the same frequency: a phase accumulator, not sin(2 pi f t)
    tph = 2 * np.pi * np.cumsum(ft) / rate
    f = sig.get("f0", 0.0) + sig.get("dev", 1500.0) * np.sin(2 * np.pi * sig.get("fa", 1000.0) * t / rate) + np.where(ft > 0, sig.get("tdev", 400.0), 0.0) * np.sin(tph)
    inc = np.round(f / rate * 4294967296.0).astype(np.int64)
    ph = (np.cumsum(inc) & 0xFFFFFFFF).astype(np.float64) * (2 * np.pi / 4294967296.0)
    amp = _amp_runs(n, sig["runs"], sig["amps"]) if "runs" in sig else np.full(n, float(sig.get("amp", 8000.0)))
    sg = float(sig.get("noise", 20.0))
    iq = np.empty(2 * n, np.int16)
    iq[0::2] = _clip16(amp * np.cos(ph) + _gauss(seed, n, 3, sg))
    iq[1::2] = _clip16(amp * np.sin(ph) + _gauss(seed, n, 4, sg))
    return iq


# ---------------------------------------------------------------- cases
def _cfg(in_rate, audio_rate, on=1, index=0, nco_freq=0, delta=0, **kw):
    d = dict(nc.DEFAULT, gate=1, rf=8330.0); d.update(kw)
    return (in_rate, nco_freq, audio_rate, d["rf"], d["af"], d["fmdev"], d["vol"], d["sq"], d["gate"], d["mute"], on, index, delta)


#: cuts_block_ends: step 1 (8000 -> 8000), gate 80, a carrier from the first sample: the squelch opens at audio sample 80, the
#: detector takes samples 86, 94, ..., its blocks end at 4078, 8078, 12078 and 16078 (test_nfm_tone_oracle.py checks that).
#: Feeds: block 1 ends inside a feed; block 2 ends on a feed's last sample; block 3 on the first sample of a feed of 1; block 4
#: collects its 4000 samples over eleven feeds, with feeds of 0, 1 and 5 among them
CUT_ENDS = (4078, 8078, 12078, 16078)
CUT_SPLITS = [5000, 3079, 3999, 1, 0, 5, 400, 1, 0, 394, 1200, 700, 5, 0, 1, 1294, 921]


def make_cases() -> list[dict]:
    cases = []

    def add(name, cfg, sig, n, splits=None, seed=None):
        seed = 100 + len(cases) if seed is None else seed
        cases.append({"name": name, "cfg": cfg, "sig": sig, "n": n, "seed": seed, "splits": splits or nc._ragged(n, seed)})

    tone = lambda tones, **kw: dict({"kind": "tone", "tones": tones, "tdev": 400.0, "dev": 1500.0, "fa": 1000.0, "amp": 8000.0}, **kw)
    # 100.0 Hz is tone 12, 103.5 Hz tone 13
    add("tone_selected", _cfg(10000, 8000, index=12, nco_freq=-700), tone([(25000, 100.0)], f0=700.0), 25000)
    add("tone_other_selected", _cfg(10000, 8000, index=20, nco_freq=-700), tone([(25000, 100.0)], f0=700.0), 25000)
    add("tone_any", _cfg(10000, 8000, index=0, nco_freq=-700), tone([(25000, 100.0)], f0=700.0), 25000)
    add("no_tone", _cfg(10000, 8000, index=12, nco_freq=-700), tone([(25000, 0.0)], f0=700.0), 25000)
    add("tone_removed", _cfg(10000, 8000, index=12, nco_freq=-700), tone([(12000, 100.0), (18000, 0.0)], f0=700.0), 30000)
    # the carrier drops for 3000 inputs in the middle of a detector block and comes back: closing zeroes the index, the partial block survives
    add("carrier_gap", _cfg(10000, 8000, index=12, nco_freq=-700), tone([(40000, 100.0)], f0=700.0, runs=[13000, 3000, 24000], amps=[8000.0, 10.0]), 40000)
    add("neighbour_tones", _cfg(10000, 8000, index=13, nco_freq=-700), tone([(15000, 100.0), (20000, 103.5)], f0=700.0), 35000)
    add("tone_muted", _cfg(10000, 8000, index=12, nco_freq=-700, mute=1), tone([(25000, 100.0)], f0=700.0), 25000)
    add("cuts_block_ends", _cfg(8000, 8000, index=12, sq=-1000.0), tone([(17000, 100.0)], noise=0.0), 17000, splits=list(CUT_SPLITS))
    add("cuts_one_feed", _cfg(8000, 8000, index=12, sq=-1000.0), tone([(17000, 100.0)], noise=0.0), 17000, splits=[17000], seed=108)
    # 48 kHz audio: N = 3000, detector rate 6000, 24000 open samples to a block; 203.5 Hz is tone 32, 67.0 Hz tone 1
    add("rate48k_tone32", _cfg(60000, 48000, index=32, nco_freq=-3000, gate=5, rf=12500.0), tone([(70000, 203.5)], f0=3000.0, dev=2000.0), 70000)
    add("rate48k_tone1_other", _cfg(48000, 48000, index=2, gate=2, rf=12500.0), tone([(60000, 67.0)], dev=2000.0), 60000)
    # ---- the AF squelch (delta_squelch): at 8000 its block is 5 samples (N = 4), the tones are 1000 and 3200 Hz, the warm-up is
    # 600 blocks = 3000 samples, zeroBack reaches Z = 800 samples; squelch -100 is the threshold 0.1; gate 1 is 80 samples (< Z),
    # gate 12 is 960 (> Z).  A weak carrier (amplitude 30 under noise 20) makes the discriminator's output noise
    af = lambda on=0, index=0, **kw: _cfg(8000, 8000, on=on, index=index, delta=1, **dict({"sq": -100.0}, **kw))
    sig1k = lambda n, **kw: tone([(n, 0.0)], **kw)
    add("af_1k_opens", af(), sig1k(20000), 20000)
    add("af_noise_closed", af(), sig1k(20000, amp=30.0), 20000)
    add("af_sig_noise_sig_gate_lt_z", af(), sig1k(24000, runs=[9000, 6000, 9000], amps=[8000.0, 30.0]), 24000)
    add("af_sig_noise_sig_gate_gt_z", af(gate=12), sig1k(24000, runs=[9000, 6000, 9000], amps=[8000.0, 30.0]), 24000)
    # past the delay line's 24000 writes: noise on both sides of the lap, and the carrier drops at write 23920, so that the
    # squelch closes a few samples before the lap: the event clears the second copies of what was written before it, and the
    # reads behind the lap take the first copies, which still hold the samples
    add("af_lap", af(), sig1k(36000, runs=[7000, 3000, 13920, 5000, 7080], amps=[8000.0, 30.0]), 36000)
    add("af_gate_24000", af(gate=300), sig1k(36000), 36000)
    add("af_all_zero", af(), {"kind": "zero"}, 12000)
    add("af_threshold_straddled", af(sq=AF_STRADDLE_SQ), sig1k(20000, noise=AF_STRADDLE_NOISE), 20000)
    add("af_and_ctcss", af(on=1, index=12), tone([(24000, 100.0)], runs=[14000, 3000, 7000], amps=[8000.0, 30.0]), 24000)
    for c in cases:
        assert sum(c["splits"]) == c["n"], c["name"]
    return cases


#: af_threshold_straddled: noise under the carrier and a threshold (negative millis) that the ratio of the two sums crosses both
#: ways after the warm-up (tests/test_nfm_tone_oracle.py keeps it honest)
AF_STRADDLE_NOISE = 600.0
AF_STRADDLE_SQ = -100.0
CASES = make_cases()


def inputs(case: dict) -> np.ndarray:
    return signal(case["sig"], case["n"], case["cfg"][0], case["seed"])


def run_oracle(L: C.CDLL, case: dict, splits=None) -> dict:
    o = OracleNfmTone(L, case["cfg"])
    feeds, events = [], []
    for x in cut(inputs(case), splits or case["splits"]):
        feeds.append(o.feed(x))
        events.append(o.events())
    m, s, p, n = o.levels()
    index, changes = o.ctcss()
    power, detected, max_index, blocks = o.powers()
    af_open, af_sums, af_count = o.af()
    res = {"feeds": feeds, "events": events, "magsq": m, "sum": s, "peak": p, "count": n, "open": bool(L.nfmo_squelch_open(o.base)),
           "state": L.nfmo_squelch_count(o.base), "index": index, "changes": changes, "power": power, "detected": detected,
           "max_index": max_index, "blocks": blocks, "af_open": af_open, "af_sums": af_sums, "af_count": af_count, "probe": o.probe()}
    o.close()
    return res


def all_events(res: dict) -> list[tuple[int, int]]:
    """(audio sample position in the whole stream, new index) of every change"""
    out, base = [], 0
    for f, (at, idx) in zip(res["feeds"], res["events"]):
        out += [(base + int(a), int(i)) for a, i in zip(at, idx)]
        base += f.size
    return out


# ---------------------------------------------------------------- random cases
def random_case(rng, i) -> dict:
    """one random configuration, signal and split list at the short shapes; the order of the rng calls is part of the case set"""
    in_rate, audio = [(10000, 8000), (8000, 8000), (12000, 8000), (16000, 8000), (9000, 8000)][int(rng.integers(5))]
    f0 = float(rng.integers(-in_rate // 8, in_rate // 8))
    n = int(rng.integers(12000, 40000))
    tones, left = [], n
    while left > 0:
        m = min(left, int(rng.integers(3000, 20000)))
        tones.append((m, float(rng.choice([0.0, TONES[int(rng.integers(32))], 100.0, 103.5]))))
        left -= m
    sig = {"kind": "tone", "tones": tones, "f0": f0, "tdev": float(rng.choice([30.0, 150.0, 400.0, 700.0])), "dev": float(rng.choice([500.0, 1500.0])),
           "fa": float(rng.integers(300, 3000)), "amp": float(rng.integers(2000, 20000)), "noise": float(rng.integers(0, 50))}
    if rng.random() < 0.5:
        sig["runs"] = [int(v) for v in rng.integers(200, in_rate, size=6)]
        sig["amps"] = [float(rng.integers(3000, 16000)), float(rng.integers(1, 100))]
    on = int(rng.random() < 0.85)
    index = int(rng.choice([0, 12, 13, int(rng.integers(1, 33))]))
    cfg = (in_rate, -int(f0), audio, float(rng.choice([5000.0, 8330.0])), float(rng.choice([3000.0, 2400.0])), int(rng.choice([2000, 1234])),
           float(rng.choice([0.5, 2.0])), float(rng.choice([-600.0, -400.0, -300.0])), int(rng.choice([0, 1, 1, 2, 5])), int(rng.random() < 0.1), on, index)
    splits, left = [], n
    while left > 0:
        m = min(left, int(rng.choice([0, 1, 5, 33, int(rng.integers(1, 3000)), int(rng.integers(1, 15000))])))
        splits.append(m); left -= m
    # the AF squelch in three of ten; its threshold is then -squelch / 1000, here 0.3 ... 0.6, or 0.1
    delta = int(rng.random() < 0.3)
    if delta:
        cfg = cfg[:7] + (float(rng.choice([cfg[7], -100.0])),) + cfg[8:]
    return {"name": f"random{i}", "cfg": cfg + (delta,), "sig": sig, "n": n, "seed": 2000 + i, "splits": splits}


RANDOM_SEED = 20261020


def random_cases(count: int = 100) -> list[dict]:
    rng = np.random.default_rng(RANDOM_SEED)
    return [random_case(rng, i) for i in range(count)]
