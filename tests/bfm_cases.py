"""Cases of the broadcast-FM stereo demodulator bank (sdrx_bfm_*) and the ctypes face of tests/bfm_oracle.c, shared by
tests/test_bfm_oracle.py (CPU), tests/test_bfm_gpu.py and the golden recorder tests/golden/make_golden_bfm.py.

A case is a demodulator configuration, a signal at the channel rate and the lengths of the feeds it is cut into:
    cfg = dict(in_rate, nco_freq, audio_rate, rf, af, vol, sq, stereo, lsb, pilot)
    sig = {"kind": ...}   see signal(); "mpx" is a stereo multiplex (L+R, 19 kHz pilot, 38 kHz DSB-SC L-R) FM-modulated to int16 I/Q

The generator is wfm_cases' portable one (counter-based splitmix64 noise, a 32-bit integer phase accumulator).

random_cases() is the draw of 100 configurations that tests/test_bfm_random_gpu.py runs in wide banks: audio rates other than
48000, resampler steps from 1 to 12 on both schedules, every list value of af, volume and squelch level.  assert_random_shares()
holds it to its floors; all of them are met (the lists and RANDOM_SEED were tuned to them).  pack_digests() is the layout of its
fixture, tests/golden/bfm_random_golden.npz."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from tests import wfm_cases as wc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_SRC = os.path.join(ROOT, "tests", "bfm_oracle.c")
ORACLE_DIR = os.path.join(ROOT, "oracle")
GOLDEN = os.path.join(ROOT, "tests", "golden", "bfm_golden.npz")

FIELDS = ("in_rate", "nco_freq", "audio_rate", "rf", "af", "vol", "sq", "stereo", "lsb", "pilot")
DEFAULT = dict(nco_freq=0, rf=60000.0, af=15000.0, vol=2.0, sq=-60.0, stereo=1, lsb=0, pilot=0)
PROBE = ("ratio", "plus", "minus", "clamp_lo", "clamp_hi", "wrap", "lock_up", "lock_reset", "sched_mismatch", "ge")

cut = wc.cut


# ---------------------------------------------------------------- oracle
def build_oracle() -> C.CDLL:
    so = os.path.join(tempfile.mkdtemp(), "libbfo.so")
    if not os.path.exists(os.path.join(ORACLE_DIR, "libsdro.so")):
        subprocess.check_call(["make", "-C", ORACLE_DIR, "libsdro.so"])
    subprocess.check_call(["cc", "-std=gnu11", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", ORACLE_SRC, "-o", so,
                           "-L" + ORACLE_DIR, "-lsdro", "-Wl,-rpath," + ORACLE_DIR, "-lm"])
    L = C.CDLL(so)
    L.bfo_create.restype = C.c_void_p
    L.bfo_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int, C.c_int, C.c_int]
    L.bfo_destroy.argtypes = [C.c_void_p]
    L.bfo_feed.restype = C.c_long
    L.bfo_feed.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_void_p, C.c_long, C.c_void_p, C.c_long, C.POINTER(C.c_long)]
    L.bfo_state.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_long), C.c_void_p, C.c_void_p]
    L.bfo_probe.argtypes = [C.c_void_p, C.c_void_p]
    L.bfo_design.restype = C.c_int
    L.bfo_design.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_float), C.c_void_p, C.POINTER(C.c_int), C.c_void_p]
    return L


class OracleBfm:
    def __init__(self, L: C.CDLL, cfg: dict):
        self.L = L
        self.cfg = cfg
        self.h = L.bfo_create(int(cfg["in_rate"]), int(cfg["nco_freq"]), int(cfg["audio_rate"]), float(cfg["rf"]), float(cfg["af"]),
                              float(cfg["vol"]), float(cfg["sq"]), int(cfg["stereo"]), int(cfg["lsb"]), int(cfg["pilot"]))
        assert self.h

    def feed(self, iq: np.ndarray):
        """(audio [n, 2] of l, r; real parts of the sink stream's Samples)"""
        iq = np.ascontiguousarray(iq, np.int16)
        n = iq.size // 2
        cap = n + 1024                          # pending (< 512) + new, at most one audio pair and one Sample per input
        audio, sink = np.empty((cap, 2), np.int16), np.empty(cap, np.int16)
        ns = C.c_long()
        k = self.L.bfo_feed(self.h, iq.ctypes.data, n, audio.ctypes.data, cap, sink.ctypes.data, cap, C.byref(ns))
        assert k <= cap and ns.value <= cap
        return audio[:k].copy(), sink[:ns.value].copy()

    def state(self) -> dict:
        s, p, n = C.c_double(), C.c_double(), C.c_long()
        ints, bits = np.zeros(3, np.int32), np.zeros(5, np.uint32)
        self.L.bfo_state(self.h, C.byref(s), C.byref(p), C.byref(n), ints.ctypes.data, bits.ctypes.data)
        return {"sum": s.value, "peak": p.value, "count": n.value, "sq_state": int(ints[0]), "locked": int(ints[1]), "lock_cnt": int(ints[2]),
                "bits": bits}

    def probe(self) -> dict:
        out = np.zeros(len(PROBE), np.int64)
        self.L.bfo_probe(self.h, out.ctypes.data)
        return dict(zip(PROBE, (int(v) for v in out)))

    def design(self):
        taps, filt = np.zeros(16 * 128, np.float32), np.zeros(2048, np.float32)
        pll, rc = np.zeros(7, np.float32), np.zeros(2, np.float32)
        inc, lvl, ld = C.c_int(), C.c_float(), C.c_int()
        nt = self.L.bfo_design(self.h, taps.ctypes.data, filt.ctypes.data, C.byref(inc), C.byref(lvl), pll.ctypes.data, C.byref(ld), rc.ctypes.data)
        return nt, taps[: 16 * nt].copy(), filt, inc.value, lvl.value, pll, ld.value, rc

    def close(self):
        if self.h:
            self.L.bfo_destroy(self.h)
            self.h = None

    __del__ = close


# ---------------------------------------------------------------- signals
def _mpx_phase(n: int, rate: int, sig: dict) -> np.ndarray:
    """carrier phase (radians, from a uint32 accumulator) of a stereo multiplex FM-modulated onto f0.  Deviations in Hz: `sum`
    of the L+R tone fs, `pilot` of the pilot at fp (from sample p_on up to p_off), `diff` of the L-R tone fd on the
    suppressed carrier at 2 * fp, phase-locked to the pilot"""
    t = np.arange(n, dtype=np.float64)
    fp = float(sig.get("fp", 19000.0))
    pil = 2 * np.pi * fp * t / rate
    on = (t >= sig.get("p_on", 0)) & (t < sig.get("p_off", n))
    m = (sig.get("sum", 20000.0) * np.sin(2 * np.pi * sig.get("fs", 1000.0) * t / rate)
         + sig.get("pilot", 7500.0) * np.sin(pil) * on
         + sig.get("diff", 15000.0) * np.sin(2 * np.pi * sig.get("fd", 700.0) * t / rate) * np.sin(2 * pil))
    inc = np.round((sig.get("f0", 0.0) + m) / rate * 4294967296.0).astype(np.int64)
    return (np.cumsum(inc) & 0xFFFFFFFF).astype(np.float64) * (2 * np.pi / 4294967296.0)


def signal(sig: dict, n: int, rate: int, seed: int) -> np.ndarray:
    if sig["kind"] != "mpx":
        return wc.signal(sig, n, rate, seed)
    ph = _mpx_phase(n, rate, sig)
    amp = np.full(n, float(sig.get("amp", 8000.0)))
    if "runs" in sig:                                   # amplitude alternating lo / hi over the listed stretches (cycled), lo first
        pos, k, hi = 0, 0, False
        while pos < n:
            r = sig["runs"][k % len(sig["runs"])]
            amp[pos:pos + r] = sig["hi"] if hi else sig["lo"]
            pos += r; k += 1; hi = not hi
    sg = float(sig.get("noise", 20.0))
    iq = np.empty(2 * n, np.int16)
    iq[0::2] = wc._clip16(amp * np.cos(ph) + wc._gauss(seed, n, 3, sg))
    iq[1::2] = wc._clip16(amp * np.sin(ph) + wc._gauss(seed, n, 4, sg))
    return iq


# ---------------------------------------------------------------- cases
def _cfg(in_rate, audio_rate=48000, **kw) -> dict:
    d = dict(DEFAULT); d.update(kw); d.update(in_rate=in_rate, audio_rate=audio_rate)
    assert set(d) == set(FIELDS)
    return d


def _tail(n, head):
    assert sum(head) <= n
    return head + [n - sum(head)]


def make_cases() -> list[dict]:
    cases = []

    def add(name, cfg, sig, n, splits, seed=None):
        seed = len(cases) + 1 if seed is None else seed
        assert sum(splits) == n, name
        cases.append({"name": name, "cfg": cfg, "sig": sig, "n": n, "seed": seed, "splits": splits})

    mpx = lambda **kw: dict({"kind": "mpx"}, **kw)
    edges = [0, 1, 511, 512, 513, 2, 700]
    # the three rates; mono, stereo, lsb_stereo; the feed lengths at the block's edges and one long feed
    add("stereo_240k", _cfg(240000, nco_freq=-20000), mpx(f0=20000.0), 9000, _tail(9000, edges))
    add("lsb_384k", _cfg(384000, lsb=1, nco_freq=31000), mpx(f0=-31000.0, sum=30000.0), 7000, _tail(7000, [1500, 0, 3]))
    add("mono_250k", _cfg(250000, stereo=0, nco_freq=12345), mpx(f0=-12345.0), 6000, _tail(6000, [513, 1000]))
    add("stereo_250k", _cfg(250000, rf=50000.0), mpx(), 6000, _tail(6000, [2049, 511]))
    add("mono_240k_one_feed", _cfg(240000, stereo=0, lsb=1), mpx(), 4096, [4096])
    # the sink stream's three forms
    add("show_pilot_stereo", _cfg(240000, pilot=1), mpx(), 5000, _tail(5000, [1025]))
    add("show_pilot_mono", _cfg(240000, pilot=1, stereo=0), mpx(), 3000, _tail(3000, [600]))
    # squelch: open above rfBW / 20 = 625 samples, saturation at 1250.  The signal starts low: the first open sample lies in the
    # fourth feed.  Stretches shorter and longer than both limits, none a multiple of 512: the counter opens and closes inside
    # blocks and across feed boundaries, m_m1Sample survives the closures, the pilot loop runs through them on demod = 0
    add("squelch_bursts", _cfg(240000, rf=12500.0, sq=-30.0), mpx(sum=2000.0, pilot=750.0, diff=1000.0, hi=12000.0, lo=60.0, noise=5.0,
                                                                  runs=[2100, 700, 300, 1700, 200, 900, 1500, 640, 650, 2600]), 12000,
        _tail(12000, [512, 1024, 300, 1300, 1388, 2000, 700]))
    add("volume_clips", _cfg(240000, vol=400.0), mpx(), 4608, _tail(4608, [1536]))
    # the pilot loop: a pilot that stops (m_lock_cnt back to 0), pilots off frequency (m_freq pinned at either limit), none
    add("pilot_stops", _cfg(240000), mpx(p_off=5500), 8000, _tail(8000, [3000, 2000]))
    add("pilot_19k2", _cfg(240000), mpx(fp=19200.0), 6000, _tail(6000, [2500]))
    # at 19.2 kHz the loop never gets there (the phasor turns at 200 Hz, +1 and -1 take turns and m_freq only swings around
    # m_minfreq, where the closed squelch left it); 45 Hz high at 48 kS/s it follows until m_maxfreq stops it
    add("pilot_19k045_48k", _cfg(48000, rf=44000.0), mpx(fp=19045.0, sum=3000.0, diff=1000.0), 6000, _tail(6000, [2200, 513]))
    add("pilot_18k8", _cfg(240000, lsb=1), mpx(fp=18800.0), 6000, _tail(6000, [1000]))
    add("noise_no_pilot", _cfg(240000), {"kind": "noise_full"}, 5000, _tail(5000, [2048]))
    add("all_zero", _cfg(240000), {"kind": "zero"}, 2048, [1024, 1024])
    # a pilot at the nominal 10 % that reaches lock: m_lock_delay = int(20.0 / (50.0 / in_rate)) = 0.4 s of samples at any rate
    add("lock_96k", _cfg(96000, rf=48000.0), mpx(sum=8000.0, diff=4000.0, fs=400.0), 43008, _tail(43008, [20000, 18500, 1]))
    return cases


CASES = make_cases()


def inputs(case: dict) -> np.ndarray:
    return signal(case["sig"], case["n"], case["cfg"]["in_rate"], case["seed"])


def run_oracle(L: C.CDLL, case: dict, splits=None, iq=None) -> dict:
    """audio and sink per feed, the state after every feed, the probe counts after the last"""
    o = OracleBfm(L, case["cfg"])
    audio, sink, states = [], [], []
    for x in cut(inputs(case) if iq is None else iq, splits or case["splits"]):
        a, s = o.feed(x)
        audio.append(a); sink.append(s); states.append(o.state())
    res = {"audio": audio, "sink": sink, "states": states, "probe": o.probe()}
    o.close()
    return res


# ---------------------------------------------------------------- random configurations
#: the seed of random_cases(): the cases the `ref` test of tests/test_bfm_oracle.py proves against the reference
RANDOM_SEED = 20261059
RANDOM_GOLDEN = os.path.join(ROOT, "tests", "golden", "bfm_random_golden.npz")     # digests: tests/golden/make_golden_bfm.py --random
#: (in_rate, audio_rate): both schedules (wfm_cases.dyadic_step), audio rates other than 48000, then step 1, a step below 1.1 and a
#: step within 2^-15 of 1; at the end the closed form's fractional steps 2.5, 1.25 and 1.5 (every other closed-form step is an integer)
RANDOM_RATES = ((240000, 48000), (250000, 48000), (384000, 48000), (384000, 44100), (250000, 44100), (200000, 44100), (192000, 32000),
                (96000, 8000), (96000, 48000), (48000, 48000), (48000, 44100), (48001, 48000), (120000, 48000), (60000, 48000), (66150, 44100))
RANDOM_RF = (12500.0, 12345.0, 50000.0, 60000.0, 80005.0, 180000.0, 220000.0)
RANDOM_AMP = (3000.0, 8000.0, 12000.0, 12000.0, 20000.0, 20000.0, 32767.0, 45000.0)            # 45000 clips
RANDOM_FP = (19000.0, 19000.0, 19000.0, 19003.0, 18996.0, 19045.0, 18800.0, 19200.0)
#: every LOCK_EVERY-th case is a lock case: 48 or 96 kS/s, a clean pilot at 10 % of 75 kHz, longer than m_lock_delay (0.4 s)
LOCK_EVERY, LOCK_AT = 16, 5
LOCK_RATES = ((48000, 48000), (96000, 48000), (48000, 44100), (96000, 8000), (48001, 48000))
MAX_FEEDS = 24
WIDE_N = 16000                      # the wide GPU bank cycles over the cases up to this length


def _f32(v) -> float:
    return float(np.float32(v))


def _random_splits(rng, n: int) -> list[int]:
    """as wfm_cases.random_case draws them, at most MAX_FEEDS feeds, the last taking the rest"""
    splits, left = [], n
    while left > 0:
        m = min(left, int(rng.choice([1, 511, 512, 513, int(rng.integers(1, 3000)), int(rng.integers(1, 30000))])))
        if len(splits) == MAX_FEEDS - 1:
            m = left
        splits.append(m); left -= m
    return splits


def random_case(rng, i: int) -> dict:
    """one random configuration, signal and split list.  Every quantity is drawn for every case, used or not: the order and number
    of the rng calls ahead of the splits do not depend on what was drawn"""
    lock = i % LOCK_EVERY == LOCK_AT
    rates = LOCK_RATES if lock else RANDOM_RATES
    in_rate, audio = rates[int(rng.integers(len(rates)))]
    rf = _f32(min(float(rng.choice(RANDOM_RF)), 0.9 * in_rate))
    af = float(rng.choice([3000.0, 15000.0, 20000.0]))
    vol = float(rng.choice([0.5, 2.0, 10.0, 400.0]))
    sq = float(rng.choice([-60.0, -30.0, -25.5, -10.0]))
    stereo, lsb, pilot = int(rng.random() < 0.65), int(rng.random() < 0.3), int(rng.random() < 0.2)
    f0 = float(rng.integers(-in_rate // 8, in_rate // 8))
    kind = str(rng.choice(["mpx"] * 16 + ["noise_full"] * 2 + ["zero"]))
    dev = min(75000.0, 0.45 * rf)                               # the multiplex's peak deviation, inside the RF filter
    share = rng.dirichlet([2.0, 2.0])
    sig = {"kind": "mpx", "f0": f0, "fp": float(rng.choice(RANDOM_FP)), "amp": float(rng.choice(RANDOM_AMP)),
           "pilot": _f32(dev * rng.choice([0.0, 0.05, 0.1, 0.1, 0.2])), "sum": _f32(0.85 * dev * share[0]), "diff": _f32(0.85 * dev * share[1]),
           "fs": float(rng.integers(100, 5000)), "fd": float(rng.integers(100, 5000)), "noise": float(rng.integers(0, 50))}
    n = int(rng.integers(2000, WIDE_N + 1)) if rng.random() < 0.6 else int(rng.integers(WIDE_N + 1, 40001))
    windows, bursts = rng.random() < 0.25, rng.random() < 0.32       # a quarter of all cases: four in five can burst
    bursts = bursts and kind == "mpx" and not lock
    if bursts:
        rf = min(rf, 60000.0)
    # the squelch counter opens above rf / 20 and stops at rf / 10: a stretch of rf / 12 and a block opens it from 0 and closes it
    # from the cap, so every stretch flips it, wherever the blocks fall
    lo, runs = float(rng.integers(1, 200)), [int(v) + 512 for v in rng.integers(int(rf / 12), int(rf / 5) + 2, size=8)]
    if bursts:                                                  # an odd number of stretches, at least three: the last one is low
        ends = np.cumsum([runs[k % 8] for k in range(64)])
        n = int(ends[max(2, max(k for k in range(0, 64, 2) if ends[k] <= max(n, ends[2])))])
    n = max(n, int(rf / 10) + 1000)                             # room for the squelch counter to reach rf / 20 and open
    p_on, p_len = int(rng.integers(0, n // 2)), int(rng.integers(n // 8, n))
    if lock:
        stereo, sq, kind = 1, -60.0, "mpx"
        rf = _f32(min(48000.0, 0.9 * in_rate))
        sig.update(fp=19000.0, pilot=7500.0, sum=8000.0, diff=4000.0, fs=400.0, amp=8000.0, noise=20.0)
        n = int((0.45 + 0.05 * rng.random()) * in_rate) + 1
    elif kind == "mpx":
        if windows:
            sig.update(p_on=p_on, p_off=p_on + p_len)
        if bursts:                                              # the squelch opens and closes inside blocks: hi above every level, lo below
            sig.update(hi=12000.0, lo=min(lo, 20.0) if sq == -60.0 else lo, noise=min(sig["noise"], 5.0), runs=runs)
    else:
        sig = {"kind": kind}
    cfg = _cfg(in_rate, audio, nco_freq=-int(f0), rf=rf, af=af, vol=vol, sq=sq, stereo=stereo, lsb=lsb, pilot=pilot)
    return {"name": f"random{i}", "cfg": cfg, "sig": sig, "n": n, "seed": 1000 + i, "splits": _random_splits(rng, n)}


def random_cases(count: int = 100) -> list[dict]:
    """the first `count` random cases, drawn in order from one generator"""
    rng = np.random.default_rng(RANDOM_SEED)
    return [random_case(rng, i) for i in range(count)]


def rate_triple(cfg: dict) -> tuple:
    """what wfm_cases.dyadic_step reads"""
    return (cfg["in_rate"], cfg["nco_freq"], cfg["audio_rate"])


def is_dyadic(case: dict) -> bool:
    """whether sdrx_bfm_create gives the channel the closed-form schedule (bfm_sched_fill_kernel) and not bfm_sched_walk_kernel"""
    return bool(wc.dyadic_step(rate_triple(case["cfg"])))


def wraps(audio: np.ndarray) -> bool:
    """a jump across the int16 range between neighbours: the qint16 conversion wrapped"""
    a = audio.astype(np.int64)
    return a.shape[0] > 1 and int(np.abs(np.diff(a, axis=0)).max()) > 40000


def random_shares(cases, runs) -> dict:
    """the counts assert_random_shares() puts floors under; runs[i] is run_oracle() of cases[i]"""
    level = lambda c: np.float32(c["cfg"]["rf"]) / np.float32(20)
    closes = 0
    for c, r in zip(cases, runs):
        open_after = [np.float32(s["sq_state"]) > level(c) for s in r["states"]]
        closes += any(a and not all(open_after[i + 1:]) for i, a in enumerate(open_after[:-1]))
    steps = [np.float32(c["cfg"]["in_rate"]) / np.float32(c["cfg"]["audio_rate"]) for c in cases]
    return {"cases": len(cases), "stereo": sum(c["cfg"]["stereo"] for c in cases),
            "closed_form": sum(is_dyadic(c) for c in cases), "serial": sum(not is_dyadic(c) for c in cases),
            "other_audio_rate": sum(c["cfg"]["audio_rate"] != 48000 for c in cases), "step_near_1": sum(bool(s < np.float32(1.1)) for s in steps),
            "locked": sum(r["states"][-1]["locked"] == 1 for r in runs), "opens_then_closes": closes,
            "wraps": sum(wraps(np.concatenate(r["audio"])) for r in runs), "audible": sum(bool(np.concatenate(r["audio"]).any()) for r in runs),
            "probe": {k: sum(r["probe"][k] for r in runs) for k in PROBE},
            "sched_mismatch_cases": sum(r["probe"]["sched_mismatch"] != 0 for r in runs)}


def assert_random_shares(cases, runs) -> dict:
    """the floors of the draw.  They are conditions on the inputs: the lists above were tuned until the draw met them, never the
    floors to the draw"""
    s = random_shares(cases, runs)
    assert s["cases"] == 100 and [c["name"] for c in cases] == [f"random{i}" for i in range(100)], s
    assert s["stereo"] >= 55 and s["closed_form"] >= 20 and s["serial"] >= 20 and s["other_audio_rate"] >= 30 and s["step_near_1"] >= 5, s
    assert s["locked"] >= 5 and s["opens_then_closes"] >= 10 and s["wraps"] >= 5 and s["audible"] >= 80, s
    assert s["sched_mismatch_cases"] == 0 and all(v > 0 for k, v in s["probe"].items() if k != "sched_mismatch"), s
    assert all(2000 <= c["n"] <= 40000 or i % LOCK_EVERY == LOCK_AT for i, c in enumerate(cases)), "n outside 2000 .. 40000"
    assert all(len(c["splits"]) <= MAX_FEEDS and sum(c["splits"]) == c["n"] for c in cases)
    return s


def sha_bytes(a: np.ndarray) -> np.ndarray:
    import hashlib
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a, np.int16).tobytes()).digest(), np.uint8)


def pack_digests(cases, results, inputs_of=None) -> dict:
    """The random draw's fixture, from the recorder's results or the oracle's (run_oracle's layout): per case the feeds and the
    input's sha256; per feed the lengths and sha256 of audio and sink stream, m_magsqSum and m_magsqPeak as double bits,
    m_magsqCount, m_squelchState, locked(), m_lock_cnt, and the bits of m_pilot_level, m_freq, m_phase and both m_y1"""
    a = {k: [] for k in ("in_sha256", "feeds", "audio_counts", "sink_counts", "audio_sha256", "sink_sha256", "levels", "state", "bits")}
    for c, r in zip(cases, results):
        a["in_sha256"].append(sha_bytes((inputs_of or inputs)(c)))
        a["feeds"].append(len(r["audio"]))
        for au, sk, st in zip(r["audio"], r["sink"], r["states"]):
            a["audio_counts"].append(au.shape[0]); a["sink_counts"].append(sk.size)
            a["audio_sha256"].append(sha_bytes(au)); a["sink_sha256"].append(sha_bytes(sk))
            a["levels"].append(np.array([st["sum"], st["peak"]], np.float64).view(np.uint64))
            a["state"].append([st["count"], st["sq_state"], st["locked"], st["lock_cnt"]])
            a["bits"].append(np.asarray(st["bits"], np.uint32))
    return {"names": np.array([c["name"] for c in cases]), "in_sha256": np.array(a["in_sha256"], np.uint8).reshape(-1, 32),
            "feeds": np.array(a["feeds"], np.int32), "audio_counts": np.array(a["audio_counts"], np.int64),
            "sink_counts": np.array(a["sink_counts"], np.int64), "audio_sha256": np.array(a["audio_sha256"], np.uint8).reshape(-1, 32),
            "sink_sha256": np.array(a["sink_sha256"], np.uint8).reshape(-1, 32), "levels": np.array(a["levels"], np.uint64).reshape(-1, 2),
            "state": np.array(a["state"], np.int64).reshape(-1, 4), "bits": np.array(a["bits"], np.uint32).reshape(-1, 5)}


PER_CASE, PER_FEED = ("in_sha256", "feeds"), ("audio_counts", "sink_counts", "audio_sha256", "sink_sha256", "levels", "state", "bits")


def load_random_golden() -> dict:
    """bfm_random_golden.npz by case name, each entry as pack_digests packs a single case"""
    g = np.load(RANDOM_GOLDEN)
    out, f0 = {}, 0
    for i, name in enumerate(g["names"].tolist()):
        f1 = f0 + int(g["feeds"][i])
        out[name] = dict({k: g[k][i:i + 1] for k in PER_CASE}, **{k: g[k][f0:f1] for k in PER_FEED})
        f0 = f1
    out["host"] = str(g["host"])
    return out


def recorded_states(states) -> list[dict]:
    """the recorder's (levels, state, bits) triples as OracleBfm.state() gives them"""
    return [{"sum": float(lv[0]), "peak": float(lv[1]), "count": int(st[0]), "sq_state": int(st[1]), "locked": int(st[2]), "lock_cnt": int(st[3]),
             "bits": np.asarray(bits, np.uint32)} for lv, st, bits in states]


# ---------------------------------------------------------------- the fixture
def golden():
    return np.load(GOLDEN)


#: the fixture keeps a case's inputs in full up to this many samples, and its sink stream in full up to SINK_FULL; beyond, the
#: sha256 of the bytes (the inputs') or of every feed's (the sink stream's)
IN_FULL, SINK_FULL = 16384, 5000


def sha(a: np.ndarray) -> str:
    import hashlib
    return hashlib.sha256(np.ascontiguousarray(a, np.int16).tobytes()).hexdigest()


def golden_case(g, case: dict) -> dict:
    """the recording of a case in run_oracle's layout; `sink` is None where the fixture keeps `sink_sha`"""
    name = case["name"]
    ac, sc = g[f"{name}/audio_counts"], g[f"{name}/sink_counts"]
    audio = np.split(g[f"{name}/audio"], np.cumsum(ac)[:-1])
    sink = np.split(g[f"{name}/sink"], np.cumsum(sc)[:-1]) if f"{name}/sink" in g else None
    sink_sha = [str(v) for v in g[f"{name}/sink_sha256"]] if sink is None else [sha(s) for s in sink]
    lv, st, bits = g[f"{name}/levels"], g[f"{name}/state"], g[f"{name}/bits"]
    states = [{"sum": float(lv[i, 0]), "peak": float(lv[i, 1]), "count": int(st[i, 0]), "sq_state": int(st[i, 1]), "locked": int(st[i, 2]),
               "lock_cnt": int(st[i, 3]), "bits": bits[i]} for i in range(len(case["splits"]))]
    return {"in": g[f"{name}/in"] if f"{name}/in" in g else None, "in_sha": str(g[f"{name}/in_sha256"]), "audio": audio, "sink": sink,
            "sink_counts": [int(v) for v in sc], "sink_sha": sink_sha, "states": states}


def assert_equals_recording(got: dict, want: dict, what: str, state_keys=("count", "sq_state", "locked", "lock_cnt", "peak")):
    """audio, sink stream and state after every feed, bit for bit; got in run_oracle's layout, want in golden_case's"""
    assert [a.shape[0] for a in got["audio"]] == [a.shape[0] for a in want["audio"]], what
    assert [s.size for s in got["sink"]] == want["sink_counts"], what
    for i, (g, w) in enumerate(zip(got["audio"], want["audio"])):
        assert np.array_equal(g, w), (what, "audio of feed", i, int(np.count_nonzero(g != w)))
    for i, s in enumerate(got["sink"]):
        if want["sink"] is not None:
            assert np.array_equal(s, want["sink"][i]), (what, "sink stream of feed", i, int(np.count_nonzero(s != want["sink"][i])))
        assert sha(s) == want["sink_sha"][i], (what, "sink stream of feed", i)
    for i, (g, w) in enumerate(zip(got["states"], want["states"])):
        for k in state_keys:
            assert g[k] == w[k], (what, "feed", i, k, g[k], w[k])
        nb = len(g["bits"])
        assert np.array_equal(np.asarray(g["bits"], np.uint32), np.asarray(w["bits"], np.uint32)[:nb]), (what, "feed", i, g["bits"], w["bits"])
        # reordering n non-negative double terms moves the sum by at most n * 2^-53 relative, on either side
        assert abs(g["sum"] - w["sum"]) <= 2 * max(w["count"], 1) * 2.0 ** -53 * w["sum"], (what, "feed", i, g["sum"], w["sum"])
