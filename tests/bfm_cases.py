"""Cases of the broadcast-FM stereo demodulator bank (sdrx_bfm_*) and the ctypes face of tests/bfm_oracle.c, shared by
tests/test_bfm_oracle.py (CPU), tests/test_bfm_gpu.py and the golden recorder tests/golden/make_golden_bfm.py.

A case is a demodulator configuration, a signal at the channel rate and the lengths of the feeds it is cut into:
    cfg = dict(in_rate, nco_freq, audio_rate, rf, af, vol, sq, stereo, lsb, pilot)
    sig = {"kind": ...}   see signal(); "mpx" is a stereo multiplex (L+R, 19 kHz pilot, 38 kHz DSB-SC L-R) FM-modulated to int16 I/Q

The generator is wfm_cases' portable one (counter-based splitmix64 noise, a 32-bit integer phase accumulator)."""
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
