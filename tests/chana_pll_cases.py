"""Cases of the ChannelAnalyzer bank with its PLL / FLL (sdrx_chanapll_*) and the ctypes face of tests/chana_pll_oracle.c, shared by
tests/test_chana_pll_oracle.py (CPU), tests/test_chana_pll_gpu.py and tests/golden/make_golden_chana_pll.py.

A case is tests/chana_cases.py's (configuration, signal, feed lengths) with three more configuration fields (pll, fll, psk_order)
and two more kinds of signal: a tone that steps to another frequency at sample `at` (sig has step2), and a constant (sig has
const).  All run at in_rate 48000 unless the Interpolator is what they are about; the tone sits at in_rate / 16 = 3000 Hz, so
nco_freq decides the offset the loop sees.  Sizes are those of tests/chana_cases.py.

random_cases() are 100 more, for the wide banks of tests/test_chana_random_gpu.py: the signal is made for the channel, n is sized
in closed groups, and assert_random_shares holds the draw to floors counted on the oracle's probes."""
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
    L.chapo_seek.argtypes = [C.c_void_p, C.c_uint64]
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

    def seek(self, filtered_samples: int):
        """chao_seek of the inner handle; the loops do not depend on the position"""
        self.L.chapo_seek(self.h, filtered_samples)

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


# ---------------------------------------------------------------- random cases: the signal is made for the channel
RANDOM_SEED = 20261050
MAX_N = 64000
#: (pll, fll, input_type): the first FORCED cases run through them three times, the draw behind adds to the ones with a loop
COMBOS = [(p, f, t) for p in (1, 0) for f in (0, 1) for t in (SIGNAL, PLLOUT, AUTOCORR)]
FORCED = 3 * len(COMBOS)
ODD_ORDER = 3
_ORDERS = [1, 2, 4, 8, 16, ODD_ORDER]
_CUT_EDGES = (511, 512, 513, 1023, 1024, 1025, 4095, 4096, 4097)
#: signal kinds by what the channel runs: a PLL, an FLL (it only ever sees a frequency), no loop
_KINDS_PLL = ["tone"] * 6 + ["step"] * 9 + ["noisy"] * 9 + ["noise", "silence", "silence", "minus", "full"]
_KINDS_FLL = ["tone"] * 7 + ["silence", "minus", "noise"]
_KINDS_OFF = ["tone"] * 6 + ["noise", "noise", "minus", "full"]


def _draw_splits(rng, n: int, must=()) -> list[int]:
    """2 to 6 ragged feeds with one zero-length feed among them: the cuts in `must`, up to two drawn ones, for half of the cases
    one next to 512 / 1024 / 4096 +- 1, and for most a feed of 1 .. 200 inputs at the front, which closes no group"""
    cuts = {int(c) for c in must if 0 < c < n}
    for _ in range(int(rng.integers(0, 3 - min(len(cuts), 2)))):
        cuts.add(int(rng.integers(1, n)))
    edge, tiny = int(rng.choice(_CUT_EDGES)), int(rng.integers(1, 201))
    if rng.random() < 0.7 and len(cuts) < 4:
        cuts.add(tiny)
    if rng.random() < 0.5 and edge < n and len(cuts) < 4:
        cuts.add(edge)
    edges = sorted(cuts | {0, n})
    out = [b - a for a, b in zip(edges[:-1], edges[1:])]
    at = int(rng.integers(0, len(out) + 1))
    return out[:at] + [0] + out[at:]


def random_case(rng, i: int) -> dict:
    """one random configuration with a signal made for it and a split list; the order of the rng calls is part of the case set.
    The tone of tests/synth.mix sits at +-in_rate / 16, so nco_freq is chosen around it: the channel sees the tone at d hertz, on
    the side its filter passes, d a drawn fraction of the rate the loop runs at (smaller for a PSK order, which multiplies it;
    larger for the FLL, whose phase has to pass 120).  n is sized in closed groups."""
    pll, fll, input_type = COMBOS[i % len(COMBOS)] if i < FORCED else (
        int(rng.random() < 0.92), int(rng.random() < 0.25), int(rng.choice([SIGNAL, SIGNAL, SIGNAL, PLLOUT, PLLOUT, AUTOCORR, AUTOCORR])))
    corr = input_type == AUTOCORR
    in_rate = int(rng.choice([48000, 48000, 50000, 96000, 12345, 12345]))
    down = int(rng.random() < 0.3)
    ratio = float(rng.choice([1.0, 1.3, 2.0, 2.6, 3.7])) if down else 1.0
    ssb, rrc = int(rng.random() < 0.55), int(rng.random() < 0.3)
    neg = int(rng.random() < 0.5)                            # the bandwidth's sign: LSB with ssb
    if corr and down and neg:
        rrc = 0                                              # behind the Interpolator a negative bandwidth makes the RRC filter all zero
    short8 = (not corr) and rng.random() < 0.07
    span = int(rng.choice([0, 1, 2])) if corr else 8 if short8 else int(rng.choice([0, 0, 1, 2, 3, 4, 4, 5, 5, 5, 6]))
    if corr and down:
        ratio = min(ratio, [2.0, 1.3, 1.0][span])            # three blocks of 4096 groups within MAX_N inputs
    down_rate = int(in_rate / ratio)
    rate = down_rate if down else in_rate
    grp = rate / (1 << span)                                 # the rate the loop runs at
    loop = "pll" if pll and not fll else "fll" if pll else "off"
    # n in closed groups
    per = (1 << span) * (in_rate / down_rate if down else 1.0)
    if corr:
        groups = int(rng.integers(2 * 4096 + 100, 3 * 4096 + 601))
    elif span == 8:
        groups = int(rng.integers(100, 301))
    else:
        groups = int(rng.integers(1500, 12001))
        if loop != "off" and rng.random() < 0.7:
            groups = max(groups, int(rng.integers(7000, 12001)))      # long enough to pull in, lock and turn
    held = 2048 if not ssb else 1024                         # what the filter holds back, and its first block
    n = int(min(groups * per + held + 8, MAX_N))
    groups = min(groups, int((n - held) / per))
    kind = str(rng.choice({"pll": _KINDS_PLL, "fll": _KINDS_FLL, "off": _KINDS_OFF}[loop]))
    if corr and kind == "silence":
        kind = "tone"
    order = int(rng.choice([2, 4, 4, 4, 8, 8, 8, 16, 16, 16, 31, 31, ODD_ORDER])) if kind == "noisy" else int(rng.choice(_ORDERS + [1, 1]))
    if kind == "step" and rng.random() < 0.85:
        order = 1                                            # the order-1 detector drops the lock at the first step off the tone
    if i < FORCED and pll and kind != "noisy":
        order = _ORDERS[(i % len(COMBOS) + i // len(COMBOS)) % len(_ORDERS)]       # every order three times among the forced cases
    frac = float(rng.choice([0.00002, 0.0001, 0.0002, 0.0004, 0.0007, 0.001])) / (order if loop == "pll" else 1)
    if loop == "fll":                                        # the FLL's phase passes 120 (19 turns) well inside the case
        frac = min(max(float(rng.choice([0.004, 0.008, 0.015, 0.03])), 50.0 / groups), 0.2)
    side = -1 if (neg if ssb else rng.random() < 0.5) else 1
    step = int(rng.choice([1, 15]))
    tone_f = 0.0 if kind == "minus" else (in_rate / 16.0) * (1 if step == 1 else -1)
    d = side * max(frac * grp, 0.4)
    nco = int(round(d - tone_f))
    if nco + tone_f == 0.0:
        nco += side
    d = abs(nco + tone_f)
    band = int(max(rng.integers(rate // 20, rate // 4), 4 * d + 200))
    if kind == "step":
        band = max(min(in_rate // 12, rate // 4), int(4 * d + 200))  # the other side, in_rate / 8 away, is outside a DSB filter too; wide, so that
                                                                     # the noise left behind the step does not look like a carrier
    low = int(rng.choice([0, 0, 50, 300]))
    sig = {"tone": dict(amp=int(rng.integers(3, 60)), tone=8000, step=step),
           "step": dict(amp=int(rng.integers(3, 60)), tone=8000, step=step, step2=16 - step, at=int(n * rng.uniform(0.6, 0.8))),
           "noisy": dict(amp=int(rng.integers(3000, 9000)), tone=3000, step=step),
           "noise": dict(amp=20000, tone=0, step=1), "silence": dict(amp=0, tone=0, step=1), "minus": dict(const=-32768),
           "full": dict(amp=32767, tone=30000, step=step)}[kind]
    must = []
    if kind == "step":
        # a feed ends on the last sample of the tone, the next right behind the block the step comes out in: locked, then lost
        must += [sig["at"], sig["at"] + int(0.75 * held * per / (1 << span)) + int(rng.integers(0, 64))]
    if corr and rng.random() < 0.45:                         # one feed that completes two blocks of 4096 calls
        a = int(rng.integers(1, 600))
        must += [a, a + int(2 * 4096 * per) + held + int(rng.integers(0, 300))]
    if span >= 4 and rng.random() < 0.75:                    # a feed that ends inside the filter's second block: one block's groups, 2 .. 32
        must.append(int((held // 2) * per / (1 << span)) + int(rng.integers(40, 120)))
    cfg = _cfg(in_rate, nco_freq=nco, down_sample=down, down_sample_rate=down_rate if down else int(rng.integers(0, 2)) * 24000,
               bandwidth=-band if neg else band, low_cutoff=low, span_log2=span, ssb=ssb, rrc=rrc, rrc_rolloff=int(rng.integers(0, 101)),
               input_type=input_type, pll=pll, fll=fll, psk_order=order)
    return {"name": f"random{i}_{loop}_{kind}", "seed": 7000 + i, "n": n, "sig": sig, "cfg": cfg, "splits": _draw_splits(rng, n, must)}


def random_cases(count: int = 100) -> list[dict]:
    """the first `count` cases, the forced combinations included, drawn in order from one generator"""
    rng = np.random.default_rng(RANDOM_SEED)
    cases = [random_case(rng, i) for i in range(count)]
    for c in cases:
        assert sum(c["splits"]) == c["n"] <= MAX_N and 2 <= len(c["splits"]) <= 6 and 0 in c["splits"], c["name"]
    return cases


def run_case(L: C.CDLL, case: dict) -> dict:
    return run_oracle(L, case["cfg"], cut(inputs(case), case["splits"]))


#: the floors of assert_random_shares: conditions on the inputs.  In brackets what the issue of this test set
#: asked for where the draw gives more
FLOORS = {"each_combo": 3, "each_order": 5, "interpolator": 20, "span_ge_1": 40, "span_ge_4": 10, "autocorr": 20, "autocorr_behind_loop": 8,
          "two_blocks_at_once": 5, "locked": 30, "lock_lost": 8, "sat_hi": 12, "sat_lo": 12, "turns_many": 15, "big_arg": 12, "arg_zero": 5,
          "loop_feed_no_group": 30, "feed_1_to_63": 20, "feed_ragged_above_64": 20, "feed_multiple_of_64": 5, "rate_12345": 5}


def random_shares(cases: list[dict], results: list[dict]) -> dict:
    """what the draw reaches, counted on the oracle's probes, per-feed output counts and states (results[i] = run_case(L, cases[i]))"""
    both = list(zip(cases, results))
    cfg = lambda c: c["cfg"]
    counts = lambda r: [o.shape[0] for o in r["out"]]
    locked = lambda r: [s[0] for s in r["states"]]
    sh = {"each_combo": min(sum(1 for c in cases if (cfg(c)["pll"], cfg(c)["fll"], cfg(c)["input_type"]) == k) for k in COMBOS),
          "each_order": min(sum(1 for c in cases if cfg(c)["pll"] and cfg(c)["psk_order"] == m) for m in (1, 2, 4, 8, 16, ODD_ORDER)),
          "interpolator": sum(1 for c in cases if cfg(c)["down_sample"]),
          "span_ge_1": sum(1 for c in cases if cfg(c)["span_log2"] >= 1), "span_ge_4": sum(1 for c in cases if cfg(c)["span_log2"] >= 4),
          "rate_12345": sum(1 for c in cases if cfg(c)["in_rate"] == 12345)}
    ac = [(c, r) for c, r in both if cfg(c)["input_type"] == AUTOCORR]
    sh["autocorr"] = len(ac)
    sh["autocorr_behind_loop"] = sum(1 for c, _ in ac if cfg(c)["pll"])
    blocks = lambda r: np.diff(np.concatenate([[0], np.cumsum(counts(r)) // 4096]))
    sh["two_blocks_at_once"] = sum(1 for _, r in ac if blocks(r).max() >= 2)
    sh["locked"] = sum(1 for _, r in both if any(locked(r)))
    sh["lock_lost"] = sum(1 for _, r in both if 1 in locked(r) and 0 in locked(r)[locked(r).index(1):])
    for k in ("sat_hi", "sat_lo", "turns_many", "big_arg", "arg_zero"):
        sh[k] = sum(1 for _, r in both if r["probe"][k] > 0)
    sh["loop_feed_no_group"] = sum(1 for c, r in both if cfg(c)["pll"] and any(m > 0 and k == 0 for m, k in zip(c["splits"], counts(r))))
    sh["feed_1_to_63"] = sum(1 for _, r in both if any(1 <= k <= 63 for k in counts(r)))
    sh["feed_ragged_above_64"] = sum(1 for _, r in both if any(k > 64 and k % 64 for k in counts(r)))
    sh["feed_multiple_of_64"] = sum(1 for _, r in both if any(k > 0 and k % 64 == 0 for k in counts(r)))
    return sh


def assert_random_shares(cases: list[dict], results: list[dict]) -> dict:
    sh = random_shares(cases, results)
    print("random shares:", sh)
    for k, floor in FLOORS.items():
        assert sh[k] >= floor, (k, sh[k], floor)
    # every autocorrelation case completes two blocks and returns something behind the 4095 leading zeros
    for c, r in zip(cases, results):
        if c["cfg"]["input_type"] == AUTOCORR:
            full = np.concatenate(r["out"])
            assert full.shape[0] >= 2 * 4096 and full[4095:].any() and not full[:4095].any(), c["name"]
    return sh
