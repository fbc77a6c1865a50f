"""Cases of the AM demodulator bank's synchronous-AM channels (sdrx_am_create_ex), shared by the golden recorder
tests/golden/make_golden_am_sync.py, tests/test_am_sync_gpu.py and tests/test_am_sync_host.py; the ctypes face of the synchronous
branch of tests/am_oracle.c (build_oracle, OracleAmSync, run_oracle); and the random draw (random_cases, assert_random_shares) of
tests/test_am_sync_oracle.py and tests/test_am_sync_random_gpu.py.

A case is a demodulator configuration, its sync options, a signal at the channel rate and the lengths of the feeds it is cut into:
    cfg  = (in_rate, nco_freq, audio_rate, rf_bandwidth, volume, squelch_db, audio_mute, bandpass_enable)     as tests/am_cases.py
    sync = (pll, sync_op, ssb_design_rate, ssb_design_bw)       sync_op 0 DSB, 1 USB, 2 LSB; the two design values as SSBFilter got them
    sig  = {"kind": ...}   see signal()

The `am2` signal is a carrier at f0 whose two sidebands carry different tones (fu above, fl below, different depths), so that a
swapped sideband changes the audio, and whose amplitude follows a list of runs.  Rates are low (4 to 8 kS/s audio) so that the
squelch opens after a few hundred samples, the AGC history (rate / 4) fills, and six to twelve filter blocks fit in under 10 000
audio samples.  The expectations (`locked`, `reopens`, `never_open`, `sat`) are asserted by the recorder's maker on the recording
itself."""
from __future__ import annotations

import ctypes as C
import hashlib

import numpy as np

from tests import am_cases as _ac
from tests.am_cases import _amp_runs
from tests.wfm_cases import _clip16, _gauss, _uniform_i16, cut  # noqa: F401  (cut is re-exported)

DSB, USB, LSB = 0, 1, 2
OPS = ("dsb", "usb", "lsb")


def block(sync_op: int) -> int:
    return 1024 if sync_op == DSB else 512


def signal(sig: dict, n: int, rate: int, seed: int) -> np.ndarray:
    kind = sig["kind"]
    iq = np.empty(2 * n, np.int16)
    if kind == "noise_full":
        iq[0::2] = _uniform_i16(seed, n, 1)
        iq[1::2] = _uniform_i16(seed, n, 2)
    elif kind == "am2":
        t = np.arange(n, dtype=np.float64)
        inc = int(round(sig.get("f0", 0.0) / rate * 4294967296.0))
        ph = ((np.arange(1, n + 1, dtype=np.int64) * inc) & 0xFFFFFFFF).astype(np.float64) * (2 * np.pi / 4294967296.0)
        amp = _amp_runs(n, sig["runs"], sig["amps"]) if "runs" in sig else np.full(n, float(sig.get("amp", 6000.0)))
        up = float(sig.get("du", 0.45)) * np.exp(2j * np.pi * float(sig.get("fu", 400.0)) * t / rate)
        lo = float(sig.get("dl", 0.25)) * np.exp(-2j * np.pi * float(sig.get("fl", 650.0)) * t / rate)
        z = amp * np.exp(1j * ph) * (1.0 + up + lo)
        sg = float(sig.get("noise", 10.0))
        iq[0::2] = _clip16(z.real + _gauss(seed, n, 3, sg))
        iq[1::2] = _clip16(z.imag + _gauss(seed, n, 4, sg))
        if "zero_at" in sig:                           # a stretch of exact zeros
            a, m = sig["zero_at"]
            iq[2 * a: 2 * (a + m)] = 0
    else:
        raise ValueError(kind)
    return iq


def _cfg(in_rate, audio_rate, nco_freq=0, rf=3000.0, vol=1.0, sq=-40.0, mute=0, bp=0):
    return (in_rate, nco_freq, audio_rate, rf, vol, sq, mute, bp)


def _ragged(n: int, seed: int) -> list[int]:
    """feed lengths adding up to n: empty and one-sample feeds, spans shorter and longer than a block"""
    rng = np.random.default_rng(seed)
    out, left = [], n
    head = [1, 0, 2, 100, 101, 0, 333]
    k = 0
    while left > 0:
        m = head[k] if k < len(head) else int(rng.choice([0, 1, 7, int(rng.integers(1, 300)), int(rng.integers(1, 1500)), int(rng.integers(1, 4000))]))
        m = min(m, left)
        out.append(m); left -= m; k += 1
    return out


def make_cases() -> list[dict]:
    cases = []

    def add(name, cfg, sync, sig, n, splits=None, **expect):
        seed = 100 + len(cases)
        cases.append({"name": name, "cfg": cfg, "sync": sync, "sig": sig, "n": n, "seed": seed, "splits": splits or _ragged(n, seed), "expect": expect})

    am2 = lambda f0, **kw: dict({"kind": "am2", "f0": f0}, **kw)
    # the three operations at the three carrier offsets, Bandpass on and off, three audio rates, in_rate equal to it or twice it.  -170 Hz
    # (and +30 Hz, later) takes the loop's phase past two pi: the saturation branches
    add("dsb_0", _cfg(8000, 8000), (1, DSB, 0, 0.0), am2(0.0), 9000, locked=True)
    add("usb_0_bp", _cfg(8000, 8000, bp=1), (1, USB, 0, 0.0), am2(0.0), 7000, locked=True)
    add("lsb_0", _cfg(12000, 6000, nco_freq=-1500), (1, LSB, 0, 0.0), am2(1500.0), 14000, locked=True)
    add("dsb_p30_bp", _cfg(16000, 8000, nco_freq=-2000, bp=1), (1, DSB, 0, 0.0), am2(2030.0), 19000, sat=True)
    add("usb_p30", _cfg(6000, 6000), (1, USB, 0, 0.0), am2(30.0), 7000, sat=True)
    add("lsb_p30_bp", _cfg(6000, 6000, bp=1), (1, LSB, 0, 0.0), am2(30.0), 6000, sat=True)
    add("dsb_m170", _cfg(4000, 4000, rf=2000.0), (1, DSB, 0, 0.0), am2(-170.0, fu=250.0, fl=420.0), 7000, sat=True)
    add("usb_m170_bp", _cfg(12000, 6000, nco_freq=1000, bp=1), (1, USB, 0, 0.0), am2(-1170.0), 12000, sat=True)
    add("lsb_m170", _cfg(8000, 8000), (1, LSB, 0, 0.0), am2(-170.0), 7000, sat=True)
    # SSBFilter designed once from other values than the channel's: the same stream through a filter made from the channel's own
    add("usb_design_default", _cfg(8000, 8000, vol=2.0), (1, USB, 0, 0.0), am2(0.0, fu=900.0, fl=300.0), 6000)
    add("usb_design_own", _cfg(8000, 8000, vol=2.0), (1, USB, 8000, 3000.0), am2(0.0, fu=900.0, fl=300.0), 6000)
    # squelch gating: a closure in the middle of a block and a reopening; muted; never open
    gap = am2(0.0, runs=[3000, 1500, 4500], amps=[6000.0, 20.0])
    add("usb_reopen", _cfg(8000, 8000), (1, USB, 0, 0.0), gap, 9000, reopens=True)
    add("dsb_reopen_bp", _cfg(8000, 8000, bp=1), (1, DSB, 0, 0.0), am2(30.0, runs=[2500, 1200, 5300], amps=[6000.0, 20.0]), 9000, reopens=True)
    add("lsb_muted", _cfg(8000, 8000, mute=1), (1, LSB, 0, 0.0), am2(0.0), 3000, never_open=True)
    add("dsb_never_open", _cfg(8000, 8000, sq=-10.0), (1, DSB, 0, 0.0), am2(0.0, amp=300.0), 3000, never_open=True)
    add("usb_noise", _cfg(8000, 8000, sq=-100.0), (1, USB, 0, 0.0), {"kind": "noise_full"}, 5000, locked=False)
    # block edges: a constant-amplitude carrier from the first sample with the squelch at -100 dB opens at audio index rate / 20 - 1 (the
    # counter reaches rate / 20 on the 400th sample), so 399 inputs bring no open sample and the feeds behind them are all open: a feed
    # shorter than a block, one of exactly B, B - 1, B + 1
    for op in (USB, DSB):
        B = block(op)
        edges = [399, 100, B - 100, B, B - 1, B + 1, 1, B - 1, 3]
        add(f"{OPS[op]}_block_edges", _cfg(8000, 8000, sq=-100.0), (1, op, 0, 0.0), am2(0.0, noise=0.0), sum(edges) + B + 77, splits=edges + [B + 77],
            edges=True)
    # the host check's trace (tests/test_am_sync_host.py): short, so that the per-sample recording stays small
    add("trace_usb_m170", _cfg(4000, 4000, rf=2000.0), (1, USB, 0, 0.0), am2(-170.0, fu=250.0, fl=420.0), 2500, trace=True, sat=True)
    for c in cases:
        assert sum(c["splits"]) == c["n"], c["name"]
        assert c["n"] <= 20000
    return cases


CASES = make_cases()
BY = {c["name"]: c for c in CASES}


def inputs(case: dict) -> np.ndarray:
    return signal(case["sig"], case["n"], case["cfg"][0], case["seed"])


def sha(a: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


# ---------------------------------------------------------------- oracle
SYNC_PROBES = ("open", "blocks", "reopenings", "closures_inside", "sat_hi", "sat_lo", "lock_up", "lock_down", "feeds_no_block", "feeds_on_edge",
               "wrapped", "bad", "nonfinite")


def build_oracle() -> C.CDLL:
    """tests/am_oracle.c as tests/am_cases.py builds it, with the faces of the synchronous branch"""
    L = _ac.build_oracle()
    L.amo_create_ex.restype = C.c_void_p
    L.amo_create_ex.argtypes = [C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float]
    L.amo_pll.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_float)]
    L.amo_sync_design.restype = C.c_int
    L.amo_sync_design.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.c_void_p]
    L.amo_sync_probe.argtypes = [C.c_void_p, C.c_void_p]
    L.amo_trace.restype = C.c_int
    L.amo_trace.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p]
    return L


class OracleAmSync(_ac.OracleAm):
    def __init__(self, L: C.CDLL, cfg, sync=(0, 0, 0, 0.0)):
        self.L = L
        self.cfg, self.sync = cfg, sync
        self.h = L.amo_create_ex(int(cfg[0]), int(cfg[1]), int(cfg[2]), float(cfg[3]), float(cfg[4]), float(cfg[5]), int(cfg[6]), int(cfg[7]),
                                 int(sync[0]), int(sync[1]), int(sync[2]), float(sync[3]))
        assert self.h

    def pll(self):
        locked, freq = C.c_int(), C.c_float()
        self.L.amo_pll(self.h, C.byref(locked), C.byref(freq))
        return bool(locked.value), float(freq.value)

    def sync_design(self):
        """(taps, filter, coef) in the layout of AmDemodBank.sync_design"""
        taps, filt, coef, flen = np.zeros(51, np.float32), np.zeros(2 * 2048, np.float32), np.zeros(5, np.float32), C.c_int()
        assert self.L.amo_sync_design(self.h, taps.ctypes.data, filt.ctypes.data, C.byref(flen), coef.ctypes.data) == 0
        return taps, filt[: 2 * flen.value].copy(), coef

    def sync_probe(self) -> dict:
        out = np.zeros(len(SYNC_PROBES), np.int64)
        self.L.amo_sync_probe(self.h, out.ctypes.data)
        return dict(zip(SYNC_PROBES, (int(v) for v in out)))

    def trace(self, path: str, path_sb: str):
        assert self.L.amo_trace(self.h, path.encode(), path_sb.encode()) == 0


def run_oracle(L: C.CDLL, case: dict, splits=None, trace=None, x=None) -> dict:
    """tests/am_cases.run_oracle's result plus, per feed, `levels` (magsq, sum, peak), `state` (count, open, squelch count, locked, bits
    of freq) and `opens`, as the recording has them, the sync probe and, for a sync case, the design"""
    o = OracleAmSync(L, case["cfg"], case["sync"])
    if trace:
        o.trace(*trace)
    design = o.sync_design() if case["sync"][0] else None
    feeds, levels, state, opens = [], [], [], []
    for part in cut(inputs(case) if x is None else x, splits or case["splits"]):
        feeds.append(o.feed(part))
        m, s, p, n = o.levels()
        locked, freq = o.pll()
        levels.append((m, s, p))
        state.append((n, int(o.squelch_open()), o.squelch_count(), int(locked), int(np.float32(freq).view(np.uint32))))
        opens.append(o.sync_probe()["open"])
    m, s, p, n = o.levels()
    res = {"feeds": feeds, "magsq": m, "sum": s, "peak": p, "count": n, "open": o.squelch_open(), "state": np.array(state, np.int64).reshape(-1, 5),
           "levels": np.array(levels, np.float64).reshape(-1, 3), "opens": np.array(opens, np.int64), "probe": o.probe(), "sync_probe": o.sync_probe(),
           "pll": o.pll(), "design": design}
    o.close()                                               # closes the trace files too
    return res


# ---------------------------------------------------------------- random cases
#: the seed of random_cases(): the cases tests/test_am_sync_oracle.py proves against the reference and tests/golden/am_sync_random_golden.npz records
RANDOM_SEED = 20261021
#: (in_rate, audio_rate): the AGC history rate / 4 is 250 (shorter than both blocks), 1000 to 2000, 8000, 11025 and 12000
RATES = [(1000, 1000), (16000, 1000), (4000, 4000), (12000, 6000), (48000, 8000), (48000, 32000), (96000, 44100), (50000, 44100), (48000, 48000),
         (62500, 48000), (60000, 48000), (120000, 48000)]
MAX_N = 80000
#: cases no longer than this feed the wide bank (`short`)
WIDE_N = 16000
FORCED = 12


def agc_len(audio_rate: int) -> int:
    return audio_rate // 4


def _to_in(audio_samples: int, in_rate: int, audio_rate: int) -> int:
    return -(-audio_samples * in_rate // audio_rate)


def _draw_splits(rng, n: int, B: int, head=()) -> list[int]:
    """feed lengths adding up to n: empty, one- and two-sample feeds, a block and its neighbours, short and long spans; after 40 feeds
    only long ones, so that a bank's rounds stay few"""
    splits, left = [], n
    for m in head:
        m = min(m, left)
        splits.append(m); left -= m
    while left > 0:
        small = int(rng.choice([0, 1, 2, B - 1, B, B + 1, int(rng.integers(1, 300)), int(rng.integers(1, 3000)), int(rng.integers(1, 30000))]))
        m = min(left, small if len(splits) < 40 else int(rng.integers(3000, 30000)))
        splits.append(m); left -= m
    return splits


def forced_case(rng, i: int) -> dict:
    """case i of the forced head: operation i % 3 at 1000 S/s (from 1000 and from 16000), at 48000 S/s and at 44100 S/s from 96000, a
    carrier that drops below the squelch level in the middle of a block for longer than the squelch takes to close, and comes back"""
    in_rate, audio = [(1000, 1000), (16000, 1000), (48000, 48000), (96000, 44100)][i // 3]
    op = i % 3
    B, hn = block(op), agc_len(audio)
    first = audio // 10 + 2 * B + B // 2                     # audio samples: the counter at its cap, the closure half-way into a block
    gap = audio // 10 + audio // 40
    rest = max(hn + 3 * B, 10 * B + audio // 20 - first) if audio > 1000 else 8 * B
    n = min(_to_in(first + gap + rest, in_rate, audio), MAX_N)
    if n == MAX_N:                                           # 16000 to 1000: what fits
        first = audio // 10 + B + B // 2
    runs = [_to_in(first, in_rate, audio), _to_in(gap, in_rate, audio), n]
    f0 = [0.0, 30.0, -170.0][op] if audio > 1000 else [0.0, 3.0, -17.0][op]
    sig = {"kind": "am2", "f0": f0, "fu": audio / 20.0, "fl": audio / 12.5, "runs": runs, "amps": [6000.0, 20.0], "noise": 10.0}
    cfg = (in_rate, 0, audio, 3000.0 if audio <= 8000 else 5000.0, 0.25 if audio > 8000 else 20.0, -40.0, 0, int(i % 2) if audio > 8000 else 0)
    head = [1, 0, 2, B - 1, B, B + 1]
    return {"name": f"forced{i}_{OPS[op]}_{audio}", "cfg": cfg, "sync": (1, op, 0, 0.0), "sig": sig, "n": n, "seed": 5000 + i,
            "splits": _draw_splits(rng, n, B, head), "expect": {}}


def random_case(rng, i: int) -> dict:
    """one random configuration, signal and split list; the order of the rng calls is part of the case set"""
    if i < FORCED:
        return forced_case(rng, i)
    same = [r for r in RATES if r[0] == r[1]]                # a third of the draws from these: only they can be `aligned` (below)
    in_rate, audio = same[int(rng.integers(len(same)))] if rng.random() < 0.35 else RATES[int(rng.integers(len(RATES)))]
    op = int(rng.integers(3))
    pll = int(rng.random() >= 0.2)
    B, hn = block(op), agc_len(audio)
    kind = str(rng.choice(["am2", "am2", "am2", "burst", "burst", "burst", "noise_full", "gap", "quiet"]))
    aligned = in_rate == audio and kind != "quiet" and bool(rng.random() < 0.7)
    offset = float(rng.choice([0.0, 0.0, 0.0, 0.0, 5.0, 30.0, -30.0, 17.0, -45.0, 170.0, -170.0, 400.0, -333.0])) * (audio / 8000.0 if audio < 8000 else 1.0)
    nco = int(rng.integers(-in_rate // 8, in_rate // 8)) if in_rate > audio else 0
    rf = float(rng.choice([3000.0, 5000.0, 8330.0, 2000.0, 10000.0]))
    if audio >= 32000:
        vol = float(rng.choice([0.1, 0.25, 0.5, 0.5, 1.0]))
    else:
        vol = float(rng.choice([0.5, 1.0, 2.0, 3.0])) * (8000 // audio)     # the audio scale is rate / 24: 41 at 1000 S/s
    sq = float(rng.choice([-100.0, -60.0, -40.0, -25.5, -10.0]))
    mute = int(rng.random() < 0.04)
    bp = int(rng.random() < 0.4)
    design_rate = int(rng.choice([0, 8000, 44100, 48000]))
    design_bw = float(rng.choice([0.0, 2400.0, 3000.0, 5000.0]))
    long = bool(rng.random() < 0.6)
    if long:                                                 # the AGC history wraps after the squelch opens, or ten blocks at 1000 S/s
        audio_n = (audio // 20 + hn + int(rng.integers(2, 6)) * B + int(rng.integers(B))) if audio > 1000 else 10 * B + 50 + int(rng.integers(B))
        n = min(_to_in(audio_n, in_rate, audio), MAX_N)
    else:
        n = int(rng.integers(WIDE_N // 2, WIDE_N + 1))
    sig = {"kind": "noise_full"} if kind == "noise_full" else {
        "kind": "am2", "f0": offset - nco, "fu": float(rng.integers(audio // 40, audio // 8)), "fl": float(rng.integers(audio // 40, audio // 8)),
        "du": float(rng.choice([0.45, 0.2, 0.7])), "dl": float(rng.choice([0.25, 0.0, 0.1])), "amp": float(rng.integers(3000, 12000)),
        "noise": float(rng.integers(0, 40))}
    head = [1, 0, 2]
    if kind == "burst":
        sig["runs"] = [int(v) for v in rng.integers(in_rate // 8, max(in_rate // 8 + 1, min(in_rate // 2, n // 3)), size=6)]
        sig["amps"] = [sig.pop("amp"), float(rng.integers(1, 25))]
        if sq == -100.0:
            sq = -40.0
    elif kind == "gap":
        sig["noise"] = 0.0
        sig["zero_at"] = (int(rng.integers(n // 2, n)), int(rng.integers(1, 200)))
    elif kind == "quiet":
        sig["amp"] = float(rng.integers(50, 250))
        sq = float(rng.choice([-25.5, -10.0]))
    if kind in ("am2", "gap", "burst") and sq == -10.0:      # -10 dB keeps all but the strongest carriers shut: `quiet` has those
        sq = -40.0
    if aligned:
        # with in_rate equal to audio_rate every input gives an audio sample, and at -100 dB any signal opens the squelch on audio
        # sample rate / 20 - 1 (as the block_edges cases above) and keeps it open: the second feed ends on a block boundary
        sq, mute = -100.0, 0
        head = [audio // 20 - 1, B, B - 1, 1, B + 1]
    cfg = (in_rate, nco, audio, rf, vol, sq, mute, bp)
    return {"name": f"random{i}", "cfg": cfg, "sync": (pll, op, design_rate, design_bw), "sig": sig, "n": n, "seed": 5000 + i,
            "splits": _draw_splits(rng, n, B, head), "expect": {}}


def random_cases(count: int = 100) -> list[dict]:
    """the first `count` cases, the forced head included, drawn in order from one generator"""
    rng = np.random.default_rng(RANDOM_SEED)
    cases = [random_case(rng, i) for i in range(count)]
    for c in cases:
        assert sum(c["splits"]) == c["n"] <= MAX_N, c["name"]
    return cases


def short(cases: list[dict]) -> list[dict]:
    """the cases short enough for the wide bank"""
    return [c for c in cases if c["n"] <= WIDE_N]


def hn_class(case: dict) -> str:
    B, hn = block(case["sync"][1]), agc_len(case["cfg"][2])
    return "below" if hn < B else "one_to_two" if B <= hn <= 2 * B else "above_eight" if hn > 8 * B else "between"


#: the floors of assert_random_shares: conditions on the inputs, see DESIGN.md 4.10
FLOORS = {"sync": 75, "envelope": 15, "each_op": 20, "three_blocks": 60, "close_inside_reopen": 15, "never_open": 10, "wrapped": 10, "hn_below_block": 8,
          "end_locked": 20, "end_unlocked": 20, "sat_hi": 10, "sat_lo": 10, "feed_no_block": 30, "feed_on_edge": 10, "in_range": 70, "short": 40,
          "audible": 55}


def random_shares(cases: list[dict], runs: list[dict]) -> dict:
    """what the draw reaches, counted on the oracle's probes (runs[i] = run_oracle(L, cases[i]))"""
    sync = [(c, r) for c, r in zip(cases, runs) if c["sync"][0]]
    sp = lambda r: r["sync_probe"]
    sh = {"sync": len(sync), "envelope": len(cases) - len(sync)}
    for op in range(3):
        sh[OPS[op]] = sum(1 for c, _ in sync if c["sync"][1] == op)
    sh["each_op"] = min(sh[o] for o in OPS)
    sh["three_blocks"] = sum(1 for _, r in sync if sp(r)["blocks"] >= 3)
    sh["close_inside_reopen"] = sum(1 for _, r in sync if sp(r)["closures_inside"] >= 1 and sp(r)["reopenings"] >= 1)
    sh["never_open"] = sum(1 for _, r in sync if sp(r)["open"] == 0)
    sh["wrapped"] = sum(1 for _, r in sync if sp(r)["wrapped"] > 0)
    sh["hn_below_block"] = sum(1 for c, _ in sync if hn_class(c) == "below")
    sh["end_locked"] = sum(1 for _, r in sync if r["pll"][0])
    sh["end_unlocked"] = sum(1 for _, r in sync if not r["pll"][0])
    sh["sat_hi"] = sum(1 for _, r in sync if sp(r)["sat_hi"] > 0)
    sh["sat_lo"] = sum(1 for _, r in sync if sp(r)["sat_lo"] > 0)
    sh["feed_no_block"] = sum(1 for _, r in sync if sp(r)["feeds_no_block"] > 0)
    sh["feed_on_edge"] = sum(1 for _, r in sync if sp(r)["feeds_on_edge"] > 0)
    sh["in_range"] = sum(1 for _, r in sync if sp(r)["bad"] == 0)
    sh["out_of_range"] = sh["sync"] - sh["in_range"]
    sh["nonfinite"] = sum(1 for _, r in sync if sp(r)["nonfinite"] > 0)
    sh["short"] = len(short(cases))
    sh["audible"] = sum(1 for _, r in sync if any(f.any() for f in r["feeds"]))
    return sh


def assert_random_shares(cases: list[dict], runs: list[dict]) -> dict:
    sh = random_shares(cases, runs)
    print("random shares:", sh)
    print(f"{sh['out_of_range']} sync cases hold a sample outside the int16 range before the conversion (to_q16's ruling is what is compared), "
          f"{sh['nonfinite']} of them a non-finite one")
    for k, floor in FLOORS.items():
        assert sh[k] >= floor, (k, sh[k], floor)
    # the forced head: every one closes inside a block and reopens, whatever the draw behind it does
    for c, r in list(zip(cases, runs))[:FORCED]:
        assert c["name"].startswith("forced") and r["sync_probe"]["closures_inside"] >= 1 and r["sync_probe"]["reopenings"] >= 1, c["name"]
    # the wide bank's subset holds every operation in each regime of the AGC history, and envelope channels
    have = {(c["sync"][1], hn_class(c)) for c in short(cases) if c["sync"][0]}
    for op in range(3):
        for cls in ("below", "one_to_two", "above_eight"):
            assert (op, cls) in have, (OPS[op], cls)
    assert any(not c["sync"][0] for c in short(cases))
    return sh
