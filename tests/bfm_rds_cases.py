"""Cases of RDS in the broadcast-FM bank (sdrx_bfmrds_create), shared by the golden recorder tests/golden/make_golden_bfm_rds.py,
tests/test_bfm_rds_gpu.py and the CPU tests.

A case is bfm_cases' (cfg, sig, n, seed, splits) plus `rds` (m_rdsActive).  The signal kind "mpx" of bfm_cases gains a 57 kHz
subcarrier: BPSK on the pilot's third harmonic at phase `rds_phi`, deviation `rds` Hz, carrying `rds_groups` (four 16-bit
blocks each, repeated for the length of the signal) with checkwords by the polynomial 0x5B9 plus the offset words,
differentially coded, as biphase symbols at 1187.5 Hz.  `lead` samples of unmodulated carrier come first.

Also the synthetic bit streams of the frameSync fixtures (framesync_streams) and the order of the recorded state words.

random_cases() is the draw of 40 configurations with RDS on that tests/test_bfm_rds_random_gpu.py runs against the recording
tests/golden/bfm_rds_random_golden.npz (pack_random() is its layout, load_random_golden() reads it back in golden_case()'s).  Its
bursting cases keep the named case's rf of 12500, so that the squelch can open inside a short case; every other case has rf of at
least 180000 where the rate allows."""
from __future__ import annotations

import os

import numpy as np

from tests import bfm_cases as bc
from tests import wfm_cases as wc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "bfm_rds_golden.npz")

#: the recorder's state words, in its order; *: float or double bits
STATE_FIELDS = ("subcarr_phi", "clock_offset", "clock_phi", "prev_clock_phi", "d_cphi", "xv0", "xv1", "xv2", "yv0", "yv1", "yv2",
                "prev_bb", "acc", "prev_acc", "lo_clock", "prev_lo_clock", "numsamples", "counter", "reading_frame", "tot_errs0",
                "tot_errs1", "dbit", "distance_remain", "mix_phase", "n_rds", "reg", "lastseen_offset_counter", "bit_counter",
                "block_bit_counter", "wrong_blocks_counter", "blocks_counter", "group_good_blocks_counter", "group0", "group1",
                "group2", "group3", "sync", "presync", "lastseen_offset", "block_number", "group_assembly_started", "good_block",
                "decoder_qua")
BB_FULL, BB_EDGE = 20000, 64

OFFSET_WORD = (252, 408, 360, 436, 848)            # A, B, C, D, C'


# ---------------------------------------------------------------- RDS coding
def syndrome(message: int, mlen: int) -> int:
    """Annex B of the standard: the remainder by x^10 + x^8 + x^7 + x^5 + x^4 + x^3 + 1 (0x5B9)"""
    reg = 0
    for i in range(mlen, 0, -1):
        reg = (reg << 1) | ((message >> (i - 1)) & 1)
        if reg & 0x400:
            reg ^= 0x5B9
    for _ in range(10):
        reg <<= 1
        if reg & 0x400:
            reg ^= 0x5B9
    return reg & 0x3FF


def block_bits(data: int, offset: int) -> list[int]:
    word = ((data & 0xFFFF) << 10) | (syndrome(data & 0xFFFF, 16) ^ OFFSET_WORD[offset])
    return [(word >> (25 - i)) & 1 for i in range(26)]


def group_bits(blocks, cprime: bool = False) -> list[int]:
    out = []
    for i, d in enumerate(blocks):
        out += block_bits(d, 4 if (i == 2 and cprime) else i)
    return out


#: a 0A group (PI 0xD314, PS segment), a 2A group (radio text), a 0B group with C' (PI again in block 3)
GROUPS = ((0xD314, 0x0408, 0xE0CD, 0x5344), (0xD314, 0x2400, 0x4845, 0x4C4C), (0xD314, 0x0C09, 0xD314, 0x5221))
CPRIME = (False, False, True)


def stream_bits(n_bits: int, groups=GROUPS, cprime=CPRIME) -> np.ndarray:
    bits = []
    k = 0
    while len(bits) < n_bits:
        bits += group_bits(groups[k % len(groups)], cprime[k % len(groups)])
        k += 1
    return np.array(bits[:n_bits], np.uint8)


# ---------------------------------------------------------------- signals
def _symbols(n: int, rate: int, sig: dict) -> np.ndarray:
    """+1 / -1 per sample: the differentially coded bits as biphase symbols"""
    tb = np.arange(n, dtype=np.float64) * (1187.5 / rate)
    idx = np.floor(tb).astype(np.int64)
    bits = stream_bits(int(idx[-1]) + 2 if n else 1)
    diff = np.bitwise_xor.accumulate(bits)
    level = 2.0 * diff[idx] - 1.0
    return np.where(tb - idx < 0.5, level, -level)


def signal(sig: dict, n: int, rate: int, seed: int) -> np.ndarray:
    if sig["kind"] != "mpx" or not sig.get("rds"):
        return bc.signal(sig, n, rate, seed)
    lead = int(sig.get("lead", 0))
    m = n - lead
    t = np.arange(m, dtype=np.float64)
    fp = float(sig.get("fp", 19000.0))
    pil = 2 * np.pi * fp * t / rate
    on = (t >= sig.get("p_on", 0)) & (t < sig.get("p_off", m))
    mod = (sig.get("sum", 20000.0) * np.sin(2 * np.pi * sig.get("fs", 1000.0) * t / rate)
           + sig.get("pilot", 7500.0) * np.sin(pil) * on
           + sig.get("diff", 15000.0) * np.sin(2 * np.pi * sig.get("fd", 700.0) * t / rate) * np.sin(2 * pil)
           + float(sig["rds"]) * _symbols(m, rate, sig) * np.cos(3 * pil + float(sig.get("rds_phi", 0.0))))
    mod = np.concatenate([np.zeros(lead), mod])
    inc = np.round((sig.get("f0", 0.0) + mod) / rate * 4294967296.0).astype(np.int64)
    ph = (np.cumsum(inc) & 0xFFFFFFFF).astype(np.float64) * (2 * np.pi / 4294967296.0)
    amp = np.full(n, float(sig.get("amp", 8000.0)))
    if "runs" in sig:
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
#: the long case: 2 s at 288 kS/s.  Bits and groups come out at RDS samples whose index is a multiple of 8, and a feed's RDS
#: samples end where a 512-sample block ends: at 240, 250 and 384 kS/s no block ends on such an index, at 288 kS/s two of nine do.  Phase, level and lead were searched on the CPU (tests/golden/make_golden_bfm_rds.py
#: --search) until the reference's own chain ran through the 50-block count, NO_SYNC, presync and sync, completed groups, and
#: put a completed group on the last RDS sample of a block; LONG_CUTS are the feed lengths that end on that block and on one
#: whose last RDS sample yields a bit
LONG_N = 576000
LONG_CFG = bc._cfg(288000, rf=200000.0)      # the RF filter has to pass the 57 kHz subcarrier's sidebands
LONG_SIG = dict(kind="mpx", rds=4000.0, rds_phi=1.5707963267948966, lead=3367, sum=8000.0, diff=4000.0, noise=5.0)
# block 190 ends on a bit, block 1090 on a bit that completes a group; the second feed leaves pending samples behind; the third
# ends at block 620, inside the stretch the decoder spends in NO_SYNC (blocks 615 to 635)
LONG_SEED = 777                      # the noise the search ran with
LONG_CUTS = (191 * 512, 100000, 621 * 512 - 191 * 512 - 100000, (1091 - 621) * 512)
FLIP_LEAD = 53


def _tail(n, head):
    assert sum(head) <= n
    return head + [n - sum(head)]


def make_cases() -> list[dict]:
    cases = []

    def add(name, cfg, sig, n, splits, rds=1, seed=None):
        seed = 100 + len(cases) if seed is None else seed
        assert sum(splits) == n, name
        cases.append({"name": name, "cfg": cfg, "sig": sig, "n": n, "seed": seed, "splits": splits, "rds": rds})

    mpx = lambda **kw: dict({"kind": "mpx", "rds": 3000.0}, **kw)
    edges = [0, 1, 511, 512, 513, 2, 700]
    # the three rates (240 kS/s is the clamped schedule: every input yields an RDS sample at phase 0), stereo and mono, the feed
    # lengths at the block's edges (0 and 1: feeds without an RDS sample), feeds that are no multiple of 64 RDS samples
    add("stereo_250k", bc._cfg(250000, nco_freq=-20000, rf=200000.0), mpx(f0=20000.0), 9000, _tail(9000, edges))
    add("lsb_384k", bc._cfg(384000, lsb=1, nco_freq=31000, rf=220000.0), mpx(f0=-31000.0, sum=30000.0), 7000, _tail(7000, [1500, 0, 3]))
    add("stereo_240k", bc._cfg(240000, rf=180000.0), mpx(), 6000, _tail(6000, [2049, 511, 1]))
    add("mono_250k", bc._cfg(250000, stereo=0, nco_freq=12345), mpx(f0=-12345.0), 6000, _tail(6000, [513, 1000]))
    add("mono_240k_one_feed", bc._cfg(240000, stereo=0), mpx(), 4096, [4096])
    add("mono_384k", bc._cfg(384000, stereo=0, rf=200000.0), mpx(), 5000, _tail(5000, [1024, 1]))
    # a squelch that opens and closes mid-stream (the mixer runs on demod = 0: r is +0 or -0 by the cosine's sign)
    add("squelch_bursts", bc._cfg(250000, rf=12500.0, sq=-30.0), mpx(sum=2000.0, pilot=750.0, diff=1000.0, rds=300.0, hi=12000.0, lo=60.0, noise=5.0,
                                                                     runs=[2100, 700, 300, 1700, 200, 900, 1500, 640, 650, 2600]), 12000,
        _tail(12000, [512, 1024, 300, 1300, 1388, 2000, 700]))
    add("pilot_stops", bc._cfg(250000), mpx(p_off=5500), 8000, _tail(8000, [3000, 2000]))
    add("noise", bc._cfg(250000), {"kind": "noise_full"}, 5000, _tail(5000, [2048]))
    add("all_zero", bc._cfg(250000), {"kind": "zero"}, 2048, [1024, 1024])
    # long enough for bits: 30 000 RDS samples, 140 bits, the first report (counter back at 0 needs 800 biphase calls: not yet)
    add("bits_250k", bc._cfg(250000, rf=200000.0), mpx(rds=4000.0, sum=8000.0, diff=4000.0), 30720, _tail(30720, [10000, 5000, 777]))
    # 0.41 s: past the 800th biphase call, where the reference picks the other reading frame (it starts on the wrong one here);
    # the fixture keeps what RDSDemod::process was given for this case (CR_CASE)
    add("flip_250k", bc._cfg(250000, rf=200000.0), mpx(rds=4000.0, sum=8000.0, diff=4000.0, lead=FLIP_LEAD), 102400, _tail(102400, [40000, 45056]))
    if LONG_CUTS is not None:
        add("long_288k", LONG_CFG, LONG_SIG, LONG_N, _tail(LONG_N, list(LONG_CUTS)), seed=LONG_SEED)
    return cases


CASES = make_cases()
CR_CASE = "flip_250k"
AUDIO_CASE = "stereo_250k"          # the one case whose audio and sink stream are recorded: RDS on does not disturb them


def inputs(case: dict) -> np.ndarray:
    return signal(case["sig"], case["n"], case["cfg"]["in_rate"], case["seed"])


# ---------------------------------------------------------------- random configurations, RDS on in every one
RANDOM_SEED = 20261101
RANDOM_GOLDEN = os.path.join(ROOT, "tests", "golden", "bfm_rds_random_golden.npz")    # tests/golden/make_golden_bfm_rds.py --random
#: RDS steps in_rate / 250000 of 0.384, 0.8, 0.96 (below 1 the schedule is clamped: every input emits), 1, 1.152, 1.536 and 2
RANDOM_RATES = (96000, 200000, 240000, 250000, 288000, 384000, 500000)
#: the long cases (every LONG_EVERY-th draw): 0.42 s of their rate, past the 800th biphase call, where the reading frame is chosen
LONG_EVERY, LONG_AT, LONG_RATES = 10, 3, (200000, 240000, 250000, 288000, 384000)
ZERO_AT, NOISE_AT = 7, 19                           # the draws that are a `zero` and a `noise_full` signal
#: draw indices left out because the recording of the reference had a sample whose mixer product rds_mix.hpp's enclosure does not
#: pin (tests/golden/make_golden_bfm_rds.py --random names them); the next index takes the place
RANDOM_SKIP = ()
WIDE_N = 12000                                      # the wide GPU bank cycles over the cases up to this length


def random_case(rng, j: int) -> dict:
    """draw j; every quantity is drawn for every case, used or not, so the order of the rng calls ahead of the splits is fixed"""
    long = j % LONG_EVERY == LONG_AT
    in_rate = int(rng.choice(LONG_RATES if long else RANDOM_RATES))
    audio = int(rng.choice([48000, 44100]))
    rf = bc._f32(min(float(rng.choice([180000.0, 200000.0, 220000.0])), 0.9 * in_rate))
    stereo, lsb = int(rng.random() < 0.7), int(rng.random() < 0.3)
    f0 = float(rng.integers(-in_rate // 16, in_rate // 16))
    sig = {"kind": "mpx", "f0": f0, "rds": float(rng.integers(300, 5001)), "rds_phi": float(rng.uniform(0.0, 2 * np.pi)),
           "lead": int(rng.integers(0, 4001)), "sum": float(rng.integers(1000, 30001)), "diff": float(rng.integers(0, 15001)),
           "fs": float(rng.integers(100, 5000)), "fd": float(rng.integers(100, 5000)), "noise": float(rng.integers(0, 50)),
           "amp": float(rng.choice([3000.0, 8000.0, 20000.0]))}
    n = int(rng.integers(3000, 30001))
    bursts, lo = rng.random() < 0.2, float(rng.integers(1, 200))
    runs = [int(v) for v in rng.integers(300, 4000, size=8)]
    sq, feeds, extra = -60.0, int(rng.integers(2, 5)), rng.random()
    if long:
        n = int((0.42 + 0.02 * extra) * in_rate)
        sig.update(sum=8000.0, diff=4000.0, amp=8000.0, noise=5.0, rds=max(sig["rds"], 2000.0), lead=min(sig["lead"], n // 8))
        splits = sorted(int(v) for v in rng.integers(1, n, size=feeds - 1))
        splits = [b - a for a, b in zip([0] + splits, splits + [n])]
    else:
        sig["lead"] = min(sig["lead"], n // 2)
        if j == ZERO_AT or j == NOISE_AT:
            sig = {"kind": "zero" if j == ZERO_AT else "noise_full"}
        elif bursts:                                            # the mixer runs on demod = 0 while the squelch is closed
            rf, sq = 12500.0, -30.0
            sig.update(hi=12000.0, lo=lo, noise=min(sig["noise"], 5.0), runs=runs, sum=2000.0, diff=1000.0, pilot=750.0, rds=min(sig["rds"], 600.0))
        splits = bc._random_splits(rng, n)
    cfg = bc._cfg(in_rate, audio, nco_freq=-int(f0), rf=rf, sq=sq, stereo=stereo, lsb=lsb)
    return {"name": f"rds_random{j}", "cfg": cfg, "sig": sig, "n": n, "seed": 5000 + j, "splits": splits, "rds": 1, "long": long}


def random_draws(count: int = 40, skip=None):
    """(kept cases, skipped cases): draws in order from one generator, the indices of `skip` (RANDOM_SKIP) set aside, until `count`
    are kept"""
    skip = RANDOM_SKIP if skip is None else skip
    rng = np.random.default_rng(RANDOM_SEED)
    kept, left, j = [], [], 0
    while len(kept) < count:
        (left if j in skip else kept).append(random_case(rng, j))
        j += 1
    return kept, left


def random_cases(count: int = 40) -> list[dict]:
    return random_draws(count)[0]


def rds_step(case: dict) -> float:
    return case["cfg"]["in_rate"] / 250000.0


def _edge(b: np.ndarray, tail: bool) -> np.ndarray:
    out = np.zeros(BB_EDGE, np.float32)
    e = min(BB_EDGE, b.size)
    if e:
        out[:e] = b[-e:] if tail else b[:e]
    return out


def pack_random(cases, results) -> dict:
    """The random draw's fixture from the recorder's results: per case the feeds and the input's sha256; per feed the counts of bits,
    groups and RDS samples, subcarr_bb's sha256 and its first and last BB_EDGE values (the tail's last value last), the report and
    the state words; all bits and all groups on end"""
    feeds = [(c, r, i) for c, r in zip(cases, results) for i in range(len(c["splits"]))]
    sha32 = lambda b: np.frombuffer(bytes.fromhex(sha_f32(b)), np.uint8)
    return {"names": np.array([c["name"] for c in cases]), "feeds": np.array([len(c["splits"]) for c in cases], np.int32),
            "in_sha256": np.array([np.frombuffer(bytes.fromhex(bc.sha(inputs(c))), np.uint8) for c in cases], np.uint8).reshape(-1, 32),
            "bit_counts": np.array([r["bits"][i].size for _, r, i in feeds], np.int64),
            "group_counts": np.array([r["groups"][i].shape[0] for _, r, i in feeds], np.int64),
            "rds_counts": np.array([r["bb"][i].size for _, r, i in feeds], np.int64),
            "bits": np.concatenate([r["bits"][i] for _, r, i in feeds]).astype(np.uint8),
            "groups": np.concatenate([r["groups"][i].reshape(-1, 4) for _, r, i in feeds]).astype(np.uint16).reshape(-1, 4),
            "bb_sha256": np.array([sha32(r["bb"][i]) for _, r, i in feeds], np.uint8).reshape(-1, 32),
            "bb_head": np.array([_edge(r["bb"][i], False) for _, r, i in feeds], np.float32).reshape(-1, BB_EDGE),
            "bb_tail": np.array([_edge(r["bb"][i], True) for _, r, i in feeds], np.float32).reshape(-1, BB_EDGE),
            "report": np.array([r["report"][i] for _, r, i in feeds], np.uint32).reshape(-1, 5),
            "state": np.array([r["state"][i] for _, r, i in feeds], np.uint64).reshape(-1, len(STATE_FIELDS))}


def load_random_golden(path: str = None) -> dict:
    """bfm_rds_random_golden.npz by case name, each entry in golden_case()'s layout (bb is None: digests and edges)"""
    g = np.load(path or RANDOM_GOLDEN)
    out, f0, b0, g0 = {}, 0, 0, 0
    for k, name in enumerate(g["names"].tolist()):
        f1 = f0 + int(g["feeds"][k])
        nb, ng = g["bit_counts"][f0:f1], g["group_counts"][f0:f1]
        b1, g1 = b0 + int(nb.sum()), g0 + int(ng.sum())
        e = [min(BB_EDGE, int(v)) for v in g["rds_counts"][f0:f1]]
        out[name] = {"bits": np.split(g["bits"][b0:b1], np.cumsum(nb)[:-1]), "groups": np.split(g["groups"][g0:g1], np.cumsum(ng)[:-1]),
                     "n_rds": [int(v) for v in g["rds_counts"][f0:f1]], "report": g["report"][f0:f1], "state": g["state"][f0:f1],
                     "in_sha": bytes(g["in_sha256"][k]).hex(), "bb": None, "bb_sha": [bytes(v).hex() for v in g["bb_sha256"][f0:f1]],
                     "bb_head": g["bb_head"][f0:f1],
                     # golden_case()'s tails hold the last e values at their end: [-e:] is read
                     "bb_tail": np.array([np.concatenate([np.zeros(BB_EDGE - e[i], np.float32), t[:e[i]]]) for i, t in enumerate(g["bb_tail"][f0:f1])], np.float32).reshape(-1, BB_EDGE)}
        f0, b0, g0 = f1, b1, g1
    out["host"], out["unsure_skipped"] = str(g["host"]), int(g["unsure_skipped"])
    return out


def random_shares(cases, gold: dict) -> dict:
    """the counts assert_random_shares() puts floors under, from the fixture (load_random_golden())"""
    rf = STATE_FIELDS.index("reading_frame")
    nbits = {c["name"]: sum(b.size for b in gold[c["name"]]["bits"]) for c in cases}
    flipped = {c["name"]: int(gold[c["name"]]["state"][-1][rf]) == 1 for c in cases}
    # biphase emits a bit on every other call and its counter goes round after 800: more than 400 bits, or the other frame
    past = [c for c in cases if c["long"] and (flipped[c["name"]] or nbits[c["name"]] > 400)]
    return {"cases": len(cases), "rates": sorted({c["cfg"]["in_rate"] for c in cases}), "clamped": sum(rds_step(c) < 1 for c in cases),
            "with_bits": sum(v > 0 for v in nbits.values()), "long": sum(c["long"] for c in cases), "long_past_800": len(past),
            "flipped": sum(flipped.values()), "mono": sum(not c["cfg"]["stereo"] for c in cases), "bursts": sum("runs" in c["sig"] for c in cases),
            "kinds": sorted({c["sig"]["kind"] for c in cases}), "samples": sum(c["n"] for c in cases)}


def assert_random_shares(cases, g) -> dict:
    s = random_shares(cases, g)
    assert s["cases"] == 40 and s["rates"] == sorted(RANDOM_RATES) and s["clamped"] >= 10 and s["with_bits"] >= 25, s
    assert s["long"] == 4 and s["long_past_800"] >= 3 and s["mono"] >= 8 and s["kinds"] == ["mpx", "noise_full", "zero"], s
    assert all(3000 <= c["n"] <= 30000 and len(c["splits"]) <= bc.MAX_FEEDS or c["long"] and 2 <= len(c["splits"]) <= 4 for c in cases)
    assert all(c["n"] >= 0.42 * c["cfg"]["in_rate"] for c in cases if c["long"])
    return s


# ---------------------------------------------------------------- frameSync streams
def framesync_streams() -> dict:
    """name -> bits for a fresh RDSDecoder (which starts in SYNC at block 0, bit 0)"""
    rng = np.random.default_rng(20260)
    valid = stream_bits(104 * 9)
    out = {"valid": valid, "cprime": stream_bits(104 * 4, groups=(GROUPS[2],), cprime=(True,))}
    err = stream_bits(104 * 12).copy()
    for at in (30, 104 + 3, 104 * 3 + 60, 104 * 3 + 61, 104 * 5 + 100, 104 * 8 + 20):
        err[at] ^= 1
    out["errors"] = err
    # 50 random blocks (more than 35 wrong: NO_SYNC), then valid groups 7 bits off the old alignment: presync, sync, groups
    lost = np.concatenate([rng.integers(0, 2, 50 * 26 + 7, dtype=np.uint8), stream_bits(104 * 6)])
    out["lose_and_resync"] = lost
    # NO_SYNC, a valid block, noise of a length that puts the next valid block at a wrong distance (presync dropped), then a
    # clean stream
    b0 = np.array(block_bits(0xD314, 0), np.uint8)
    out["presync_dropped"] = np.concatenate([rng.integers(0, 2, 50 * 26, dtype=np.uint8), b0, rng.integers(0, 2, 11, dtype=np.uint8), b0,
                                             rng.integers(0, 2, 40, dtype=np.uint8), stream_bits(104 * 5)])
    # exactly 36 bad blocks of 50: the threshold (35 would stay in sync)
    mixed = []
    for i in range(50):
        blk = block_bits(0x1000 + i, i % 4)
        if i >= 14:
            blk[5] ^= 1
        mixed += blk
    out["bad_36_of_50"] = np.concatenate([np.array(mixed, np.uint8), stream_bits(104 * 6)])
    mixed = []
    for i in range(50):
        blk = block_bits(0x1000 + i, i % 4)
        if i >= 15:
            blk[5] ^= 1
        mixed += blk
    out["bad_35_of_50"] = np.concatenate([np.array(mixed, np.uint8), stream_bits(104 * 6)])
    out["random"] = rng.integers(0, 2, 6000, dtype=np.uint8)
    return out


# ---------------------------------------------------------------- the fixture
def golden():
    return np.load(GOLDEN)


def sha_f32(a: np.ndarray) -> str:
    import hashlib
    return hashlib.sha256(np.ascontiguousarray(a, np.float32).tobytes()).hexdigest()


def golden_case(g, case: dict) -> dict:
    name = case["name"]
    nb, ng, nr = g[f"{name}/bit_counts"], g[f"{name}/group_counts"], g[f"{name}/rds_counts"]
    res = {"bits": np.split(g[f"{name}/bits"], np.cumsum(nb)[:-1]), "groups": np.split(g[f"{name}/groups"].reshape(-1, 4), np.cumsum(ng)[:-1]),
           "n_rds": [int(v) for v in nr], "report": g[f"{name}/report"], "state": g[f"{name}/state"], "in_sha": str(g[f"{name}/in_sha256"]),
           "bb": np.split(g[f"{name}/bb"], np.cumsum(nr)[:-1]) if f"{name}/bb" in g else None}
    if res["bb"] is None:
        res["bb_sha"] = [str(v) for v in g[f"{name}/bb_sha256"]]
        res["bb_head"], res["bb_tail"] = g[f"{name}/bb_head"], g[f"{name}/bb_tail"]
    return res


def state_words(st) -> np.ndarray:
    """a BfmRdsState (sdrangel_amd) as the recorder's words"""
    v = [st.subcarr_phi, st.clock_offset, st.clock_phi, st.prev_clock_phi, st.d_cphi, *st.xv, *st.yv, st.prev_bb, st.acc, st.prev_acc,
         st.lo_clock, st.prev_lo_clock, st.numsamples, st.counter, st.reading_frame, st.tot_errs[0], st.tot_errs[1], st.dbit,
         st.distance_remain, st.mix_phase, st.n_rds, st.reg, st.lastseen_offset_counter, st.bit_counter, st.block_bit_counter,
         st.wrong_blocks_counter, st.blocks_counter, st.group_good_blocks_counter, *st.group, st.sync, st.presync, st.lastseen_offset,
         st.block_number, st.group_assembly_started, st.good_block, st.decoder_qua]
    assert len(v) == len(STATE_FIELDS)
    return np.array([int(x) & 0xFFFFFFFFFFFFFFFF for x in v], np.uint64)


def same_float_bits(got: int, want: int) -> bool:
    """equal bits, or both NaN (m_report.qua is 0.0 / 0 * 100 until an error was counted; the NaN's sign is the host's)"""
    nan = lambda b: (b & 0x7F800000) == 0x7F800000 and (b & 0x007FFFFF) != 0
    return got == want or (nan(got) and nan(want))
