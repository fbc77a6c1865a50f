"""Streams that take the channel banks past 2^30, 2^31, 2^32 and 2^33 input samples without an oracle that has to follow them.

The raw stream is P | B | B | B | ...: a short prefix P and one block B of N samples repeated for ever.  N is a multiple of
2^(D+2) for the deepest chain D of the bank, so every stage has the same decimation phase and the same rotation phase (index mod 4
at every depth) at the start of every repetition, and N >= 46 * 2^D, so the memory of the deepest chain (order-48 stages: fewer than
46 * 2^D raw samples) lies inside one repetition.  From repetition 2 on, a chain's output is therefore the same in every repetition:
W2 == W3, feed by feed, when every repetition is cut at the same places.  tests/test_long_stream.py proves that with the oracle
alone; tests/test_long_stream_gpu.py compares the banks with W2 at stream positions where only the position has changed.

Repetition k (k = 0, 1, ...) starts at the absolute position len(P) + k * N.  The cut N - len(P) inside a repetition therefore
falls on a multiple of N: on 2^30, 2^31, 2^32 and 2^33 exactly, in the repetition that holds them."""
from functools import lru_cache

import numpy as np

from tests import bank_path_cases as B
from tests import oracle_py as orc
from tests import synth
from tests.test_bank_paths_gpu import POOL, ragged
from tests.test_chan_gpu import FS, cfg3_channels
from tests.test_wide24_gpu import _band_of

R = 16                                                      # repetitions of B in the travel buffer Brep
P_LEN = 5003                                                # odd, prime: a multiple of nothing
N16 = 1 << 20                                               # D <= 12: a multiple of 2^14, >= 46 * 2^12
N24 = 1 << 19                                               # D <= 13: a multiple of 2^15, >= 46 * 2^13
THRESHOLDS16 = (1 << 30, 1 << 31, 1 << 32, 1 << 33)
THRESHOLDS24 = (1 << 30, 1 << 31, 1 << 32)

BANKS16 = {"cfg3": dict(in_rate=FS, channels=list(zip(*cfg3_channels())), options="default")}
BANKS16.update({c["name"]: c for c in B.CASES if c["name"] in ("warm2_raw", "cover1")})

STAGES24 = (0, 1, 6, 7, 12, 13)                             # the bank of test_wide24_gpu.test_bank24_mixed_depths
IN_RATE24 = 1 << 22
DECIM24 = ((6, 1, 16), (3, 0, 12))                          # (log2, fcpos, input bits): decimate64_sup, decimate8_inf


def n_ok(n, depth, order=48):
    """the two conditions on the block length for a chain of `depth` stages"""
    return n % (1 << (depth + 2)) == 0 and n >= (order - 2) * (1 << depth)


def ragged_cuts(n, p_len, depth):
    """feed boundaries inside one repetition: feeds of 0, 3, under one chunk, several chunks, 1, ~2500, many, 0 samples, then up to
    the multiple of N, then the rest.  The ragged ones sit inside a group of four outputs at every depth (taken on the absolute
    position: repetitions start at p_len mod 2^(depth + 2)); the multiple of N is the opposite, aligned at every depth."""
    def rg(q):
        return ragged(p_len + q, depth) - p_len
    b1 = rg(4095 + 6 * 4096 + 1234)
    b2 = rg(b1 + 1 + 2500)
    b3 = rg(n // 2 + 12345)
    cuts = [0, 0, 3, 4095, b1, b1 + 1, b2, b3, b3, n - p_len, n]
    assert all(a <= b for a, b in zip(cuts, cuts[1:])) and b3 < n - p_len
    return cuts


def group_cuts(n, p_len, g):
    """the same kinds of feed for a decimator that takes whole groups of g samples"""
    def dn(q):
        return q // g * g
    b3 = dn(n // 2 + 12345)
    cuts = [0, 0, g, dn(4095), dn(29905), dn(29905) + g, dn(29905) + g + dn(2500), b3, b3, n - p_len, n]
    assert all(a <= b for a, b in zip(cuts, cuts[1:])) and b3 < n - p_len and all(c % g == 0 for c in cuts) and p_len % g == 0
    return cuts


def periodic_outputs(feed, p, b, cuts):
    """[W0, W1, W2, W3] of one chain: W0 = [its output for P], Wk = its output for every feed of repetition k"""
    out = [[feed(p)]]
    for _ in range(3):
        out.append([feed(b[2 * a: 2 * e]) for a, e in zip(cuts, cuts[1:])])
    return out


def block16(n, seed):
    """as the input of test_bank_paths_gpu.reference(): full-scale noise, a tone, runs of -32768"""
    b = synth.mix(n, seed, 32767, 3000, 3)
    for a, k in ((1000, 1), (5001, 2), (77_777, 3), (n // 2, 64), (n - 5000, 700)):
        b[2 * a: 2 * (a + k)] = -32768
    return b


@lru_cache(maxsize=1)
def bank16(name):
    """one 16-bit bank: prefix, block, cuts, per channel its plan and [W0, W1, W2, W3] -- the same for both engines"""
    case = BANKS16[name]
    plans = [orc.chan_plan(case["in_rate"], r, f) for r, f in case["channels"]]
    depth = max(len(p[0]) for p in plans)
    seed = 700 + list(BANKS16).index(name)
    p, b = synth.mix(P_LEN, seed + 50, 32767, 0), block16(N16, seed)
    cuts = ragged_cuts(N16, P_LEN, depth)
    W = list(POOL.map(lambda pl: periodic_outputs(orc.Chain(pl[0]).feed, p, b, cuts), plans))
    return dict(name=name, case=case, plans=plans, depth=depth, depths=[len(pl[0]) for pl in plans], n=N16, p=p, b=b, cuts=cuts, W=W)


@lru_cache(maxsize=1)
def bank24():
    """the 24-bit bank: pass-through, 1, 6, 7, 12 and 13 stages on {int32, int32} samples"""
    rng = np.random.default_rng(5)
    channels = [_band_of(IN_RATE24, rng.integers(0, 3, size=k)) for k in STAGES24]
    plans = [orc.chan_plan(IN_RATE24, r, f) for r, f in channels]
    depth = max(len(p[0]) for p in plans)
    p, b = synth.noise24(P_LEN, 811), synth.noise24(N24, 812)
    b[::13] = -(1 << 23)
    cuts = ragged_cuts(N24, P_LEN, depth)

    def run(pl):
        feed = orc.Chain24(pl[0]).feed if len(pl[0]) else np.copy       # no stage: the input goes straight through
        return periodic_outputs(feed, p, b, cuts)

    W = list(POOL.map(run, plans))
    return dict(name="bank24", channels=channels, plans=plans, depth=depth, depths=[len(pl[0]) for pl in plans], n=N24, p=p, b=b,
                cuts=cuts, W=W)


@lru_cache(maxsize=2)
def decim24(log2, fcpos, bits):
    """one 24-bit decimator on int16 input; every feed is whole groups, the prefix an odd number of them"""
    g = orc.lib().sdro_decim_group_int16(log2, fcpos) // 2
    p_len = 77 * g
    p, b = synth.mix(p_len, 821 + log2, 32767, 0), block16(N24, 822 + log2)
    cuts = group_cuts(N24, p_len, g)
    W = [periodic_outputs(orc.Decim24(log2, fcpos, bits).process, p, b, cuts)]
    return dict(name=f"decim24_{log2}_{fcpos}_{bits}", group=g, depth=log2, depths=[log2], n=N24, p=p, b=b, cuts=cuts, W=W)
