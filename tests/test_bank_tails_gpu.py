"""GPU: the array histories of the lean bank kernel (tree_mx_kernel.hpp) where they can go wrong, bit-exact against the oracle
chains (reference: DownChannelizer::feed, sdrbase/dsp/downchannelizer.cpp:50-91) and against the VALU engine.

The lean kernel has no history walk: the wave that stores the last 16 dwords of an array copies slot -> head and tail -> slot
itself, and one wave does it for the root arms.  A wrong copy shows in the first outputs behind a chunk boundary (4096 input
samples of a pass), so the feeds are a few chunks long:
  * 3, 4 and 5 chunks, each one sample short, exact and one sample over: the warm-up chunk in front of a feed, an interior chunk
    boundary and a ragged last chunk all occur;
  * the longest of them again in two and in three feeds, cut off the chunk grid;
  * one feed of 33 chunks + 1 in two pieces, so that the second pass of a bank (16 input chunks per chunk of its own) crosses its
    own chunk boundaries too.
The input is full-scale noise with a tone, and runs of -32768 around every chunk boundary, so the tail dwords that go through the
slots carry the wrap-negated values of the alternating arms.  The banks (tests/bank_tail_cases.py; tests/test_chan_tails.py holds
them to what they are here for): 2 and 32 channels, and banks of tests/bank_path_cases.py under the default options, with four-
and six-arm children, lower/upper pairs of both, every epilogue class, and roots with plain, alternating and both odd kinds."""
from functools import lru_cache

import numpy as np
import pytest

import sdrangel_amd as sa
from tests import bank_tail_cases as T
from tests import oracle_py as orc
from tests import synth
from tests.test_chan_gpu import assert_engine

pytestmark = pytest.mark.gpu

C = 4096
SINGLE = [k * C + d for k in (3, 4, 5) for d in (-1, 0, 1)]
LONG = 33 * C + 1
# every run: the feed boundaries, from 0 to the total
RUNS = [[0, n] for n in SINGLE] + [[0, 2 * C + 777, 5 * C + 1], [0, C - 5, 3 * C + 2049, 5 * C + 1], [0, 17 * C + 1234, LONG]]


@lru_cache(maxsize=None)
def signal(seed):
    x = synth.mix(LONG, seed, 32767, 3000, 3)
    for k in list(range(1, 7)) + [16, 17, 32, 33]:
        for a, b in ((k * C - 70, k * C - 40), (k * C - 20, min(k * C + 8, LONG))):
            x[2 * a: 2 * b] = -32768
    x.setflags(write=False)
    return x


@lru_cache(maxsize=None)
def reference(name):
    """per run, per channel: the oracle's output, fed the same pieces -- computed once, the same for both engines"""
    in_rate, channels = T.BANKS[name]
    x = signal(300 + sorted(T.BANKS).index(name))
    plans = [orc.chan_plan(in_rate, r, f) for r, f in channels]
    want = []
    for cuts in RUNS:
        per_ch = []
        for modes, _, _ in plans:
            ch = orc.Chain(modes)
            per_ch.append(np.concatenate([ch.feed(x[2 * a: 2 * b]) for a, b in zip(cuts, cuts[1:])]))
        want.append(per_ch)
    return x, plans, want


def run_engine(name, engine, monkeypatch):
    monkeypatch.setenv("SDRX_CHAN_ENGINE", engine)
    monkeypatch.delenv("SDRX_CHAN_MAX_LEVELS", raising=False)
    monkeypatch.delenv("SDRX_CHAN_LDS_KB", raising=False)
    in_rate, channels = T.BANKS[name]
    x, plans, _ = reference(name)
    bank = sa.ChannelizerBank(in_rate, [r for r, _ in channels], [f for _, f in channels])
    for c, (modes, out_rate, ofs) in enumerate(plans):
        m, r, o = bank.info(c)
        assert np.array_equal(m, modes) and (r, o) == (out_rate, ofs), c
    got = []
    for cuts in RUNS:
        bank.reset()
        for a, b in zip(cuts, cuts[1:]):
            bank.feed(x[2 * a: 2 * b])
            assert_engine(bank, engine)
        got.append([bank.read(c).copy() for c in range(len(channels))])
    bank.close()
    return got


@pytest.mark.parametrize("name", list(T.BANKS))
def test_histories_bit_exact(name, monkeypatch):
    _, plans, want = reference(name)
    got = {e: run_engine(name, e, monkeypatch) for e in ("mfma", "valu")}
    bad = []
    for k, cuts in enumerate(RUNS):
        for c in range(len(plans)):
            w, m, v = want[k][c], got["mfma"][k][c], got["valu"][k][c]
            if m.size != w.size or not np.array_equal(m, w):
                bad.append(("mfma vs oracle", cuts, c, len(plans[c][0]), m.size, w.size))
            if v.size != w.size or not np.array_equal(v, w):
                bad.append(("valu vs oracle", cuts, c, len(plans[c][0]), v.size, w.size))
            if m.size != v.size or not np.array_equal(m, v):
                bad.append(("mfma vs valu", cuts, c, len(plans[c][0]), m.size, v.size))
    assert not bad, (name, bad[:6])
    # the feeds are long enough to say something: the shallowest channel has outputs behind every chunk boundary
    assert max(w.size for w in want[0]) // 2 >= (SINGLE[0] >> min(len(p[0]) for p in plans)) - 1
