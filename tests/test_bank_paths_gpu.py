"""GPU: every bank of tests/bank_path_cases.py -- together they take every branch of tree_kernel.hpp the planner can plan -- under
both engines, bit-exact against the oracle chains (reference: DownChannelizer::feed, sdrbase/dsp/downchannelizer.cpp:50-91).

Input: full-scale noise with a tone and runs of -32768 (the int16 wrap of the odd arms' negation, on both polyphase arms).
Feeds: an empty one, two under one 4096-sample chunk, one of several chunks, and boundaries that sit inside a group of four
outputs at every depth of the bank (so every level's first and last jobs of a feed take the partial-store path)."""
from concurrent.futures import ThreadPoolExecutor
from functools import lru_cache

import numpy as np
import pytest

import sdrangel_amd as sa
from tests import bank_path_cases as B
from tests import oracle_py as orc
from tests import synth
from tests.test_chan_gpu import assert_engine

pytestmark = pytest.mark.gpu
POOL = ThreadPoolExecutor(max_workers=16)


def ragged(p, depth):
    """the first position >= p whose output index at every depth <= `depth` is 0 or not a multiple of 4"""
    while True:
        d = next((d for d in range(depth + 1) if (p >> d) and (p >> d) % 4 == 0), None)
        if d is None:
            return p
        p = ((p >> d) + 1) << d                             # every position below this one has the same index at depth d


@lru_cache(maxsize=1)
def reference(name):
    """input, feed boundaries, per channel (modes, oracle output of every feed) -- the same for both engines"""
    case = next(c for c in B.CASES if c["name"] == name)
    plans = [orc.chan_plan(case["in_rate"], r, f) for r, f in case["channels"]]
    depth = max(len(p[0]) for p in plans)
    n = ragged(max(1 << 20, 40 << depth), depth)            # >= 40 outputs for the deepest channel
    x = synth.mix(n, 90 + B.CASES.index(case), 32767, 3000, 3)
    for a, k in ((1000, 1), (5001, 2), (77_777, 3), (n // 2, 64), (n - 5000, 700)):
        x[2 * a: 2 * (a + k)] = -32768
    b1 = ragged(4095 + 6 * 4096 + 1234, depth)              # several chunks
    b2 = ragged(b1 + 1 + 2500, depth)
    b3 = ragged(n // 2 + 12345, depth)
    bounds = [0, 0, 3, 4095, b1, b1 + 1, b2, b3, b3, n]     # cuts: 0, 3, 4092, several chunks, 1, ~2500, many, 0, the rest
    assert all(a <= b for a, b in zip(bounds, bounds[1:])) and b3 < n

    def run(modes):
        ch = orc.Chain(modes)
        return modes, [ch.feed(x[2 * a: 2 * b]) for a, b in zip(bounds, bounds[1:])]

    return x, bounds, list(POOL.map(run, [p[0] for p in plans])), plans


@pytest.mark.parametrize("engine", B.ENGINES)
@pytest.mark.parametrize("name", [c["name"] for c in B.CASES])
def test_bank_paths_bit_exact(name, engine, monkeypatch):
    case = next(c for c in B.CASES if c["name"] == name)
    monkeypatch.setenv("SDRX_CHAN_ENGINE", engine)
    if B.OPTIONS[case["options"]]:
        levels, kb = B.OPTIONS[case["options"]]
        monkeypatch.setenv("SDRX_CHAN_MAX_LEVELS", str(levels))
        monkeypatch.setenv("SDRX_CHAN_LDS_KB", str(kb))
    else:
        monkeypatch.delenv("SDRX_CHAN_MAX_LEVELS", raising=False)
        monkeypatch.delenv("SDRX_CHAN_LDS_KB", raising=False)
    x, bounds, ref, plans = reference(name)
    bank = sa.ChannelizerBank(case["in_rate"], [r for r, _ in case["channels"]], [f for _, f in case["channels"]])
    for c, (modes, out_rate, ofs) in enumerate(plans):
        m, r, o = bank.info(c)
        assert np.array_equal(m, modes) and (r, o) == (out_rate, ofs), c
    have = [0] * len(ref)
    for k, (a, b) in enumerate(zip(bounds, bounds[1:])):
        bank.feed(x[2 * a: 2 * b])
        if b > 0:
            assert_engine(bank, engine)
        for c, (_, segs) in enumerate(ref):
            have[c] += segs[k].size // 2
            assert bank.available(c) == have[c], (name, engine, k, c)
    bad = []
    for c, (modes, segs) in enumerate(ref):
        want = np.concatenate(segs)
        got = bank.read(c)
        if got.size != want.size or not np.array_equal(got, want):
            bad.append((c, len(modes), int((got[: want.size] != want[: got.size]).sum())))
    bank.close()
    assert not bad, (name, engine, bad)
