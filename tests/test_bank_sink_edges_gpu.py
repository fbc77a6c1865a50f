"""GPU: the lean bank kernel's sink stores and root fill at their edges, under both engines, bit for bit against the oracle chains
(reference: DownChannelizer::feed, sdrbase/dsp/downchannelizer.cpp:50-91).

tree_mx_kernel decides per job, on the scalar side, whether the job's 256 outputs lie wholly inside the range [lo, hi) a feed may
store: such a job stores 16 bytes per lane with no compare, a job on the edge of a feed takes the per-lane path.  The root arms are
filled by one of three bodies, for roots with plain odd arms (E+O), alternating ones (E+A), or both (E+O+A); a root with even arms
only does not exist: a root is an inner node, and the planner gives it the odd arms its children read.  The banks here are small
(3 channels, tests/bank_sink_edge_cases.py) and the feeds short (at most 6 chunks of the pass they are aimed at), chosen so that

* `lo` and `hi` fall inside a lane's four outputs and inside a job at every pass depth: feeds of 1, 3, 4093, 4096, 4099, 8191 and
  12289 samples, carried across consecutive feeds of one bank (schedule "ragged");
* one feed has chunks that are neither its first nor its last (the compare-free path), and a feed of one sample follows it (the
  per-lane path, in the same bank): schedule "long" for pass 0 (5 chunks of 4096 samples: the channel that ends at depth 2 and the
  node streams to pass 1), schedule "deep" for pass 1 (5 chunks of 65536 input samples: the node streams to pass 2).  Pass 2 would
  need feeds of 3 M samples to have an interior chunk; there its jobs take the per-lane path here, and the compare-free path of
  pass 2 rests on the long feeds of tests/test_bank_paths_gpu.py and tests/test_fullsize_gpu.py;
* two channels share one stage chain, so that one node's sink list has two entries (bank "twins");
* a channel ends inside pass 0 on a node that a deep channel goes on from, and beside the sibling a deep channel goes through: a
  sink with a shift next to arm stores in one job (banks "shallow_A", "all_kinds", "centre_O");
* the first pass's root has alternating odd arms only ("shallow_A"), plain ones only ("centre_O"), and both ("all_kinds", "twins").
  Which kinds a root has follows from the first stage of its channels: a centre stage reads the plain odd arm, a lower or upper
  one the alternating copy (chan_plan.cpp: alloc_arms).

That the lean kernel and not the general one runs these banks cannot be seen from last_launch() (both are "tree_kernel<mfma>");
tests/test_chan_lower_root.py checks on the host that the lowering takes every pass of each bank and which root kinds it records."""
from functools import lru_cache

import numpy as np
import pytest

import sdrangel_amd as sa
from tests import bank_path_cases as B
from tests import oracle_py as orc
from tests import synth
from tests.bank_sink_edge_cases import BANKS, IN_RATE

pytestmark = pytest.mark.gpu

SCHEDULES = {
    "ragged": [1, 3, 4093, 4096, 4099, 8191, 12289],
    "long": [5 * 4096 + 17, 1, 2 * 4096 + 5],
    "deep": [5 * 65536 + 17, 1],
}


@lru_cache(maxsize=None)
def reference(bank, schedule):
    """input, feed boundaries, per channel (modes, rate, offset, oracle output of every feed) -- the same for both engines"""
    channels, _ = BANKS[bank]
    bounds = np.concatenate([[0], np.cumsum(SCHEDULES[schedule])])
    n = int(bounds[-1])
    x = synth.mix(n, 700 + sorted(BANKS).index(bank), 32767, 3000, 3)
    for a, k in ((2, 1), (4090, 7), (n // 2, 64), (n - 300, 200)):        # runs of -32768: the int16 wrap of the odd arms' negation
        x[2 * a: 2 * (a + k)] = -32768
    ref = []
    for r, f in channels:
        modes, out_rate, ofs = orc.chan_plan(IN_RATE, r, f)
        ch = orc.Chain(modes)
        ref.append((modes, out_rate, ofs, [ch.feed(x[2 * a: 2 * b]) for a, b in zip(bounds, bounds[1:])]))
    return x, bounds, ref


def test_banks_are_what_they_are_for():
    """the chains behind the banks' names (no GPU work: the oracle's plan)"""
    for name, (channels, _) in BANKS.items():
        plans = [[int(m) for m in orc.chan_plan(IN_RATE, r, f)[0]] for r, f in channels]
        assert 2 <= len(plans) <= 4
        assert max(len(p) for p in plans) >= 9, name                       # three passes: sinks at every pass depth
    t = [[int(m) for m in orc.chan_plan(IN_RATE, r, f)[0]] for r, f in BANKS["twins"][0]]
    assert t[0] == t[2] != t[1]
    for name in ("all_kinds", "shallow_A", "centre_O"):
        plans = [[int(m) for m in orc.chan_plan(IN_RATE, r, f)[0]] for r, f in BANKS[name][0]]
        short = min(plans, key=len)
        assert len(short) < 4, name                                         # ends inside pass 0 (4 levels)
        # a deeper channel goes on from the node the short one ends on, or through that node's sibling
        assert any(len(p) > len(short) and p[: len(short) - 1] == short[:-1] for p in plans), name


@pytest.mark.parametrize("engine", B.ENGINES)
@pytest.mark.parametrize("schedule", sorted(SCHEDULES))
@pytest.mark.parametrize("bank_name", sorted(BANKS))
def test_sink_edges_bit_exact(bank_name, schedule, engine, monkeypatch):
    monkeypatch.setenv("SDRX_CHAN_ENGINE", engine)
    monkeypatch.delenv("SDRX_CHAN_MAX_LEVELS", raising=False)
    monkeypatch.delenv("SDRX_CHAN_LDS_KB", raising=False)
    channels, _ = BANKS[bank_name]
    x, bounds, ref = reference(bank_name, schedule)
    bank = sa.ChannelizerBank(IN_RATE, [r for r, _ in channels], [f for _, f in channels])
    for c, (modes, out_rate, ofs, _) in enumerate(ref):
        m, r, o = bank.info(c)
        assert np.array_equal(m, modes) and (r, o) == (out_rate, ofs), c
    have = [0] * len(ref)
    for k, (a, b) in enumerate(zip(bounds, bounds[1:])):
        bank.feed(x[2 * a: 2 * b])
        assert bank.last_launch()["kernel"] == f"tree_kernel<{engine}>"     # the engine asked for is the one that ran
        for c, (_, _, _, segs) in enumerate(ref):
            have[c] += segs[k].size // 2
            assert bank.available(c) == have[c], (bank_name, schedule, engine, k, c)
    bad = []
    for c, (modes, _, _, segs) in enumerate(ref):
        want = np.concatenate(segs)
        got = bank.read(c)
        if got.size != want.size or not np.array_equal(got, want):
            bad.append((c, len(modes), int((got[: want.size] != want[: got.size]).sum())))
    bank.close()
    assert not bad, (bank_name, schedule, engine, bad)
