"""GPU: the 100 random cases of the ChannelAnalyzer bank with its loops (random_cases() of tests/chana_pll_cases.py: a signal made
for every channel, so that loops lock, saturate and lose lock, and autocorrelation channels complete blocks; the CPU tests of
tests/test_chana_pll_oracle.py assert those shares and tie the oracle to the reference) as mixed banks of 33, 33 and 34 channels,
then all 100 in one handle (25 workgroups of the walk, a second be_ncof_kernel workgroup) and 257 channels, the cases cycled (65
workgroups of the walk, the last with one live wave; a fifth NCOF workgroup with one live lane; blockIdx.y up to 256 in the group,
post, corr, emit and carry kernels).  Every channel follows its own split list, so within a round some channels get an empty feed.

The comparison is the one of tests/test_chana_pll_gpu.py, no tolerance anywhere: after every feed every Sample, m_magsq,
isPllLocked and the bits of the three state floats, against tests/chana_pll_oracle.c, which runs each case once.

Also: two feeds queued through feed_dev with one sync behind them, reset() in mid-stream, and the stream position past 2^31 with
the loops on.  A failure prints the channel and its case dict (cfg, sig, n, seed, splits); REGRESSIONS pins a reduced one."""
import functools

import numpy as np
import pytest

from tests import chana_pll_cases as pc
from tests import test_chana_pll_gpu as pg
from tests.demod_families import naming
from tests.demod_mixed import feed_rounds

pytestmark = pytest.mark.gpu
BANKS = ((0, 33), (33, 66), (66, 100))
WIDE = 257
WALK_WAVES = 4                                              # channels per workgroup of chana_walk_kernel
#: indices into random_cases() of cases that once failed in a bank, run alone in a one-channel handle
REGRESSIONS = []


@functools.lru_cache(maxsize=None)
def expected() -> tuple:
    """(cases, oracle results, inputs cut into feeds), computed once and shared by every test below"""
    cases = pc.random_cases()
    assert len(cases) == 100
    L = pc.build_oracle()
    cuts = [pc.cut(pc.inputs(c), c["splits"]) for c in cases]
    return cases, [pc.run_oracle(L, c["cfg"], x) for c, x in zip(cases, cuts)], cuts


def check_channel(case, ch, where, outs, states, want):
    with naming(case, ch, where):
        pg.assert_feeds_equal(outs, want["out"], f"{where} channel {ch}")
        for r, (g, w) in enumerate(zip(states, want["states"])):
            assert g == w, (f"{where} channel {ch} state (locked, freq, delta phi, phi hat as bits, magsq) after feed {r}", g, w)
        assert len(states) == len(want["states"])


def run_bank(pick, where, bank=None):
    """channel ch runs case pick[ch]: every feed's Samples and the state behind it, then the state once every list has ended"""
    cases, wants, cuts = expected()
    bank = bank or pg.make_bank([cases[i]["cfg"] for i in pick])
    states = [[] for _ in pick]

    def read(bank, ch):
        states[ch].append(pg.state_of(bank, ch))
        return bank.read(ch)

    got = feed_rounds(bank, [cuts[i] for i in pick], read, idle=lambda bank, ch: bank.read(ch).shape[0])
    for ch, i in enumerate(pick):
        check_channel(cases[i], ch, where, got[ch], states[ch], wants[i])
        with naming(cases[i], ch, where):                    # the empty feeds behind a channel's last one left its state alone
            assert pg.state_of(bank, ch) == wants[i]["states"][-1], f"{where} channel {ch} after the last round"
    return bank


@pytest.mark.parametrize("k", range(len(BANKS)))
def test_random_cases_in_one_handle(k):
    lo, hi = BANKS[k]
    run_bank(list(range(lo, hi)), f"cases [{lo}:{hi}]").close()


def test_all_random_cases_in_one_handle():
    """100 channels: 25 workgroups of the walk, a second 64-lane workgroup of the NCOF phase walk"""
    run_bank(list(range(100)), "all cases").close()


def test_wide_bank_of_cycled_random_cases():
    """257 channels, channel c running case c mod 100"""
    cases = expected()[0]
    bank = run_bank([c % len(cases) for c in range(WIDE)], f"{WIDE} channels")
    ll = bank.last_launch()
    # the last kernel the handle notes is fftcorr's transform, (blocks a feed can complete) x channels workgroups
    assert ll["kernel"] == "chana_corr_kernel" and ll["grid"] >= WIDE and ll["grid"] % WIDE == 0 and ll["block"] == 1024, ll
    assert (WIDE + WALK_WAVES - 1) // WALK_WAVES == 65 and WIDE % WALK_WAVES == 1 and WIDE % 64 == 1
    bank.close()


def test_queued_feeds_without_a_sync():
    """cases [0:33] through feed_dev: each round's two consecutive feeds are queued back to back with one sync behind them; the
    second feed's Samples and the state behind both are compared"""
    import torch
    cases, wants, cuts = expected()
    pick = list(range(*BANKS[0]))
    bank = pg.make_bank([cases[i]["cfg"] for i in pick])
    keep = torch.zeros(2, dtype=torch.int16, device="cuda")
    rounds = max(len(cuts[i]) for i in pick)
    compared = 0
    for r in range(0, rounds, 2):
        held = []
        for q in (r, r + 1):
            parts = [cuts[i][q] if q < len(cuts[i]) else np.zeros(0, np.int16) for i in pick]
            held.append((parts, [torch.from_numpy(p.copy()).cuda() if p.size else keep for p in parts]))
        torch.cuda.synchronize()
        for parts, ts in held:
            bank.feed_dev([t.data_ptr() for t in ts], [p.size // 2 for p in parts])
        bank.sync()
        for ch, i in enumerate(pick):
            with naming(cases[i], ch, "queued"):
                g, n_feeds = bank.read(ch), len(cuts[i])
                w = wants[i]["out"][r + 1] if r + 1 < n_feeds else np.zeros((0, 2), np.int16)
                assert g.shape == w.shape and np.array_equal(g, w), (f"round {r}", ch, g.shape, w.shape)
                assert pg.state_of(bank, ch) == wants[i]["states"][min(r + 1, n_feeds - 1)], (f"round {r}", ch)
                compared += g.shape[0]
    assert compared > 33 * 500
    bank.close()


def test_reset_then_the_same_cases_again():
    """reset() in mid-stream -- groups and fftcorr blocks open, loops locked -- then the whole cases: as a fresh handle"""
    cases, wants, cuts = expected()
    lo, hi = BANKS[1]
    pick = list(range(lo, hi))
    bank = pg.make_bank([cases[i]["cfg"] for i in pick])
    head = 3
    for r in range(head):
        bank.feed([cuts[i][r] if r < len(cuts[i]) else np.zeros(0, np.int16) for i in pick])
    at = [min(head, len(cuts[i])) - 1 for i in pick]         # the last feed each channel has had
    for ch, i in enumerate(pick):
        assert pg.state_of(bank, ch) == wants[i]["states"][at[ch]], (ch, cases[i])
    seen = [sum(o.shape[0] for o in wants[i]["out"][: a + 1]) for i, a in zip(pick, at)]
    assert sum(1 for i, a in zip(pick, at) if wants[i]["states"][a][0]) >= 3                                          # locked loops
    assert sum(1 for i, k in zip(pick, seen) if cases[i]["cfg"]["input_type"] == pc.AUTOCORR and k % 4096) >= 3      # open blocks
    assert sum(1 for i, k in zip(pick, seen) if cases[i]["cfg"]["span_log2"] >= 1 and k) >= 3                        # open groups
    bank.reset()
    for ch in range(len(pick)):
        assert pg.state_of(bank, ch) == (0, 0, 0, 0, 0.0), ch
    run_bank(pick, f"cases [{lo}:{hi}] after reset", bank=bank).close()


def test_seek_past_two_to_the_31_with_the_loops_on():
    """sdrx_chana_seek against the oracle's chapo_seek: the groups and fftcorr's call counter follow the position, the loops do not
    depend on it.  A PLL with span_log2 >= 3, an FLL behind the Interpolator, an autocorrelation behind a PLL"""
    cases, _, cuts = expected()
    cfg = lambda c: c["cfg"]
    first = lambda ok: next(i for i, c in enumerate(cases) if ok(cfg(c)))
    pick = [first(lambda k: k["pll"] and not k["fll"] and k["span_log2"] >= 3 and k["input_type"] != pc.AUTOCORR),
            first(lambda k: k["pll"] and k["fll"] and k["down_sample"] and k["input_type"] != pc.AUTOCORR),
            first(lambda k: k["pll"] and not k["fll"] and k["input_type"] == pc.AUTOCORR)]
    positions = [(1 << 31) + 5, (1 << 32) + (1 << 31) + 4 * 4000 + 2, (1 << 33) + 255]
    L = pc.build_oracle()
    bank = pg.make_bank([cases[i]["cfg"] for i in pick])
    oras = [pc.OraclePll(L, cases[i]["cfg"]) for i in pick]
    for ch, pos in enumerate(positions):
        bank.seek(ch, pos)
        oras[ch].seek(pos)
    states = [[] for _ in pick]

    def read(bank, ch):
        states[ch].append(pg.state_of(bank, ch))
        return bank.read(ch)

    got = feed_rounds(bank, [cuts[i] for i in pick], read, idle=lambda bank, ch: bank.read(ch).shape[0])
    for ch, i in enumerate(pick):
        want = {"out": [], "states": []}
        for x in cuts[i]:
            want["out"].append(oras[ch].feed(x)); want["states"].append(oras[ch].state())
        assert sum(o.shape[0] for o in want["out"]) > 500 and any(o.any() for o in want["out"]), cases[i]
        check_channel(cases[i], ch, f"seek to {positions[ch]}", got[ch], states[ch], want)
    bank.close()


def test_regressions_alone():
    for i in REGRESSIONS:
        run_bank([i], f"case {i} alone").close()
