"""GPU: the per-channel work arena of the WFM bank and of the channel back-end while it grows.  A channel's arena starts at
4096 samples and doubles; the front of `tail` (fftfilt's overlap) and of `dem` / `res` (the resampler window / the pending
resampler outputs) carry state from feed to feed and have to arrive in the new arena.  Every feed bit for bit against the
CPU oracles of the neighbouring tests (wc.run_oracle, orc.Backend)."""
import numpy as np
import pytest

import sdrangel_amd as sa
from tests import synth
from tests import wfm_cases as wc
from tests.test_backend_gpu import CFGS, mk, ulp_diff
from tests.test_wfm_gpu import assert_feeds_equal, check_levels, gcfg, run_gpu

pytestmark = pytest.mark.gpu

#: 4096 -> 8192 at the second feed, -> 16384 at the fourth, -> 32768 at the sixth; each time the raw remainder (the running
#: total mod 512: 440, 29, 31) and the back-end's pending resampler outputs are not empty, and an overlap buffer is live
GROWING = [3000, 4097, 100, 8193, 513, 20000]
#: per-feed lengths of three channels of one handle: capacities 4096, 8192 and 32768 next to each other in the pointer table
MIXED = [100, 5000, 20000]


@pytest.fixture(scope="module")
def oracle():
    return wc.build_oracle()


def wfm_case(splits, seed=None):
    case = dict({c["name"]: c for c in wc.CASES}["default_120k"])
    case.update(n=sum(splits), splits=list(splits))
    if seed is not None:
        case["seed"] = seed
    return case


@pytest.fixture(scope="module")
def growing(oracle):
    case = wfm_case(GROWING)
    return case, wc.run_oracle(oracle, case)


def test_wfm_growth_carries_the_overlap_and_the_resampler_window(growing):
    case, want = growing
    bank, got = run_gpu(case)
    assert_feeds_equal(got, want["feeds"], "growing")
    check_levels(bank, 0, want, "growing")


def test_wfm_reset_after_growth_clears_what_the_grown_arena_carries(growing):
    case, want = growing
    bank, first = run_gpu(case)
    bank.reset()
    _, second = run_gpu(case, bank=bank)
    assert_feeds_equal(second, first, "second pass vs first")
    assert_feeds_equal(second, want["feeds"], "second pass")
    check_levels(bank, 0, want, "second pass")


def test_wfm_channels_of_different_capacities_in_one_handle(oracle):
    cases = [wfm_case([m] * 3, seed=200 + k) for k, m in enumerate(MIXED)]
    want = [wc.run_oracle(oracle, c) for c in cases]
    cuts = [wc.cut(wc.inputs(c), c["splits"]) for c in cases]
    bank = sa.WfmDemodBank([gcfg(c["cfg"]) for c in cases])
    got = [[] for _ in cases]
    for r in range(3):
        bank.feed([x[r] for x in cuts])
        for c in range(len(cases)):
            got[c].append(bank.read(c))
    for c in range(len(cases)):
        assert_feeds_equal(got[c], want[c]["feeds"], f"channel {c}")
        check_levels(bank, c, want[c], f"channel {c}")


@pytest.mark.parametrize("k", [1, 7, 10], ids=["ssb_1024", "dsb_2048", "no_filter_nondyadic"])
def test_backend_growth_carries_the_pending_outputs_and_the_overlap(k):
    g, o = mk(CFGS[k])
    bank = sa.BackendBank([g])
    x = synth.mix(sum(GROWING), 900 + k, 12000, 6000, 1 + k % 3)
    pos = 0
    for i, m in enumerate(GROWING):
        seg = x[2 * pos: 2 * (pos + m)]
        pos += m
        bank.feed([seg])
        want, got = o.feed(seg), bank.read(0)
        assert got.size == want.size, (i, got.size, want.size)
        assert ulp_diff(got, want) == 0, i


def test_backend_channels_of_different_capacities_in_one_handle():
    pairs = [mk(CFGS[k]) for k in (1, 7, 10)]
    bank = sa.BackendBank([p[0] for p in pairs])
    xs = [synth.mix(3 * m, 950 + c, 12000, 6000, 1 + c) for c, m in enumerate(MIXED)]
    for r in range(3):
        segs = [x[2 * r * m: 2 * (r + 1) * m] for x, m in zip(xs, MIXED)]
        bank.feed(segs)
        for c, (_, o) in enumerate(pairs):
            want, got = o.feed(segs[c]), bank.read(c)
            assert got.size == want.size, (c, r, got.size, want.size)
            assert ulp_diff(got, want) == 0, (c, r)
