"""GPU: the ChannelAnalyzer bank with the PLL, the FLL and InputPLL (sdrx_chanapll_*), bit for bit, no tolerance anywhere (the
loops feed back): every case of tests/chana_pll_cases.py against the reference's recording (tests/golden/chana_pll_golden.npz:
every Sample of every feed, m_magsq, isPllLocked and the bits of the three floats after every feed), random configurations
against the oracle (tests/chana_pll_oracle.c), one feed against uneven splits, reset, and one handle of mixed channels across
several workgroups of the walk kernel with PLL-off channels and empty feeds through feed_dev."""
import os

import numpy as np
import pytest

import sdrangel_amd as sa
from tests import chana_cases as cc
from tests import chana_pll_cases as pc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BY = {c["name"]: c for c in pc.CASES}


@pytest.fixture(scope="module")
def oracle():
    return pc.build_oracle()


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "chana_pll_golden.npz"))


def make_bank(cfgs) -> sa.ChannelAnalyzerBank:
    return sa.ChannelAnalyzerBank([sa.ChanaCfg(**{k: int(v) for k, v in c.items() if k != "psk_order"}) for c in cfgs],
                                  psk_order=[c["psk_order"] for c in cfgs])


def state_of(bank, c):
    """as the oracle's and the recorder's: (locked, bits of freq, delta phi, phi hat, m_magsq)"""
    k, f, d, p = bank.pll_state(c)
    return (int(k),) + tuple(int(np.float32(v).view(np.uint32)) for v in (f, d, p)) + (bank.magsq(c),)


def run_gpu(cfg, feeds, bank=None):
    bank = bank or make_bank([cfg])
    out, states = [], []
    for x in feeds:
        bank.feed([x])
        out.append(bank.read(0))
        states.append(state_of(bank, 0))
    return bank, out, states


def cat(parts):
    return np.concatenate(parts) if parts else np.zeros((0, 2), np.int16)


def assert_feeds_equal(got, want, what):
    assert [g.shape[0] for g in got] == [w.shape[0] for w in want], what
    for i, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), (what, i, int(np.count_nonzero(g != w)), np.argwhere(g != w)[0].tolist())


@pytest.mark.parametrize("case", pc.CASES, ids=[c["name"] for c in pc.CASES])
def test_case_equals_the_reference_recording(golden, case):
    name = case["name"]
    bank, out, states = run_gpu(case["cfg"], pc.cut(golden[f"{name}/in"], case["splits"]))
    want = golden[f"{name}/out"]
    full = cat(out)
    print(f"{name}: {full.shape[0]} Samples, {int(np.count_nonzero(full != want)) if full.shape == want.shape else 'shape'} differ; state {states[-1]}")
    assert [o.shape[0] for o in out] == golden[f"{name}/counts"].tolist(), name
    assert np.array_equal(full, want), (name, int(np.count_nonzero(full != want)), np.argwhere(full != want)[0].tolist())
    assert [s[4] for s in states] == golden[f"{name}/magsq"].tolist(), name
    assert np.array_equal(np.array([s[1:4] for s in states], np.uint32).reshape(-1, 3), golden[f"{name}/state_bits"]), name
    assert [s[0] for s in states] == golden[f"{name}/locked"].tolist(), name
    assert bank.positive_only(0) == bool(case["cfg"]["ssb"])
    ll = bank.last_launch()
    if case["cfg"]["pll"] and case["cfg"]["input_type"] != pc.AUTOCORR:
        assert ll["kernel"] == "chana_walk_kernel" and ll["block"] == 256 and ll["grid"] == 1 and ll["lds_bytes"] == 0, ll


def test_random_configurations_in_one_handle_equal_the_oracle(oracle):
    """26 channels: seven workgroups of the walk kernel, the last with two waves that have a channel.  Three feeds of uneven
    lengths, channel by channel against the oracle"""
    rng = np.random.default_rng(20261020)
    cfgs = [pc.random_cfg(rng) for _ in range(26)]
    assert len({(c["pll"], c["fll"], c["input_type"]) for c in cfgs}) >= 8
    n = 5000
    xs = [pc.random_signal(rng, n) for _ in cfgs]
    bank = make_bank(cfgs)
    oras = [pc.OraclePll(oracle, c) for c in cfgs]
    total = 0
    for a, b in ((0, 1023), (1023, 1023), (1023, 4097), (4097, 5000)):
        bank.feed([x[2 * a: 2 * b] for x in xs])
        for c in range(len(cfgs)):
            w = oras[c].feed(xs[c][2 * a: 2 * b])
            g = bank.read(c)
            assert g.shape == w.shape and np.array_equal(g, w), (c, cfgs[c], g.shape, w.shape)
            assert state_of(bank, c) == oras[c].state(), (c, cfgs[c])
            total += g.shape[0]
    assert total > 26 * 500
    ll = bank.last_launch()
    assert ll["kernel"] == "chana_corr_kernel" or (ll["kernel"] == "chana_walk_kernel" and ll["grid"] == 7), ll


@pytest.mark.parametrize("name", ["pll_lock_lost_dsb", "psk16_lsb", "pll_down_96k_37k", "fll_pll_in1_lsb", "corr_pll", "pll_span8"])
def test_one_feed_equals_uneven_splits(golden, name):
    case = BY[name]
    x = golden[f"{name}/in"]
    _, one, st_one = run_gpu(case["cfg"], [x])
    rng = np.random.default_rng(len(name))
    splits, left = [], case["n"]
    while left > 0:
        m = min(left, int(rng.choice([0, 1, 63, 64, 65, 1023, 1024, 3000, 4097])))
        splits.append(m); left -= m
    _, parts, st_parts = run_gpu(case["cfg"], pc.cut(x, splits))
    assert np.array_equal(cat(one), cat(parts)) and np.array_equal(cat(one), golden[f"{name}/out"]), name
    assert st_one[-1] == st_parts[-1], name


def test_reset_equals_a_fresh_handle(golden):
    for name in ("pll_lock_lost_dsb", "psk4_noisy", "fll_pll", "corr_pll"):
        case = BY[name]
        feeds = pc.cut(golden[f"{name}/in"], case["splits"])
        bank, first, st_first = run_gpu(case["cfg"], feeds)
        bank.feed([golden["minus_32768/in"][: 2 * 777]])                # leave every loop somewhere else
        bank.reset()
        assert state_of(bank, 0) == (0, 0, 0, 0, 0.0)
        _, again, st_again = run_gpu(case["cfg"], feeds, bank=bank)
        assert_feeds_equal(again, first, name + " after reset")
        assert st_again == st_first, name


def test_mixed_channels_pll_off_and_empty_feeds_through_feed_dev(oracle, golden):
    """11 channels (three workgroups of the walk kernel): loops of every kind between channels without one; in every round some
    channels get an empty feed.  The channels without a loop equal a bank made by sdrx_chana_create on the same inputs"""
    import torch
    names = ["pll_lock_lost_dsb", None, "psk16_lsb", "fll_pll", None, "in1_unfed", "corr_pll", "pll_span8", None, "fll_pll_in1_lsb", "pll_down_96k_37k"]
    plain = [{c["name"]: c for c in cc.CASES}[n] for n in ("usb", "corr_lsb_loud", "span3")]
    cfgs, xs, it = [], [], iter(plain)
    for n in names:
        if n is None:
            c = next(it)
            cfgs.append(dict(c["cfg"], pll=0, fll=0, psk_order=1)); xs.append(cc.inputs(c))
        else:
            cfgs.append(BY[n]["cfg"]); xs.append(golden[f"{n}/in"])
    bank = make_bank(cfgs)
    off = [i for i, n in enumerate(names) if n is None]
    old = sa.ChannelAnalyzerBank([sa.ChanaCfg(pll=0, fll=0, **{k: int(v) for k, v in c["cfg"].items()}) for c in plain])
    oras = [pc.OraclePll(oracle, c) for c in cfgs]
    pos = [0] * len(cfgs)
    keep = torch.zeros(2, dtype=torch.int16, device="cuda")
    for rnd, step in enumerate((700, 1, 3000, 1024, 4097, 2000)):
        parts = []
        for c, x in enumerate(xs):
            m = 0 if (c + rnd) % 4 == 0 else min(step, x.size // 2 - pos[c])
            parts.append(x[2 * pos[c]: 2 * (pos[c] + m)]); pos[c] += m
        ts = [torch.from_numpy(p.copy()).cuda() if p.size else keep for p in parts]
        torch.cuda.synchronize()
        bank.feed_dev([t.data_ptr() for t in ts], [p.size // 2 for p in parts])
        old.feed([parts[c] for c in off])
        for c in range(len(cfgs)):
            w = oras[c].feed(parts[c])
            g = bank.read(c)
            assert g.shape == w.shape and np.array_equal(g, w), (rnd, c, names[c], g.shape, w.shape)
            assert state_of(bank, c) == oras[c].state(), (rnd, c, names[c])
        for i, c in enumerate(off):
            assert np.array_equal(bank.read(c), old.read(i)) and bank.magsq(c) == old.magsq(i), (rnd, c)
        bank.sync()
    ll = bank.last_launch()
    assert ll["kernel"] == "chana_corr_kernel", ll
