"""GPU: the AM demodulator bank's synchronous-AM chain (sdrx_am_create_ex) on the 100 configurations of
am_sync_cases.random_cases() against tests/am_oracle.c, which tests/test_am_sync_oracle.py ties to the reference on these very
cases (to the rebuilt recorder in full where the reference is present, to its digests in
tests/golden/am_sync_random_golden.npz anywhere).  The rules are those of tests/test_am_sync_gpu.py (assert_feeds_equal,
check_state), fed from the oracle's result: after every feed the audio, m_magsq, the peak, the count, the squelch state,
getPllLocked() and the bits of getPllFrequency() bit for bit, the level sum within the reorder bound; once per sync channel
sync_design() equal to the oracle's; for an envelope channel pll() is (False, 0.0) and the envelope design equals the oracle's.

The draw: audio at 1000 S/s (the AGC history rate / 4 shorter than both block lengths), 4000 to 8000, 32000, 44100 and 48000 S/s
(the history longer than most feeds), resampler steps from 1 to 16 with non-dyadic ones, the three operations and envelope
channels, every squelch level, four SSBFilter designs; see DESIGN.md 4.10.  As banks of 33, 33 and 34 channels in one handle each
(nine workgroups of am_sync_walk_kernel, the last with one live wave in the banks of 33; three groups of am_sync_psum_kernel), all
100 in one handle (25 workgroups of the walk, a second workgroup of the 64-lane kernels, seven psum groups), and 257 channels
with the shorter cases cycled (65 workgroups of the walk, the last with one live wave; 17 psum groups; blockIdx.y up to 256).
Every channel is cut by its own list; in the wide bank one channel gets nothing in the first call.  Three sync channels as a
chain of ten queued feed_dev spans, and the 1000 S/s cases fed sample by sample across their first block boundary.

A failure prints the channel and its case dict (cfg, sync, sig, n, seed, splits); REGRESSIONS pins a reduced one."""
import functools

import numpy as np
import pytest

import sdrangel_amd as sa
from tests import am_sync_cases as sc
from tests.demod_families import naming
from tests.demod_mixed import feed_rounds
from tests.test_am_sync_gpu import assert_feeds_equal, check_state, gcfg, gsync
from tests.test_demod_queued_gpu import BIG, HEAD

pytestmark = pytest.mark.gpu
BANKS = ((0, 33), (33, 66), (66, 100))
WIDE = 257
#: indices into random_cases() of cases that once failed in a bank, run alone in a one-channel handle
REGRESSIONS = []
#: the queued chain: DSB at 48000, USB at 1000 and LSB at 44100 from 96000, of the forced head
CHAIN = (6, 1, 11)


@functools.lru_cache(maxsize=None)
def expected() -> tuple:
    """(the random cases, their oracle results, the oracle), computed once and left unchanged; the draw's shares are asserted on the
    oracle's probes before anything runs on the device"""
    cases = sc.random_cases()
    L = sc.build_oracle()
    runs = [sc.run_oracle(L, c) for c in cases]
    sc.assert_random_shares(cases, runs)
    return cases, runs, L


@functools.lru_cache(maxsize=None)
def cuts_of(index: int, lead_empty: bool = False):
    """a case's input cut by its own list, synthesised once"""
    case = expected()[0][index]
    return sc.cut(sc.inputs(case), ([0] if lead_empty else []) + case["splits"])


def as_gold(case, run) -> dict:
    """an oracle result under the keys check_state reads from the recording"""
    return {case["name"] + "/levels": run["levels"], case["name"] + "/state": run["state"]}


def make_bank(cases):
    return sa.AmDemodBank([gcfg(c["cfg"]) for c in cases], sync=[gsync(c["sync"]) for c in cases])


def assert_design(bank, ch, case, L):
    if case["sync"][0]:
        want = sc.OracleAmSync(L, case["cfg"], case["sync"]).sync_design()
        got = bank.sync_design(ch)
        assert got[1].size == 2 * 2 * sc.block(case["sync"][1])
        for g, w, key in zip(got, want, ("taps", "filter", "coef")):
            assert g.size == w.size and np.array_equal(g.view(np.uint32), w.view(np.uint32)), ("sync design", key)
    else:
        assert bank.pll(ch) == (False, 0.0)
        nt, taps, bp, inc, lvl = sc.OracleAmSync(L, case["cfg"], case["sync"]).design()
        g = bank.design(ch)
        assert g[0] == nt and g[3] == inc and np.float32(g[4]) == np.float32(lvl)
        assert np.array_equal(g[1].view(np.uint32), taps.view(np.uint32)) and np.array_equal(g[2].view(np.uint32), bp.view(np.uint32))


def run_bank(pick, where, empty_first=()):
    """channel c runs case pick[c] cut by its own list; the channels of `empty_first` get an empty feed before it.  The state is
    compared after every feed, the audio of every feed at the end"""
    cases, runs, L = expected()
    chans = [cases[i] for i in pick]
    bank = make_bank(chans)
    for ch, case in enumerate(chans):
        with naming(case, ch, where):
            assert_design(bank, ch, case, L)
    golds = [as_gold(cases[i], runs[i]) for i in pick]
    seen = [0] * len(pick)

    def read(bank, ch):
        case, r = chans[ch], seen[ch] - (1 if ch in empty_first else 0)
        seen[ch] += 1
        audio = bank.read(ch)
        with naming(case, ch, where):
            if r < 0:                                       # the leading empty feed: nothing out, nothing moved
                assert audio.size == 0 and bank.levels(ch) == (0.0, 0.0, 0.0, 0) and not bank.squelch_open(ch) and bank.pll(ch) == (False, 0.0)
            else:
                check_state(bank, ch, golds[ch], case, r, f"{where} channel {ch} {case['name']} feed {r}")
                if not case["sync"][0]:
                    assert bank.pll(ch) == (False, 0.0)
        return audio

    got = feed_rounds(bank, [cuts_of(i, ch in empty_first) for ch, i in enumerate(pick)], read, idle=lambda bank, ch: bank.read(ch).shape[0])
    for ch, i in enumerate(pick):
        with naming(chans[ch], ch, where):
            feeds = got[ch][1:] if ch in empty_first else got[ch]
            assert_feeds_equal(feeds, runs[i]["feeds"], f"{where} channel {ch} {chans[ch]['name']}")
            check_state(bank, ch, golds[ch], chans[ch], -1, f"{where} channel {ch} {chans[ch]['name']} at the end")
    return bank


def kinds_of(pick) -> set:
    cases = expected()[0]
    return {(cases[i]["sync"][1] + 1) if cases[i]["sync"][0] else 0 for i in pick}


@pytest.mark.parametrize("k", range(len(BANKS)))
def test_random_cases_in_one_handle(k):
    lo, hi = BANKS[k]
    assert kinds_of(range(lo, hi)) == {0, 1, 2, 3}, "envelope channels and the three operations in one handle"
    run_bank(list(range(lo, hi)), f"am sync cases [{lo}:{hi}]")


def test_all_random_cases_in_one_handle():
    """100 channels: 25 workgroups of the walk, a second workgroup of the 64-lane per-channel kernels, seven psum groups"""
    run_bank(list(range(100)), "am sync all cases")


def test_wide_bank_of_cycled_random_cases():
    """257 channels over the cases of at most WIDE_N samples, cycled: 65 workgroups of the walk, the last with one live wave, 17 psum
    groups, blockIdx.y up to 256; channel 1 is fed nothing in the first call and runs one call behind its neighbours"""
    cases = expected()[0]
    short = [i for i, c in enumerate(cases) if c["n"] <= sc.WIDE_N]
    assert len(short) >= 40 and kinds_of(short) == {0, 1, 2, 3}
    pick = [short[c % len(short)] for c in range(WIDE)]
    # the lone live wave of the last workgroup and the late channel are sync channels
    pick[WIDE - 1], pick[1] = (next(i for i in short if cases[i]["sync"][0] and cases[i]["sync"][1] == op) for op in (sc.USB, sc.DSB))
    run_bank(pick, f"am sync {WIDE} channels", empty_first=(1,))


# ---------------------------------------------------------------- queued feeds
def chain_case(case, ch):
    """the case's stream cut into ten spans: HEAD of tests/test_demod_queued_gpu.py stretched over everything but the last span, which
    is long enough for two blocks of audio and then some"""
    in_rate, audio = case["cfg"][0], case["cfg"][2]
    B = sc.block(case["sync"][1])
    last = -(-(2 * B + 100) * in_rate // audio)
    body = case["n"] - last
    scale = body / sum(HEAD)
    spans = [m if m <= 1 else int(m * scale) + 3 * ch for m in HEAD]
    if ch == 1:
        spans[2], spans[4] = spans[4], spans[2]             # the empty and the one-sample span of the channels do not all coincide
    spans[BIG] += body - sum(spans)
    assert spans[BIG] > 4 * max(spans[:BIG]) and min(spans) == 0 and 1 in spans
    spans.append(last)
    return dict(case, splits=spans)


def test_feed_dev_chain_of_sync_channels():
    """ten feed_dev spans over streams uploaded once and nothing that synchronises in between: the five history pairs of the sync
    chain (and the envelope ones under them) are ten feeds deep, and the work buffers grow in the seventh, when the last span's
    audio and the final state are read.  The oracle is fed the same spans"""
    import torch
    cases, _, L = expected()
    chain = [chain_case(cases[i], ch) for ch, i in enumerate(CHAIN)]
    assert [(c["sync"][1], c["cfg"][0], c["cfg"][2]) for c in chain] == [(sc.DSB, 48000, 48000), (sc.USB, 1000, 1000), (sc.LSB, 96000, 44100)]
    xs = [sc.inputs(c) for c in chain]
    wants = [sc.run_oracle(L, c, x=x) for c, x in zip(chain, xs)]
    offs = [np.concatenate(([0], np.cumsum(c["splits"]))).tolist() for c in chain]
    bank = make_bank(chain)
    dev = [torch.from_numpy(x.copy()).cuda() for x in xs]
    torch.cuda.synchronize()                                # once, before the first feed: the uploads are not on the handle's stream
    for r in range(10):
        bank.feed_dev([d.data_ptr() + 4 * o[r] for d, o in zip(dev, offs)], [o[r + 1] - o[r] for o in offs])
    for ch, (case, want) in enumerate(zip(chain, wants)):
        with naming(case, ch, "am sync feed_dev chain"):
            last = want["feeds"][-1]
            assert last.size >= 2 * sc.block(case["sync"][1]) and last.any() and want["sync_probe"]["blocks"] >= 4
            assert want["opens"][-1] - want["opens"][-2] >= 2 * sc.block(case["sync"][1]), "two blocks complete inside the last span"
            assert_feeds_equal([bank.read(ch)], [last], f"chain channel {ch}")
            check_state(bank, ch, as_gold(case, want), case, -1, f"chain channel {ch}")
    del dev
    bank.close()


# ---------------------------------------------------------------- the AGC history shorter than a block
@pytest.mark.parametrize("index", [0, 1, 2])
def test_history_shorter_than_a_block_sample_by_sample(index):
    """a 1000 S/s case of the forced head alone (hn = 250, B = 1024 or 512): one feed up to B - 3 open samples, five one-sample feeds
    across the first block boundary (B - 2 ... B + 2 open samples), then the rest in one feed.  The term that leaves the moving
    average comes from the same feed's block, from the block's tail and from the carried history in turn"""
    cases, _, L = expected()
    case = cases[index]
    B = sc.block(case["sync"][1])
    assert case["cfg"][2] == 1000 and case["cfg"][0] == 1000 and case["sync"] == (1, index, 0, 0.0) and sc.agc_len(1000) < B
    x = sc.inputs(case)
    # the input after which B - 3 samples have been open: asked of the oracle, one sample at a time
    o = sc.OracleAmSync(L, case["cfg"], case["sync"])
    k = 0
    while o.sync_probe()["open"] < B - 3:
        o.feed(x[2 * k: 2 * k + 2]); k += 1
    o.close()
    splits = [k, 1, 1, 1, 1, 1, case["n"] - k - 5]
    want = sc.run_oracle(L, case, splits=splits, x=x)
    assert list(want["opens"][:6]) == [B - 3, B - 2, B - 1, B, B + 1, B + 2] and want["sync_probe"]["blocks"] >= 4
    bank = make_bank([case])
    gold = as_gold(case, want)
    got = []
    with naming(case, 0, "am sync hn < B"):
        for i, part in enumerate(sc.cut(x, splits)):
            bank.feed([part])
            got.append(bank.read(0))
            check_state(bank, 0, gold, case, i, f"{case['name']} feed {i}")
        assert_feeds_equal(got, want["feeds"], case["name"])


def test_regression_alone():
    for index in REGRESSIONS:
        run_bank([index], f"am sync case {index} alone")
