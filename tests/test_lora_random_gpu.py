"""GPU: the LoRa demodulator bank (sdrx_lora_*) against the scalar oracle tests/lora_oracle.cpp, which tests/test_lora_oracle.py
ties to the reference: to the recorder feed by feed where the reference is present, and to the recorder's digests in
tests/golden/lora_random_golden.npz anywhere.  Everything is bit for bit: int16 Samples, the text, integer state.

The 100 random cases of lora_cases.random_cases() as banks of 33, 33 and 34 channels in one handle each, all 100 in one handle,
and 257 channels with the cases cycled: 65 workgroups of the walk, the last with one live wave.  Every channel is cut by its own
list, so the four waves of a walk workgroup run different n, and n = 0 once a channel's list has ended.  Then the named cases
with two and three lines in one feed, alone and as channels 3 .. 5 among random neighbours (the text slots, read_text's join and
a buffer that is too small); an arena that grows in a bank while the delay lines and the synch state are carried; two feeds
queued on the stream without a sync between them, with per-channel lengths and empty feeds on either side; reset() in a bank; and
the hand-over from a channelizer bank, where the device path, the host path and the oracle fed what the channelizer gave agree.

Out of scope here: stream counts past 2^31.  The walk is serial, so getting there takes minutes per channel, and the ABI cannot
set the count; the closed forms that take the 64-bit count are checked on the host (tests/lora_check.cpp, `angle`).

A failure prints the channel and its case dict (cfg, sig, n, seed, splits); REGRESSIONS pins a reduced one."""
import functools

import numpy as np
import pytest

import sdrangel_amd as sa
from tests import lora_cases as lc
from tests.demod_families import naming
from tests.demod_mixed import feed_rounds

pytestmark = pytest.mark.gpu
BANKS = ((0, 33), (33, 66), (66, 100))
WIDE = 257
#: indices into random_cases() of cases that once failed in a bank, run alone in a one-channel handle
REGRESSIONS = []


def gcfg(cfg) -> sa.LoraCfg:
    return sa.LoraCfg(in_rate=int(cfg[0]), nco_freq=int(cfg[1]), bandwidth=int(cfg[2]))


@functools.lru_cache(maxsize=None)
def oracle():
    return lc.build_oracle()


@functools.lru_cache(maxsize=None)
def expected() -> tuple:
    """(the random cases, their oracle results), computed once and left unchanged"""
    cases = lc.random_cases()
    assert len(cases) == 100
    return cases, [lc.run_oracle(oracle(), c) for c in cases]


@functools.lru_cache(maxsize=None)
def expected_named() -> dict:
    return {c["name"]: (c, lc.run_oracle(oracle(), c)) for c in lc.NAMED}


@functools.lru_cache(maxsize=None)
def cuts_of(name: str):
    """a case's input cut by its own list, synthesised once"""
    case = {c["name"]: c for c in lc.random_cases() + lc.NAMED}[name]
    return lc.cut(lc.inputs(case), case["splits"])


def read(bank, ch):
    return bank.read(ch), bank.read_text(ch)


def idle(bank, ch) -> int:
    return bank.read(ch).shape[0] + len(bank.read_text(ch))


def state_of(bank, ch):
    st = bank.state(ch)
    return [getattr(st, k) for k in lc.STATE]


def check_feed(got, want: dict, i: int, what):
    """got: (Samples, text) of one feed; want: the oracle's result, feed i of it"""
    samples, text = got
    w = want["feeds"][i]
    assert samples.shape == w.shape, (what, "feed", i, samples.shape, w.shape)
    bad = (samples != w).any(axis=1)
    assert not bad.any(), (what, "feed", i, int(np.count_nonzero(bad)), "of", w.shape[0], "Samples differ, the first at", int(np.flatnonzero(bad)[0]))
    assert text == want["texts"][i], (what, "feed", i, text, want["texts"][i])


def check_channel(bank, ch, case, got, want, where):
    with naming(case, ch, where):
        assert len(got) == len(want["feeds"])
        for i, g in enumerate(got):
            check_feed(g, want, i, f"{where} channel {ch}")
        assert state_of(bank, ch) == lc.state_list(want["counters"][-1]), (where, ch, state_of(bank, ch), want["counters"][-1])


def run_bank(cases, wants, where):
    bank = sa.LoraDemodBank([gcfg(c["cfg"]) for c in cases])
    got = feed_rounds(bank, [cuts_of(c["name"]) for c in cases], read, idle)
    for ch, (case, want) in enumerate(zip(cases, wants)):
        check_channel(bank, ch, case, got[ch], want, where)
    bank.close()


# ---------------------------------------------------------------- the random cases
@pytest.mark.parametrize("k", range(len(BANKS)))
def test_random_cases_in_one_handle(k):
    cases, wants = expected()
    lo, hi = BANKS[k]
    run_bank(cases[lo:hi], wants[lo:hi], f"lora cases [{lo}:{hi}]")


def test_all_random_cases_in_one_handle():
    """100 channels: 25 workgroups of the walk"""
    cases, wants = expected()
    run_bank(cases, wants, "lora all cases")


def test_wide_bank_of_cycled_random_cases():
    """257 channels, channel c running case c mod 100: 65 workgroups of the walk, the last with one live wave"""
    cases, wants = expected()
    pick = [c % len(cases) for c in range(WIDE)]
    run_bank([cases[i] for i in pick], [wants[i] for i in pick], f"lora {WIDE} channels")


def test_regression_alone():
    cases, wants = expected()
    for index in REGRESSIONS:
        run_bank([cases[index]], [wants[index]], f"lora case {index} alone")


# ---------------------------------------------------------------- more than one line in a feed; the tie above zero
@pytest.mark.parametrize("name", [c["name"] for c in lc.NAMED])
def test_named_case_alone(name):
    case, want = expected_named()[name]
    run_bank([case], [want], name)


@pytest.mark.parametrize("names", [("two_lines_one_feed", "three_lines_one_feed", "three_lines_late"),
                                   ("three_lines_short_feed", "three_lines_late", "two_lines_one_feed")], ids=["whole", "cut"])
def test_lines_as_channels_3_to_5_among_random_neighbours(names):
    """the text slots of neighbours in one walk workgroup and the next: channels 3, 4 and 5 end two and three lines in a feed
    while the channels around them run random cases"""
    cases, wants = expected()
    named = [expected_named()[n] for n in names]
    order = [(cases[i], wants[i]) for i in (0, 9, 21)] + named + [(cases[i], wants[i]) for i in (54, 77)]
    assert all(w["counters"][-1]["lines"] >= 1 for _, w in order)            # the neighbours print lines of their own
    run_bank([c for c, _ in order], [w for _, w in order], "lines in channels 3 .. 5")


def test_read_text_of_several_lines_with_a_buffer_that_is_too_small():
    case, want = expected_named()["three_lines_one_feed"]
    bank = sa.LoraDemodBank([gcfg(case["cfg"])] * 2)
    x = lc.inputs(case)
    bank.feed([x, x[:2000]])
    text = want["texts"][0]
    assert text.count("\n") == 3
    with pytest.raises(sa.SdrxError, match="too small"):
        bank.read_text(0, cap=len(text) - 1)
    assert bank.read_text(0, cap=len(text)) == text and bank.read_text(0) == text
    assert bank.read_text(1) == ""
    bank.close()


# ---------------------------------------------------------------- the arena grows in a bank
def test_arena_growth_in_a_bank():
    """eight channels get feeds of 1, 64 and 200 samples and then the rest in one feed, many times the longest so far: the work
    arena grows while the delay lines and the synch state are carried"""
    cases, _ = expected()
    pick = [0, 2, 9, 21, 23, 32, 37, 47]
    chosen = [cases[i] for i in pick]
    assert all(c["n"] > 20 * 265 for c in chosen)
    splits = [[1, 64, 200, c["n"] - 265] for c in chosen]
    wants = [lc.run_oracle(oracle(), c, splits=s) for c, s in zip(chosen, splits)]
    assert sum(w["counters"][-1]["lines"] for w in wants) >= 4
    bank = sa.LoraDemodBank([gcfg(c["cfg"]) for c in chosen])
    got = feed_rounds(bank, [lc.cut(lc.inputs(c), s) for c, s in zip(chosen, splits)], read, idle)
    for ch, (case, want) in enumerate(zip(chosen, wants)):
        check_channel(bank, ch, case, got[ch], want, "arena growth")
    bank.close()


# ---------------------------------------------------------------- queued feeds, reset
def test_queued_feeds_in_a_bank_without_a_sync():
    """33 channels, feed_dev twice with nothing between: per-channel lengths, every fifth channel empty in the first call, every
    seventh in the second.  After one sync the second feed's Samples and text and the state behind both equal the oracle's"""
    torch = pytest.importorskip("torch")
    cases, _ = expected()
    chosen = cases[:33]
    firsts = []
    for ch, c in enumerate(chosen):
        a = (c["n"] * (3 + ch % 5)) // 9
        firsts.append(0 if ch % 5 == 0 else c["n"] if ch % 7 == 0 else a)
    assert 0 in firsts and any(f == c["n"] for f, c in zip(firsts, chosen))
    splits = [[f, c["n"] - f] for f, c in zip(firsts, chosen)]
    wants = [lc.run_oracle(oracle(), c, splits=s) for c, s in zip(chosen, splits)]
    dev = [torch.from_numpy(np.concatenate([lc.inputs(c), np.zeros(2, np.int16)])).cuda() for c in chosen]      # never empty
    torch.cuda.synchronize()
    bank = sa.LoraDemodBank([gcfg(c["cfg"]) for c in chosen])
    bank.feed_dev([d.data_ptr() for d in dev], [s[0] for s in splits])
    bank.feed_dev([d.data_ptr() + 4 * s[0] for d, s in zip(dev, splits)], [s[1] for s in splits])
    bank.sync()
    for ch, (case, want) in enumerate(zip(chosen, wants)):
        with naming(case, ch, "queued feeds"):
            check_feed(read(bank, ch), want, 1, f"queued feeds channel {ch}")
            assert state_of(bank, ch) == lc.state_list(want["counters"][-1])
    bank.close()


def test_reset_in_a_bank():
    """33 channels fed half their streams, reset, then fed whole: every channel as from a fresh start"""
    cases, _ = expected()
    chosen = cases[33:66]
    xs = [lc.inputs(c) for c in chosen]
    wants = [lc.run_oracle(oracle(), c, splits=[c["n"]]) for c in chosen]
    bank = sa.LoraDemodBank([gcfg(c["cfg"]) for c in chosen])
    bank.feed([x[: 2 * (c["n"] // 2)] for x, c in zip(xs, chosen)])
    assert any(state_of(bank, ch)[5] > 0 for ch in range(len(chosen)))      # lines were printed before the reset
    bank.reset()
    for ch in range(len(chosen)):
        assert state_of(bank, ch) == [0, 0, 0, 0, 0, 0], ch
    bank.feed(xs)
    for ch, (case, want) in enumerate(zip(chosen, wants)):
        check_channel(bank, ch, case, [read(bank, ch)], want, "after reset")
    bank.close()


# ---------------------------------------------------------------- behind a channelizer bank
def test_feed_bank_behind_a_channelizer_bank_equals_the_oracle():
    """four channels of different rates and bandwidths: the hand-over on the device, feeding what the channelizer bank's read()
    returns, and the oracle fed the same, feed by feed"""
    rng = np.random.default_rng(5)
    rate = 4 * 62500
    x = rng.integers(-3000, 3000, 2 * 40000).astype(np.int16)
    chan = sa.ChannelizerBank(rate, [62500, 62500, 31250, 31250], [0, 31250, -62500, 15625])
    rates = [chan.info(c)[1] for c in range(4)]
    cfgs = [(rates[0], 0, 62500), (rates[1], -1000, 31250), (rates[2], 500, 20833), (rates[3], 0, 7813)]
    assert all(cfg[2] <= cfg[0] for cfg in cfgs)
    on_dev, on_host = sa.LoraDemodBank([gcfg(c) for c in cfgs]), sa.LoraDemodBank([gcfg(c) for c in cfgs])
    outs = [[] for _ in cfgs]
    got_dev, got_host = [[] for _ in cfgs], [[] for _ in cfgs]
    for part in (x[:30000], x[30000:]):
        chan.feed(part)
        on_dev.feed_bank(chan)
        given = [chan.read(c) for c in range(4)]
        on_host.feed(given)
        for c in range(4):
            outs[c].append(given[c])
            got_dev[c].append(read(on_dev, c)); got_host[c].append(read(on_host, c))
    for c, cfg in enumerate(cfgs):
        want = lc.run_spans(oracle(), cfg, outs[c])
        assert sum(f.shape[0] for f in want["feeds"]) > 1000
        for i in range(2):
            check_feed(got_dev[c][i], want, i, f"device path channel {c}")
            check_feed(got_host[c][i], want, i, f"host path channel {c}")
        assert state_of(on_dev, c) == state_of(on_host, c) == lc.state_list(want["counters"][-1])
