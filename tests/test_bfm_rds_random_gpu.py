"""GPU: RDS in the broadcast-FM bank (sdrx_bfmrds_*) on the 40 random configurations of bfm_rds_cases.random_cases() against the
recording of the reference's own classes (tests/golden/bfm_rds_random_golden.npz): bits, groups, subcarr_bb, report and the 43 state
words after every feed, by tests/test_bfm_rds_gpu.assert_feed_equals, and no unsure sample on any channel.  There is no portable RDS
oracle: the 57 kHz mixer's cosine is the host libm's.

The draw: seven rates, RDS steps from 0.384 to 2 -- below 1 the schedule is clamped and every input emits -- audio at 48000 and
44100, mono and stereo, random subcarrier level, phase and lead, bursts that close the squelch, noise, zeros, and four cases past
the 800th biphase call.  All 40 in one handle; interleaved with 25 RDS-off channels of bfm_cases.random_cases() in a handle of 65
(two workgroups of bfm_rds_sched_kernel), the plain ones against tests/bfm_oracle.c; and 130 channels cycled over the shorter cases.

A failure prints the channel and its case dict; REGRESSIONS pins a reduced one."""
import functools

import numpy as np
import pytest

import sdrangel_amd as sa
from tests import bfm_cases as bc
from tests import bfm_rds_cases as rc
from tests import test_bfm_random_gpu as plain
from tests.demod_families import naming
from tests.demod_mixed import feed_rounds
from tests.test_bfm_gpu import check_open, gcfg
from tests.test_bfm_rds_gpu import assert_feed_equals, snapshot

pytestmark = pytest.mark.gpu
WIDE, PLAIN = 130, 25
#: indices into random_cases() of cases that once failed in a bank, run alone in a one-channel handle
REGRESSIONS = []


@functools.lru_cache(maxsize=None)
def expected() -> tuple:
    """(the random RDS cases, the recording by case name), loaded once and left unchanged"""
    cases, gold = rc.random_cases(), rc.load_random_golden()
    rc.assert_random_shares(cases, gold)
    return cases, gold


@functools.lru_cache(maxsize=None)
def cuts_of(name: str, lead_empty: bool = False):
    """a case's input cut by its own list, synthesised once"""
    if name.startswith("rds_"):
        case = {c["name"]: c for c in expected()[0]}[name]
        x = rc.inputs(case)
        assert bc.sha(x) == expected()[1][name]["in_sha"], "the generator gave other samples than the recorder was fed"
    else:
        return plain.cuts_of(name, lead_empty)
    return bc.cut(x, ([0] if lead_empty else []) + case["splits"])


def run_bank(chans, where, empty_first=()):
    """chans: (case, rds on) per channel, each cut by its own list; RDS channels against the recording, plain ones against
    tests/bfm_oracle.c"""
    gold = expected()[1]
    on = [bool(r) for _, r in chans]
    bank = sa.BfmBank([gcfg(c["cfg"]) for c, _ in chans], rds=[int(r) for r in on])
    read = lambda b, ch: snapshot(b, ch) if on[ch] else plain.got_feed(b, ch)
    idle = lambda b, ch: b.rds_bits(ch).size + b.rds_bb(ch).size + b.rds_groups(ch).shape[0] if on[ch] else plain.idle(b, ch)
    got = feed_rounds(bank, [cuts_of(c["name"], ch in empty_first) for ch, (c, _) in enumerate(chans)], read, idle)
    for ch, (case, r) in enumerate(chans):
        with naming(case, ch, where):
            feeds = got[ch]
            what = f"{where} channel {ch} {case['name']}"
            if ch in empty_first:
                assert on[ch] and feeds[0]["bits"].size == 0 and feeds[0]["bb"].size == 0 and feeds[0]["groups"].shape[0] == 0
                feeds = feeds[1:]
            if on[ch]:
                want = gold[case["name"]]
                assert len(feeds) == len(want["n_rds"])
                for i, f in enumerate(feeds):
                    assert_feed_equals(f, want, i, what)
                assert bank.rds_unsure(ch) == 0, "a sample whose mixer product the enclosure does not pin"
            else:
                want = plain.expected()[1][int(case["name"][len("random"):])]
                g = {"audio": [f["audio"] for f in feeds], "sink": [f["sink"] for f in feeds], "states": [f["state"] for f in feeds]}
                bc.assert_equals_recording(g, want, what, state_keys=plain.STATE_KEYS)
                check_open(g, want, case["cfg"], what)
                for call in (bank.rds_bits, bank.rds_groups, bank.rds_report, bank.rds_state, bank.rds_unsure):
                    with pytest.raises(sa.SdrxError, match="without RDS"):
                        call(ch)
    return bank


def test_random_rds_cases_in_one_handle():
    """40 channels, RDS on in all: 10 workgroups of each walk, every RDS step in one handle"""
    cases, _ = expected()
    run_bank([(c, 1) for c in cases], "rds all cases")


def test_rds_and_plain_channels_interleaved():
    """65 channels: the 40 RDS cases and 25 RDS-off cases of the plain draw, alternating -- two workgroups of the 64-lane kernels,
    bfm_rds_sched_kernel among them, walk workgroups with RDS waves next to plain ones"""
    cases, _ = expected()
    off = plain.expected()[0][:PLAIN]
    chans = []
    for i, c in enumerate(cases):
        chans.append((c, 1))
        if i < len(off):
            chans.append((off[i], 0))
    assert len(chans) == 65 and [r for _, r in chans[:50]] == [1, 0] * 25 and {c["cfg"]["stereo"] for c in off} == {0, 1}
    run_bank(chans, "rds and plain interleaved")


def test_wide_rds_bank():
    """130 channels over the RDS cases of at most WIDE_N samples, cycled: 33 workgroups of the walks, three of the 64-lane kernels;
    clamped schedules and steps above 1 side by side; channel 1 is fed nothing in the first call"""
    cases, _ = expected()
    short = [c for c in cases if c["n"] <= rc.WIDE_N]
    chans = [(short[ch % len(short)], 1) for ch in range(WIDE)]
    assert sum(rc.rds_step(c) < 1 for c, _ in chans) >= 20 and sum(rc.rds_step(c) > 1 for c, _ in chans) >= 20
    run_bank(chans, f"rds {WIDE} channels", empty_first=(1,))


def test_regression_alone():
    cases, _ = expected()
    for index in REGRESSIONS:
        run_bank([(cases[index], 1)], f"rds case {index} alone")
