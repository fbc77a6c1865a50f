"""GPU: the ATV demodulator bank (sdrx_atv_*) on the 100 random configurations of atv_cases.random_cases() against
tests/atv_oracle.cpp, which tests/test_atv_oracle.py ties to the reference on these very cases (to the recorder feed by feed where
the reference is present, to its digests in tests/golden/atv_random_golden.npz anywhere).  Everything is exact: events, stored
frames, screen, scope stream and the state's 28 words after every feed.

The draw: lines of 9 to 700 samples and tops of 0 to a third of the line, all six standards and four modulations, both syncs on and
off, the levels, offsets up to half the rate, the decimator and the FFT filter, video with and without loss, noise, constants,
zeros and clipped input; at least half of it is FM under a classic standard (the stretch walk) and a tenth has a top of 64 samples
or more.  As banks of 33, 33 and 34 channels in one handle each, all 100 in one handle, and 257 channels with the cases cycled (65
workgroups of the walk, the last with one live wave).  Every channel is cut by its own list, so the four waves of a walk workgroup
run different lengths, and none once a channel's list has ended; in the wide bank one channel gets nothing in the first call.

A failure prints the channel and its case dict (cfg, sig, n, seed, splits); REGRESSIONS pins a reduced one."""
import functools

import pytest

import sdrangel_amd as sa
from tests import atv_cases as ac
from tests.demod_families import naming
from tests.demod_mixed import feed_rounds
from tests.test_atv_gpu import assert_feed, gcfg, got_feed

pytestmark = pytest.mark.gpu
BANKS = ((0, 33), (33, 66), (66, 100))
WIDE = 257
#: indices into random_cases() of cases that once failed in a bank, run alone in a one-channel handle
REGRESSIONS = []


@functools.lru_cache(maxsize=None)
def expected() -> tuple:
    """(the random cases, their oracle results), computed once and left unchanged"""
    cases = ac.random_cases()
    ac.assert_random_shares(cases)
    L = ac.build_oracle()
    return cases, [ac.run_oracle(L, c) for c in cases], L


@functools.lru_cache(maxsize=None)
def cuts_of(name: str, lead_empty: bool = False):
    """a case's input cut by its own list, synthesised once"""
    case = {c["name"]: c for c in expected()[0]}[name]
    return ac.cut(ac.inputs(case), ([0] if lead_empty else []) + case["splits"])


def idle(bank, ch) -> int:
    return bank.read(ch).size + bank.frames(ch)[1]


def run_bank(cases, wants, where, empty_first=()):
    """channel c runs cases[c] cut by its own list; the channels of `empty_first` get an empty feed before it"""
    bank = sa.ATVBank([gcfg(c["cfg"]) for c in cases])
    for ch, (case, want) in enumerate(zip(cases, wants)):
        assert ac.design_words(bank.design(ch)) == want["design"], (where, ch, case)
    got = feed_rounds(bank, [cuts_of(c["name"], ch in empty_first) for ch, c in enumerate(cases)], got_feed, idle)
    for ch, (case, want) in enumerate(zip(cases, wants)):
        with naming(case, ch, where):
            feeds = got[ch]
            if ch in empty_first:
                assert feeds[0]["n_events"] == 0 and feeds[0]["scope"].size == 0 and not feeds[0]["screen"].any()
                feeds = feeds[1:]
            assert len(feeds) == len(want["feeds"])
            for i, g in enumerate(feeds):
                assert_feed(g, want["feeds"][i], f"{where} channel {ch} {case['name']} feed {i}", case["cfg"]["frames_cap"])


@pytest.mark.parametrize("k", range(len(BANKS)))
def test_random_cases_in_one_handle(k):
    cases, wants, _ = expected()
    lo, hi = BANKS[k]
    run_bank(cases[lo:hi], wants[lo:hi], f"atv cases [{lo}:{hi}]")


def test_all_random_cases_in_one_handle():
    """100 channels: 25 workgroups of the walk"""
    cases, wants, _ = expected()
    run_bank(cases, wants, "atv all cases")


def test_wide_bank_of_cycled_random_cases():
    """257 channels, channel c running case c mod 100: 65 workgroups of the walk, the last with one live wave; channel 1 is fed
    nothing in the first call and runs one call behind its neighbours"""
    cases, wants, _ = expected()
    pick = [c % len(cases) for c in range(WIDE)]
    run_bank([cases[i] for i in pick], [wants[i] for i in pick], f"atv {WIDE} channels", empty_first=(1,))


def test_regression_alone():
    cases, wants, _ = expected()
    for index in REGRESSIONS:
        run_bank([cases[index]], [wants[index]], f"atv case {index} alone")
