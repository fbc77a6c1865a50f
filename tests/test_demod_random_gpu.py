"""GPU: the 100 random cases of every demodulator-bank family -- random_cases() of tests/{wfm,am,nfm,ssb,udpsrc}_cases.py, the ones
the `ref` tests of tests/test_<family>_oracle.py prove against the reference sample for sample -- as mixed banks of 33, 33 and 34
channels in one handle each: three waves of psum_rows and two crossed 16-row tiles, every channel with its own resampler step and
schedule, squelch gate, delay, AGC history, block size, span, format and split list.  Then all 100 in one handle, and 257 channels
(the cases cycled): more than one 64-lane workgroup of every kernel that takes its channel from the block index.  The comparison is the one of
tests/test_<family>_gpu.py, imported from there: bit for bit, and for udpsrc formats 2 and 3 the ruling of assert_streams.

What the random cases reach is asserted on the CPU (test_random_cases_cover_the_branches in every tests/test_<family>_oracle.py).
Two probes no random case reaches stay with their named cases alone: nfm `clamped_reads` (a gate of 24000 samples or more:
gate60_clamped) and ssb `dl_wraps` (long_history).

A failure prints the channel and its case dict (cfg, sig, n, seed, splits); REGRESSIONS pins a reduced one."""
import functools

import pytest

import sdrangel_amd as sa
from tests.demod_families import FAMILIES, naming
from tests.demod_mixed import feed_rounds

pytestmark = pytest.mark.gpu
BANKS = ((0, 33), (33, 66), (66, 100))
WIDE = 257
#: (family, index into random_cases()) of cases that once failed in a bank, alone in a one-channel handle.  udpsrc 66: format 2
#: with fm_deviation 100 and gain -3, |d| up to 720; a device atan2 within 3 ulp of the host's left 244 of 5840 open samples up
#: to 4 units off, hence udp_atan2f (sdrangel_amd/csrc/udpsrc_scan.hpp)
REGRESSIONS = [("udpsrc", 66)]


@functools.lru_cache(maxsize=None)
def expected(family: str) -> tuple:
    """(cases, oracle results) of one family, computed once and shared by its banks"""
    fam = FAMILIES[family]
    cases = fam.cm.random_cases()
    assert len(cases) == 100
    L = fam.cm.build_oracle()
    return cases, [fam.cm.run_oracle(L, case) for case in cases]


def make_bank(fam, cases, where):
    try:
        return fam.Bank([fam.gcfg(c["cfg"]) for c in cases])
    except sa.SdrxError as e:
        for ch, case in enumerate(cases):                   # which one: every generated configuration is a documented one
            try:
                fam.Bank([fam.gcfg(case["cfg"])]).close()
            except sa.SdrxError as e1:
                raise AssertionError(f"{where} channel {ch}, case {case!r}: create refused it: {e1}") from e
        raise


def run_bank(fam, cases, wants, where):
    bank = make_bank(fam, cases, where)
    cuts = {}                                               # a case that sits in several channels is synthesised once
    for c in cases:
        if id(c) not in cuts:
            cuts[id(c)] = fam.cm.cut(fam.cm.inputs(c), c["splits"])
    got = feed_rounds(bank, [cuts[id(c)] for c in cases], fam.read)
    for ch, (case, want) in enumerate(zip(cases, wants)):
        with naming(case, ch, where):
            fam.check_feeds(case, got[ch], want, f"{where} channel {ch}")
            fam.check_state(bank, ch, want, f"{where} channel {ch}")
    bank.close()


@pytest.mark.parametrize("k", range(len(BANKS)))
@pytest.mark.parametrize("family", list(FAMILIES))
def test_random_cases_in_one_handle(family, k):
    cases, wants = expected(family)
    lo, hi = BANKS[k]
    run_bank(FAMILIES[family], cases[lo:hi], wants[lo:hi], f"{family} cases [{lo}:{hi}]")


@pytest.mark.parametrize("family", list(FAMILIES))
def test_all_random_cases_in_one_handle(family):
    """100 channels: a second 64-lane workgroup of the per-channel kernels, seven psum_rows waves"""
    cases, wants = expected(family)
    run_bank(FAMILIES[family], cases, wants, f"{family} all cases")


@pytest.mark.parametrize("family", list(FAMILIES))
def test_wide_bank_of_cycled_random_cases(family):
    """257 channels, channel c running case c mod 100: one channel alone in a fifth 64-lane workgroup, one row alone in a
    seventeenth psum_rows wave, a back-end schedule and a pinned pointer table wider than the 256 of the rate tools"""
    cases, wants = expected(family)
    pick = [c % len(cases) for c in range(WIDE)]
    run_bank(FAMILIES[family], [cases[i] for i in pick], [wants[i] for i in pick], f"{family} {WIDE} channels")


@pytest.mark.parametrize("family,index", REGRESSIONS)
def test_regression_alone(family, index):
    cases, wants = expected(family)
    run_bank(FAMILIES[family], [cases[index]], [wants[index]], f"{family} case {index} alone")
