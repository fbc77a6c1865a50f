"""GPU: the broadcast-FM stereo demodulator bank (sdrx_bfm_*) on the 100 random configurations of bfm_cases.random_cases() against
tests/bfm_oracle.c, which tests/test_bfm_oracle.py ties to the reference on these very cases (to the recorder feed by feed where
the reference is present, to its digests in tests/golden/bfm_random_golden.npz anywhere).  The rules are those of
bfm_cases.assert_equals_recording: every l, r pair, every Sample of the sink stream, m_magsqCount, locked(), m_magsqPeak and the
bits of m_pilot_level, m_freq and m_phase exact after every feed, m_magsqSum inside the reorder bound, squelch_open() as
test_bfm_gpu.check_open reads it; and per channel every design product (taps, filter, NCO step, level, loop constants, lock delay,
de-emphasis constants) equal to the oracle's.

The draw: fifteen (in_rate, audio_rate) pairs -- audio at 48000, 44100, 32000 and 8000, steps of 1, 1.0000208 and 1.088 next to 12,
the closed form's fractional steps 2.5, 1.25 and 1.5 -- so that max_out, the schedule (closed form or serial walk) and the
de-emphasis constants differ from channel to channel of one handle; all of af, volume, squelch level; mono and stereo, lsb, the pilot on the sink stream; pilots on, off and off frequency,
bursts that open and close the squelch inside blocks, clipped input, noise and zeros; six cases long enough to lock.  As banks of
33, 33 and 34 channels in one handle each, all 100 in one handle (25 workgroups of the walk, two of the 64-lane kernels), and 257
channels with the shorter cases cycled (65 workgroups of the walk, the last with one live wave; five of the 64-lane kernels).
Every channel is cut by its own list; in the wide bank one channel gets nothing in the first call.

A failure prints the channel and its case dict (cfg, sig, n, seed, splits); REGRESSIONS pins a reduced one."""
import functools

import numpy as np
import pytest

import sdrangel_amd as sa
from tests import bfm_cases as bc
from tests.demod_families import naming
from tests.demod_mixed import feed_rounds
from tests.test_bfm_gpu import check_open, gcfg, state

pytestmark = pytest.mark.gpu
BANKS = ((0, 33), (33, 66), (66, 100))
WIDE = 257
STATE_KEYS = ("count", "locked", "peak")
#: indices into random_cases() of cases that once failed in a bank, run alone in a one-channel handle
REGRESSIONS = []
#: the named cases of the serial-schedule test: closed form by their steps (5, 8, 2, 5)
SERIAL_NAMED = ("stereo_240k", "lsb_384k", "lock_96k", "mono_240k_one_feed")


def as_recording(run: dict) -> dict:
    """run_oracle()'s result in golden_case()'s layout"""
    return {"audio": run["audio"], "sink": run["sink"], "sink_counts": [int(s.size) for s in run["sink"]], "sink_sha": [bc.sha(s) for s in run["sink"]],
            "states": run["states"]}


@functools.lru_cache(maxsize=None)
def expected() -> tuple:
    """(the random cases, their oracle results, each channel's design products, the oracle), computed once and left unchanged"""
    cases = bc.random_cases()
    L = bc.build_oracle()
    runs = [bc.run_oracle(L, c) for c in cases]
    bc.assert_random_shares(cases, runs)
    return cases, [as_recording(r) for r in runs], [bc.OracleBfm(L, c["cfg"]).design() for c in cases], L


@functools.lru_cache(maxsize=None)
def named() -> tuple:
    cases = [{c["name"]: c for c in bc.CASES}[n] for n in SERIAL_NAMED]
    L = expected()[3]
    return cases, [as_recording(bc.run_oracle(L, c)) for c in cases], [bc.OracleBfm(L, c["cfg"]).design() for c in cases]


@functools.lru_cache(maxsize=None)
def cuts_of(name: str, lead_empty: bool = False):
    """a case's input cut by its own list, synthesised once"""
    case = {c["name"]: c for c in expected()[0] + named()[0]}[name]
    return bc.cut(bc.inputs(case), ([0] if lead_empty else []) + case["splits"])


def got_feed(bank, ch) -> dict:
    k = bank.read_sink(ch)
    assert not np.any(k[:, 1])
    return {"audio": bank.read(ch), "sink": k[:, 0].copy(), "state": state(bank, ch, None)}


def idle(bank, ch) -> int:
    return bank.read(ch).shape[0] + bank.read_sink(ch).shape[0]


def assert_design(bank, ch, want):
    """as test_bfm_gpu.test_design_products_equal_the_oracle compares them"""
    g = bank.design(ch)
    assert g[0] == want[0] == 72 and g[3] == want[3] and g[6] == want[6], "taps per phase, NCO step or lock delay"
    for i in (1, 2, 5, 7):
        assert np.array_equal(g[i].view(np.uint32), want[i].view(np.uint32)), ("design product", i)
    assert np.float32(g[4]) == np.float32(want[4]), "squelch level"


def run_bank(cases, wants, designs, where, empty_first=()):
    """channel c runs cases[c] cut by its own list; the channels of `empty_first` get an empty feed before it.  Returns the bank and
    what it gave, per channel in run_oracle's layout"""
    bank = sa.BfmBank([gcfg(c["cfg"]) for c in cases])
    for ch, (case, d) in enumerate(zip(cases, designs)):
        with naming(case, ch, where):
            assert_design(bank, ch, d)
    got = feed_rounds(bank, [cuts_of(c["name"], ch in empty_first) for ch, c in enumerate(cases)], got_feed, idle)
    out = []
    for ch, (case, want) in enumerate(zip(cases, wants)):
        with naming(case, ch, where):
            feeds = got[ch]
            if ch in empty_first:
                f = feeds[0]
                assert f["audio"].shape[0] == 0 and f["sink"].size == 0 and f["state"]["count"] == 0 and not f["state"]["open"]
                feeds = feeds[1:]
            assert len(feeds) == len(want["audio"])
            g = {"audio": [f["audio"] for f in feeds], "sink": [f["sink"] for f in feeds], "states": [f["state"] for f in feeds]}
            what = f"{where} channel {ch} {case['name']}"
            bc.assert_equals_recording(g, want, what, state_keys=STATE_KEYS)
            check_open(g, want, case["cfg"], what)
            out.append(g)
    return bank, out


def mix_of(cases) -> set:
    return {(bc.is_dyadic(c), c["cfg"]["stereo"]) for c in cases}


EVERY_MIX = {(False, 0), (False, 1), (True, 0), (True, 1)}


@pytest.mark.parametrize("k", range(len(BANKS)))
def test_random_cases_in_one_handle(k):
    cases, wants, designs, _ = expected()
    lo, hi = BANKS[k]
    assert mix_of(cases[lo:hi]) == EVERY_MIX, "both schedules, stereo and mono"
    run_bank(cases[lo:hi], wants[lo:hi], designs[lo:hi], f"bfm cases [{lo}:{hi}]")


def test_all_random_cases_in_one_handle():
    """100 channels: 25 workgroups of the walk, two of bfm_prep_kernel, bfm_sched_walk_kernel, bfm_blockscan_kernel and
    bfm_lastopen_kernel"""
    cases, wants, designs, _ = expected()
    bank, _ = run_bank(cases, wants, designs, "bfm all cases")
    ll = bank.last_launch()
    assert ll["kernel"] == "bfm_walk_kernel" and ll["grid"] == 25 and ll["block"] == 256, ll


def test_wide_bank_of_cycled_random_cases():
    """257 channels over the cases of at most WIDE_N samples, cycled: 65 workgroups of the walk, the last with one live wave, five
    of the 64-lane kernels; channel 1 is fed nothing in the first call and runs one call behind its neighbours"""
    cases, wants, designs, _ = expected()
    short = [i for i, c in enumerate(cases) if c["n"] <= bc.WIDE_N]
    assert len(short) >= 40 and mix_of([cases[i] for i in short]) == EVERY_MIX
    pick = [short[c % len(short)] for c in range(WIDE)]
    bank, _ = run_bank([cases[i] for i in pick], [wants[i] for i in pick], [designs[i] for i in pick], f"bfm {WIDE} channels", empty_first=(1,))
    ll = bank.last_launch()
    assert ll["kernel"] == "bfm_walk_kernel" and ll["grid"] == 65, ll


def test_serial_schedule_switch(monkeypatch):
    """SDRX_BFM_SERIAL_SCHEDULE=1 (read by sdrx_bfm_create): bfm_sched_walk_kernel on the steps that bfm_prep_kernel and
    bfm_sched_fill_kernel otherwise take in closed form -- four named cases and the first 12 random cases with such a step in one
    handle, walk and closed form against the same oracle on the same channels, and against each other"""
    cases, wants, designs, _ = expected()
    pick = [i for i, c in enumerate(cases) if bc.is_dyadic(c)][:12]
    ncases, nwants, ndesigns = named()
    assert len(pick) == 12 and all(bc.is_dyadic(c) for c in ncases)
    both = []
    for serial in (False, True):
        if serial:
            monkeypatch.setenv("SDRX_BFM_SERIAL_SCHEDULE", "1")
        else:
            monkeypatch.delenv("SDRX_BFM_SERIAL_SCHEDULE", raising=False)
        _, got = run_bank(ncases + [cases[i] for i in pick], nwants + [wants[i] for i in pick], ndesigns + [designs[i] for i in pick],
                          "bfm serial schedule" if serial else "bfm closed form")
        both.append(got)
    for ch, (a, b) in enumerate(zip(*both)):
        for i in range(len(a["audio"])):
            assert np.array_equal(a["audio"][i], b["audio"][i]) and np.array_equal(a["sink"][i], b["sink"][i]), (ch, i)
            sa_, sb = a["states"][i], b["states"][i]
            assert np.array_equal(sa_["bits"], sb["bits"]) and all(sa_[k] == sb[k] for k in ("peak", "count", "locked", "open")), (ch, i)


def test_regression_alone():
    cases, wants, designs, _ = expected()
    for index in REGRESSIONS:
        run_bank([cases[index]], [wants[index]], [designs[index]], f"bfm case {index} alone")
