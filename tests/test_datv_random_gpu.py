"""GPU: the DATV receiver bank on datv_cases.random_cases(), 100 seeded configurations whose shares and coverage
tests/test_datv_oracle.py asserts on the CPU: banks of 33 / 33 / 34, of all 100 and of 257 channels (the draw cycled), every
channel with its own cuts, against tests/datv_oracle.cpp on the tables the handle built.  Every comparison is exact, and no draw
is skipped: create accepts all hundred."""
import numpy as np
import pytest

import sdrangel_amd as sa
from tests import datv_cases as dc
from tests.test_datv_gpu import gcfg, got_feed, tables_of

pytestmark = pytest.mark.gpu

CASES = dc.random_cases()


@pytest.fixture(scope="module")
def oracle():
    return dc.build_oracle()


@pytest.fixture(scope="module")
def runs(oracle):
    """every draw through the oracle with its own cuts, once, on the bank's tables, and left unchanged"""
    return {c["name"]: dc.run_oracle(oracle, c, tables=tables_of(c["cfg"])) for c in CASES}


@pytest.fixture(scope="module")
def xs():
    return {c["name"]: dc.inputs(c) for c in CASES}


def run_bank(cases, runs, xs):
    bank = sa.DatvBank([gcfg(c["cfg"]) for c in cases])
    parts = [dc.cut(xs[c["name"]], c["splits"]) for c in cases]
    for r in range(max(len(p) for p in parts)):
        bank.feed([p[r] if r < len(p) else p[0][:0] for p in parts])
        for i, c in enumerate(cases):
            if r < len(parts[i]):
                dc.assert_same_feed(got_feed(bank, i), runs[c["name"]]["feeds"][r], f"channel {i} {c['name']} feed {r}")


@pytest.mark.parametrize("lo,hi", [(0, 33), (33, 66), (66, 100)])
def test_the_draw_in_three_banks(runs, xs, lo, hi):
    run_bank(CASES[lo:hi], runs, xs)


def test_the_draw_in_one_bank(runs, xs):
    assert len(CASES) == 100
    run_bank(CASES, runs, xs)


def test_the_draw_cycled_over_257_channels(runs, xs):
    run_bank([CASES[(37 * i) % 100] for i in range(257)], runs, xs)


def test_every_draw_emits_symbols_and_the_design_is_the_oracles(runs):
    bank = sa.DatvBank([gcfg(c["cfg"]) for c in CASES])
    for i, c in enumerate(CASES):
        assert dc.design_words(bank.design(i)) == runs[c["name"]]["design"], c["name"]
        assert sum(f["cost"].size for f in runs[c["name"]]["feeds"]) > 0, c["name"]
    assert len({bank.table_digests(i)[2] for i in range(100)}) >= 12        # constellation tables: shared where the design is the same
