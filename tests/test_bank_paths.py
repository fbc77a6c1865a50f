"""Which branches of tree_kernel.hpp the bank's plans select, checked on the host (tests/chan_plan_paths.cpp, no GPU): every case of
tests/bank_path_cases.py still takes the paths it is there for, the cases together take every path either engine can take, and
a seeded sweep of random banks under every option set finds no path outside that vocabulary -- so a planner change that opens a
new kernel path fails here until a case (and with it tests/test_bank_paths_gpu.py) covers it."""
import tempfile

import numpy as np
import pytest

from tests import bank_path_cases as B


@pytest.fixture(scope="module")
def lister():
    return B.build_lister(tempfile.mkdtemp())


@pytest.mark.parametrize("case", B.CASES, ids=[c["name"] for c in B.CASES])
def test_case_takes_its_paths(lister, case):
    got = B.case_paths(lister, case)
    for e in B.ENGINES:
        missing = set(case["paths"][e]) - got[e]
        assert not missing, (e, sorted(missing))
        assert got[e] <= set(B.REACHABLE[e]), (e, sorted(got[e] - set(B.REACHABLE[e])))


def test_vocabulary_is_covered_per_engine():
    for e in B.ENGINES:
        assert set(B.UNREACHABLE[e]) <= set(B.VOCAB)
        claimed = set().union(*(c["paths"][e] for c in B.CASES))
        assert claimed <= set(B.REACHABLE[e]), (e, sorted(claimed - set(B.REACHABLE[e])))
        assert claimed == set(B.REACHABLE[e]), (e, sorted(set(B.REACHABLE[e]) - claimed))


def test_deepest_case_at_61M(lister):
    """the 17-stage chain: the deepest one the GPU test's feed (5.4 M samples) still gets 40 outputs from at 61.44 MS/s"""
    case = next(c for c in B.CASES if c["name"] == "deep17_61M")
    (r,) = B.run_lister(lister, [B.lister_line("mfma", case["options"], case["in_rate"], case["channels"])])
    assert case["in_rate"] == 61_440_000 and r["depth"] == 17


def test_random_plans_stay_inside_the_vocabulary(lister):
    rng = np.random.default_rng(8)
    banks = [B.random_bank(rng) for _ in range(6000)]
    lines = [B.lister_line(e, o, ir, ch) for ir, ch in banks for o in B.OPTIONS for e in B.ENGINES]
    res = B.run_lister(lister, lines)
    planned = 0
    seen = {e: set() for e in B.ENGINES}
    for line, r in zip(lines, res):
        if r["error"]:
            continue
        planned += 1
        e = line.split()[0]
        outside = set(r["paths"]) - set(B.REACHABLE[e])
        assert not outside, (sorted(outside), line)
        seen[e].update(r["paths"])
    assert planned >= 0.99 * len(lines)
    for e in B.ENGINES:                                     # the sweep itself is wide: most of the vocabulary shows up
        assert len(seen[e]) >= 0.9 * len(B.REACHABLE[e]), (e, sorted(set(B.REACHABLE[e]) - seen[e]))
