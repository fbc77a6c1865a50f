"""The lowering of the bank plan for the lean kernel (sdrangel_amd/csrc/chan_lower.cpp, tree_mx_kernel.hpp), without a GPU.

tests/chan_lower_check.cpp plans a bank, lowers it and checks, for every pass the lean kernel runs: each lowered job touches the
same LDS bytes as the TkMJob it came from, a level's jobs are a permutation sorted by class, no store of a level meets another
access of that level, and everything stays inside the pass's LDS.  The cases: every bank of tests/golden/chan_plan_tables.json
(both engines, the deep-pass option sets included) and a few thousand seeded random banks under the option sets of
tests/bank_path_cases.py."""
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

from tests.bank_path_cases import OPTIONS, random_bank

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sdrangel_amd", "csrc")
with open(os.path.join(ROOT, "tests", "golden", "chan_plan_tables.json")) as _f:
    GOLDEN = json.load(_f)["cases"]


@pytest.fixture(scope="module")
def checker():
    exe = os.path.join(tempfile.mkdtemp(), "chan_lower_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-I" + CSRC,
                           os.path.join(ROOT, "tests", "chan_lower_check.cpp"), os.path.join(CSRC, "chan_plan.cpp"),
                           os.path.join(CSRC, "chan_lower.cpp"), "-o", exe])
    return exe


def _run(exe, lines):
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=600, check=True)
    return [json.loads(l) for l in out.stdout.splitlines()]


def _line(engine, lds_kb, max_levels, in_rate, channels):
    return f"{engine} {lds_kb} {max_levels} {in_rate} {len(channels)} " + " ".join(f"{i} {r} {f}" for i, (r, f) in enumerate(channels))


@pytest.mark.parametrize("case", GOLDEN, ids=[f"{c['name']}-{c['engine']}" for c in GOLDEN])
def test_golden_banks_lower_exactly(checker, case):
    (got,) = _run(checker, [_line(case["engine"], case["lds_kb"], case["max_levels"], case["in_rate"], [(r, f) for _, r, f in case["channels"]])])
    assert got["error"] == "" and got["lower"] == ""
    assert got["bad"] == []
    if case["engine"] == "valu":
        assert got["mx_passes"] == 0                      # the VALU engine never runs the lean kernel
    elif case["max_levels"] == 0:
        assert got["mx_passes"] == got["passes"] > 0      # default plans: every pass is all matrix-core
        assert got["jobs"] > 0


def test_default_banks_run_the_lean_kernel(checker):
    # the benchmark's banks: every pass on the lean kernel, and the branch-free class carries a share of the jobs
    for name in ("cfg3_32", "chan128", "cfg4"):
        case = next(c for c in GOLDEN if c["name"] == name and c["engine"] == "mfma")
        (got,) = _run(checker, [_line("mfma", 0, 0, case["in_rate"], [(r, f) for _, r, f in case["channels"]])])
        assert got["mx_passes"] == got["passes"]
        assert got["classes"][0] > 0 and sum(got["classes"]) == got["jobs"]


@pytest.mark.parametrize("opt", sorted(OPTIONS))
def test_random_banks_lower_exactly(checker, opt):
    rng = np.random.default_rng(20261016 + sorted(OPTIONS).index(opt))
    ml, kb = OPTIONS[opt] or (0, 0)
    lines = []
    for _ in range(1000):
        ir, ch = random_bank(rng)
        lines.append(_line("mfma", kb, ml, ir, ch))
    res = _run(checker, lines)
    assert len(res) == len(lines)
    lean = 0
    for line, got in zip(lines, res):
        if got["error"]:
            continue                                      # a bank the planner refuses is not the lowering's business
        assert got["lower"] == "", line
        assert got["bad"] == [], line
        lean += got["mx_passes"]
    assert lean > 0
