"""The lowered root records of the lean bank kernel (TkLRoot: sdrangel_amd/csrc/chan_lower.cpp, tree_mx_kernel.hpp), without a GPU.

tree_mx_kernel fills the root arms at one per-lane address plus immediate offsets and copies the root history into one window: it
reads a base and the set of odd-arm kinds from the record, no longer the six arm offsets, the window and the array count of
TkSubtree.  tests/chan_lower_root_check.cpp plans a bank, lowers it, restates the kernel's addresses from the record and compares
them with the planner's tables; then it moves each of those table entries in turn and expects the lowering to refuse the pass.  The
cases: every bank of tests/golden/chan_plan_tables.json and seeded random banks under the option sets of tests/bank_path_cases.py;
together they must have roots with plain odd arms only, alternating only, and both."""
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

from tests.bank_path_cases import OPTIONS, random_bank
from tests.bank_sink_edge_cases import BANKS, IN_RATE
from tests.test_chan_lower import GOLDEN, _line

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sdrangel_amd", "csrc")


@pytest.fixture(scope="module")
def checker():
    exe = os.path.join(tempfile.mkdtemp(), "chan_lower_root_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-I" + CSRC,
                           os.path.join(ROOT, "tests", "chan_lower_root_check.cpp"), os.path.join(CSRC, "chan_plan.cpp"),
                           os.path.join(CSRC, "chan_lower.cpp"), "-o", exe])
    return exe


def _run(exe, lines):
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=600, check=True)
    res = [json.loads(l) for l in out.stdout.splitlines()]
    assert len(res) == len(lines)
    return res


def _check(lines, res):
    kinds = np.zeros(4, dtype=int)
    for line, got in zip(lines, res):
        if got["error"]:
            continue                                      # a bank the planner refuses is not the lowering's business
        assert got["lower"] == "", line
        assert got["bad"] == [], line
        assert got["refused"] == got["tampered"], line
        kinds += got["kinds"]
    return kinds


def test_golden_banks_root_records(checker):
    lines = [_line(c["engine"], c["lds_kb"], c["max_levels"], c["in_rate"], [(r, f) for _, r, f in c["channels"]]) for c in GOLDEN]
    res = _run(checker, lines)
    kinds = _check(lines, res)
    assert kinds[1:].sum() > 0
    for c, got in zip(GOLDEN, res):
        if c["engine"] == "valu":
            assert sum(got["kinds"]) == 0 and got["tampered"] == 0          # the VALU engine never runs the lean kernel
        elif c["max_levels"] == 0:
            assert sum(got["kinds"]) > 0 and got["tampered"] > 0            # default plans: every subtree has a record


@pytest.mark.parametrize("name", sorted(BANKS))
def test_sink_edge_banks_run_the_lean_kernel(checker, name):
    """the banks of tests/test_bank_sink_edges_gpu.py: every pass on the lean kernel (last_launch() cannot tell it from the general
    one), and the first pass's root has the arms the bank is named for"""
    channels, kinds = BANKS[name]
    line = _line("mfma", 0, 0, IN_RATE, channels)
    (got,) = _run(checker, [line])
    assert got["error"] == "" and got["lower"] == "" and got["bad"] == []
    assert got["mx_passes"] == got["passes"] >= 3                 # a deep channel: three passes, a sink at every pass depth
    assert got["first"] == ("O" in kinds) * 1 + ("A" in kinds) * 2
    assert got["refused"] == got["tampered"] > 0


@pytest.mark.parametrize("opt", sorted(OPTIONS))
def test_random_banks_root_records(checker, opt):
    rng = np.random.default_rng(20261017 + sorted(OPTIONS).index(opt))
    ml, kb = OPTIONS[opt] or (0, 0)
    lines = []
    for _ in range(300):
        ir, ch = random_bank(rng)
        lines.append(_line("mfma", kb, ml, ir, ch))
    kinds = _check(lines, _run(checker, lines))
    # a root is an inner node: it has children, so at least one odd-arm kind; under the default options, where every pass is lean,
    # all three sets occur (the deep option sets leave few lean passes)
    assert kinds[0] == 0 and kinds[1:].sum() > 0, kinds
    if OPTIONS[opt] is None:
        assert (kinds[1:] > 0).all(), kinds
