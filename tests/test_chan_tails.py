"""The array histories of the lean bank kernel as the lowering sets them up (sdrangel_amd/csrc/chan_lower.cpp: MX_TAIL_BIT),
without a GPU.

tree_mx_kernel.hpp has no history walk: the wave that runs the tail job of an array copies slot -> head and tail -> slot itself.
tests/chan_tail_check.cpp plans a bank, lowers it and restates the kernel's address arithmetic: every array of every lean pass has
exactly one tail job, that job's own stores are the array's last 16 dwords, the slot derived from the job's words is the array's
own (store_base + 16 * array index), and no job of the level touches a head, a slot or another job's tail.  The cases: the golden
banks, 3000 seeded random banks (the option sets of tests/bank_path_cases.py), and the banks of tests/bank_tail_cases.py, which
must also hold the kinds of tail job the GPU test is there for."""
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

from tests import bank_tail_cases as T
from tests.bank_path_cases import OPTIONS, random_bank

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sdrangel_amd", "csrc")
with open(os.path.join(ROOT, "tests", "golden", "chan_plan_tables.json")) as _f:
    GOLDEN = json.load(_f)["cases"]


@pytest.fixture(scope="module")
def checker():
    exe = os.path.join(tempfile.mkdtemp(), "chan_tail_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-I" + CSRC,
                           os.path.join(ROOT, "tests", "chan_tail_check.cpp"), os.path.join(CSRC, "chan_plan.cpp"),
                           os.path.join(CSRC, "chan_lower.cpp"), "-o", exe])
    return exe


def _run(exe, lines):
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=600, check=True)
    res = [json.loads(l) for l in out.stdout.splitlines()]
    assert len(res) == len(lines)
    return res


def _line(engine, lds_kb, max_levels, in_rate, channels):
    return f"{engine} {lds_kb} {max_levels} {in_rate} {len(channels)} " + " ".join(f"{i} {r} {f}" for i, (r, f) in enumerate(channels))


@pytest.mark.parametrize("case", GOLDEN, ids=[f"{c['name']}-{c['engine']}" for c in GOLDEN])
def test_golden_banks_one_tail_job_per_array(checker, case):
    (got,) = _run(checker, [_line(case["engine"], case["lds_kb"], case["max_levels"], case["in_rate"], [(r, f) for _, r, f in case["channels"]])])
    assert got["error"] == "" and got["lower"] == ""
    assert got["bad"] == []
    if case["engine"] == "mfma" and case["max_levels"] == 0:
        assert got["mx_passes"] == got["passes"] > 0      # default plans: every pass is lean, none was refused for its histories
        assert got["tails"] > 0 and sum(got["counts"]) == got["tails"] == sum(got["classes"])
        # every array is covered once: the tail jobs' array counts add up to the arrays below the roots
        assert sum(n * c for n, c in zip((4, 6, 8, 10, 12), got["counts"])) == got["arrays"]


@pytest.mark.parametrize("opt", sorted(OPTIONS))
def test_random_banks_one_tail_job_per_array(checker, opt):
    rng = np.random.default_rng(20261018 + sorted(OPTIONS).index(opt))
    ml, kb = OPTIONS[opt] or (0, 0)
    lines = []
    for _ in range(1000):
        ir, ch = random_bank(rng)
        lines.append(_line("mfma", kb, ml, ir, ch))
    lean = 0
    for line, got in zip(lines, _run(checker, lines)):
        if got["error"]:
            continue                                      # a bank the planner refuses is not the lowering's business
        assert got["lower"] == "", line
        assert got["bad"] == [], line
        assert sum(n * c for n, c in zip((4, 6, 8, 10, 12), got["counts"])) == got["arrays"], line
        lean += got["mx_passes"]
    assert lean > 0


@pytest.mark.parametrize("name", sorted(T.BANKS))
def test_gpu_cases_hold_their_tail_jobs(checker, name):
    in_rate, channels = T.BANKS[name]
    (got,) = _run(checker, [T.line(in_rate, channels)])
    assert got["error"] == "" and got["lower"] == "" and got["bad"] == []
    assert got["mx_passes"] == got["passes"] > 0
    need = T.NEEDS[name]
    for n in need["counts"]:
        assert got["counts"][n // 2 - 2] > 0, (name, "tail jobs of", n, "arrays")
    for c in need["classes"]:
        assert got["classes"][c] > 0, (name, "tail jobs of class", c)
    for k in need["roots"]:
        assert got["roots"][("EO", "EA", "EOA").index(k)] > 0, (name, "root", k)
