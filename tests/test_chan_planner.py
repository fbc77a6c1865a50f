"""The channelizer bank's planner on its own, without a GPU: every table tree_kernel reads, byte for byte, for fixed banks under
both engines (tests/golden/chan_plan_tables.json).  The cases: cfg 3's 32 channels, bench's chan128 and cfg4 banks (the 64 KB
budget), the two deep-pass option sets of test_chan_gpu.py, a single-channel group (what reconfigure / add_channel make), and
seeded mixed-rate banks at 2.4 MS/s with channels that end at inner nodes and lower-only / upper-only pairs."""
import hashlib
import json
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sdrangel_amd", "csrc")
with open(os.path.join(ROOT, "tests", "golden", "chan_plan_tables.json")) as _f:
    CASES = json.load(_f)["cases"]


@pytest.fixture(scope="module")
def planner():
    exe = os.path.join(tempfile.mkdtemp(), "chan_plan_check")
    # plain g++, no ROCm include path: the planner and its table layouts are host-only code; flags as in csrc/Makefile
    subprocess.check_call(["g++", "-O3", "-std=c++17", "-ffp-contract=off", "-Wall", "-I" + CSRC,
                           os.path.join(ROOT, "tests", "chan_plan_check.cpp"), os.path.join(CSRC, "chan_plan.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("case", CASES, ids=[f"{c['name']}-{c['engine']}" for c in CASES])
def test_plan_tables_match_golden(planner, case):
    line = f"{case['engine']} {case['lds_kb']} {case['max_levels']} {case['in_rate']} {len(case['channels'])} "
    line += " ".join(f"{i} {r} {f}" for i, r, f in case["channels"])
    # the planner takes its options as arguments only: switches in the environment must change nothing
    env = dict(os.environ, SDRX_CHAN_ENGINE="valu" if case["engine"] == "mfma" else "mfma", SDRX_CHAN_LDS_KB="16", SDRX_CHAN_MAX_LEVELS="2")
    out = subprocess.run([planner], input=line + "\n", capture_output=True, text=True, timeout=120, env=env, check=True)
    got = json.loads(out.stdout)
    assert got["error"] == ""
    assert got["streams"] == case["streams"]
    assert got["passes"] == case["passes"]
    assert got["sinks"] == case["sinks"]
    for table, want in case["sha256"].items():
        assert hashlib.sha256(bytes.fromhex(got[table])).hexdigest() == want, table
