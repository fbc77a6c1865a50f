"""The cut of the AM bank's synchronous-AM chain (sdrangel_amd/csrc/am_sync_scan.hpp: m_pllFilt's pairing order over the compacted
sequence, the loop step the device walk shares with the ChannelAnalyzer bank, the AGC terms as a rounded prefix sum, the delay
selection, and every carry across feeds that end anywhere) on the host, against what the reference recorded per open sample
(tests/golden/am_sync_golden.npz, the `trace` case): tests/am_sync_check.cpp.  Built with plain g++, and once more with the address
and undefined-behaviour sanitizers; the stand-alone program alone runs under them."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

from tests import am_sync_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sdrangel_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "am_sync_check.cpp")
GOLD = os.path.join(ROOT, "tests", "golden", "am_sync_golden.npz")
CASE = sc.BY["trace_usb_m170"]


def _build(name, extra):
    exe = os.path.join(tempfile.mkdtemp(), name)
    # plain g++, no ROCm include path: the header compiles for the host on its own
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-I" + CSRC] + extra + [SRC, "-o", exe])
    return exe


@pytest.fixture(scope="module")
def check():
    return _build("am_sync_check", ["-O2"])


@pytest.fixture(scope="module")
def trace():
    g = np.load(GOLD)
    d = tempfile.mkdtemp()
    tr, sb = os.path.join(d, "trace.bin"), os.path.join(d, "trace.bin.sb")
    g[CASE["name"] + "/trace"].astype(np.float32).tofile(tr)
    g[CASE["name"] + "/trace_sb"].astype(np.float32).tofile(sb)
    return tr, sb, g


def _chain(exe, trace, seed):
    rate, sync = CASE["cfg"][2], 1 + CASE["sync"][1]
    return subprocess.run([exe, "chain", str(rate), str(sync), str(seed), trace[0], trace[1]], capture_output=True, text=True, timeout=300)


@pytest.mark.parametrize("seed", [1, 2, 20261020])
def test_cut_equals_the_recording_across_random_feeds(check, trace, seed):
    out = _chain(check, trace, seed)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout + out.stderr
    samples, blocks, feeds = (int(v) for v in out.stdout.split()[1:4])
    g = trace[2]
    assert samples == int(g[CASE["name"] + "/opens"][-1]) > 2000 and blocks == samples // sc.block(CASE["sync"][1]) >= 4 and feeds > 4, out.stdout


def test_the_step_reproduces_the_recorded_oscillator_and_takes_a_saturation_branch(check, trace):
    out = subprocess.run([check, "probe", str(CASE["cfg"][2]), trace[0]], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.startswith("probe "), out.stdout + out.stderr
    n, sat_hi, sat_lo, up, down, bad, locked, freq = (int(v) for v in out.stdout.split()[1:])
    g = trace[2]
    assert bad == 0 and [sat_hi, sat_lo, up, down] == list(g[CASE["name"] + "/probe"]), out.stdout
    assert sat_hi + sat_lo > 0
    assert [locked, freq] == list(g[CASE["name"] + "/state"][-1, 3:5])


def test_the_recorded_cases_cover_what_they_are_for():
    """what the maker asserted when it recorded, read back from the fixture: a locked and an unlocked end, a saturation branch,
    inputs that are the generator's"""
    g = np.load(GOLD)
    ends = [bool(g[c["name"] + "/state"][-1, 3]) for c in sc.CASES]
    assert any(ends) and not all(ends)
    assert any(int(g[c["name"] + "/probe"][0]) > 0 for c in sc.CASES) and any(int(g[c["name"] + "/probe"][1]) > 0 for c in sc.CASES)
    for c in sc.CASES:
        assert str(g[c["name"] + "/in_sha256"]) == sc.sha(sc.inputs(c)), c["name"]


def test_cut_is_clean_under_the_host_sanitizers(trace):
    exe = _build("am_sync_check_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    out = _chain(exe, trace, 3)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout + out.stderr
