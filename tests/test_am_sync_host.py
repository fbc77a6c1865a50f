"""The cut of the AM bank's synchronous-AM chain (sdrangel_amd/csrc/am_sync_scan.hpp: m_pllFilt's pairing order over the compacted
sequence, the loop step the device walk shares with the ChannelAnalyzer bank, the AGC terms as a rounded prefix sum, the delay
selection, and every carry across feeds that end anywhere) on the host, against what the reference recorded per open sample
(tests/golden/am_sync_golden.npz, the `trace` case): tests/am_sync_check.cpp.  Built with plain g++, and once more with the address
and undefined-behaviour sanitizers; the stand-alone program alone runs under them.

Two more traces come from tests/am_oracle.c (amo_trace, the recorder's layout), which tests/test_am_sync_oracle.py ties to the
reference: USB at 1000 S/s, where the AGC history (250) is shorter than a block, and DSB at 48000 S/s, where it is 12000 -- the
two regimes tests/test_am_sync_random_gpu.py takes the device to."""
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


# ---------------------------------------------------------------- traces from the oracle
#: indices into am_sync_cases.random_cases(): the forced USB case at 1000 S/s (hn < B) and the forced DSB case at 48000 S/s
ORACLE_TRACES = {"usb_1000": 1, "dsb_48000": 6}


@pytest.fixture(scope="module")
def oracle_traces():
    L = sc.build_oracle()
    cases = sc.random_cases(max(ORACLE_TRACES.values()) + 1)
    out = {}
    for key, index in ORACLE_TRACES.items():
        case = cases[index]
        d = tempfile.mkdtemp()
        tr, sb = os.path.join(d, "trace.bin"), os.path.join(d, "trace.bin.sb")
        run = sc.run_oracle(L, case, trace=(tr, sb))
        out[key] = (case, run, tr, sb)
    return out


def _chain_of(exe, case, tr, sb, seed):
    return subprocess.run([exe, "chain", str(case["cfg"][2]), str(1 + case["sync"][1]), str(seed), tr, sb], capture_output=True, text=True, timeout=300)


def _assert_chain(out, case, run):
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout + out.stderr
    samples, blocks, feeds = (int(v) for v in out.stdout.split()[1:4])
    B = sc.block(case["sync"][1])
    assert samples == run["sync_probe"]["open"] and blocks == samples // B == run["sync_probe"]["blocks"] >= 9 and feeds > 9, out.stdout


@pytest.mark.parametrize("key", list(ORACLE_TRACES))
@pytest.mark.parametrize("seed", [1, 20261021])
def test_cut_equals_the_oracle_trace_across_random_feeds(check, oracle_traces, key, seed):
    case, run, tr, sb = oracle_traces[key]
    hn, B = sc.agc_len(case["cfg"][2]), sc.block(case["sync"][1])
    assert (hn < B) if key == "usb_1000" else (hn > 8 * B)
    assert run["sync_probe"]["reopenings"] >= 1 and run["sync_probe"]["wrapped"] > 0          # the chain stood still once; the history wrapped
    _assert_chain(_chain_of(check, case, tr, sb, seed), case, run)


@pytest.mark.parametrize("key", list(ORACLE_TRACES))
def test_the_step_reproduces_the_oracle_trace(check, oracle_traces, key):
    case, run, tr, _ = oracle_traces[key]
    out = subprocess.run([check, "probe", str(case["cfg"][2]), tr], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.startswith("probe "), out.stdout + out.stderr
    n, sat_hi, sat_lo, up, down, bad, locked, freq = (int(v) for v in out.stdout.split()[1:])
    sp = run["sync_probe"]
    assert bad == 0 and n == sp["open"] and [sat_hi, sat_lo, up, down] == [sp["sat_hi"], sp["sat_lo"], sp["lock_up"], sp["lock_down"]], out.stdout
    assert [locked, freq] == list(run["state"][-1, 3:5])


def test_cut_is_clean_under_the_host_sanitizers_on_the_oracle_traces(oracle_traces):
    exe = _build("am_sync_check_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    for key in ORACLE_TRACES:
        case, run, tr, sb = oracle_traces[key]
        _assert_chain(_chain_of(exe, case, tr, sb, 3), case, run)
