"""The fetch step of the LoRa bank (sdrangel_amd/csrc/lora_scan.hpp: the first-strict-maximum picks and the mov sums in the
reference's order, finetune, the squelch, synch(), dumpRaw() and the four lorabits functions, and the closed form of m_angle) on the
host, against what the reference recorded per fetch (tests/golden/lora_golden.npz, the `trace` case): tests/lora_check.cpp.  Built
with plain g++, and once more with the address and undefined-behaviour sanitizers; the stand-alone program alone runs under them."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sdrangel_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "lora_check.cpp")
GOLD = os.path.join(ROOT, "tests", "golden", "lora_golden.npz")


def _build(name, extra):
    exe = os.path.join(tempfile.mkdtemp(), name)
    # plain g++, no ROCm include path: the header compiles for the host on its own
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-I" + CSRC] + extra + [SRC, "-o", exe])
    return exe


@pytest.fixture(scope="module")
def check():
    return _build("lora_check", ["-O2"])


@pytest.fixture(scope="module")
def trace():
    g = np.load(GOLD)
    d = tempfile.mkdtemp()
    tr, tx = os.path.join(d, "trace.bin"), os.path.join(d, "text.bin")
    g["trace/trace"].astype(np.float32).tofile(tr)
    g["trace/text"].astype(np.uint8).tofile(tx)
    return tr, tx, g


def _replay(exe, trace, seed):
    return subprocess.run([exe, "replay", str(seed), trace[0], trace[1]], capture_output=True, text=True, timeout=300)


@pytest.mark.parametrize("seed", [1, 2, 20261021])
def test_fetch_step_equals_the_recording_across_random_feeds(check, trace, seed):
    out = _replay(check, trace, seed)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout + out.stderr
    fetches, lines, feeds = (int(v) for v in out.stdout.split()[1:4])
    g = trace[2]
    assert fetches == g["trace/trace"].shape[0] == int(g["trace/state"][-1, 4]) // 64 > 100
    assert lines == int(g["trace/state"][-1, 5]) >= 1 and feeds > 3, out.stdout


def test_the_trace_has_a_lock_a_dump_and_closed_fetches():
    """what the replay goes through: a preamble lock (m_time back to 0 with the squelch open, m_tune set), the dump, fetches with
    the squelch closed"""
    t = np.load(GOLD)["trace/trace"]
    time, tune, after = t[:, 258], t[:, 259], t[:, 257]
    locks = [j for j in range(1, t.shape[0]) if after[j] >= 0 and time[j] == 0 and time[j - 1] > 12]
    assert locks and tune[locks[-1]] != 0
    assert any(after[j] < 0 and time[j - 1] > 70 for j in range(1, t.shape[0]))
    assert np.count_nonzero(after < 0) >= 3


def test_angle_closed_form(check):
    out = subprocess.run([check, "angle"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout + out.stderr
    # the running sums over three periods, and the three closed forms around 2^31, 2^32, 2^33 and 2^40
    assert [int(v) for v in out.stdout.split()[1:3]] == [3 * 512 + 7, 4 * 1024], out.stdout


def test_fetch_step_is_clean_under_the_host_sanitizers(trace):
    exe = _build("lora_check_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    for args in (["replay", "3", trace[0], trace[1]], ["angle"]):
        out = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout + out.stderr
