"""CPU: tests/golden/lora_golden.npz against the generator of tests/lora_cases.py (the input hashes) and what the maker asserted when
it recorded, read back from the fixture: a lock and a line where a case claims them, the dump clipped at 140 symbols, m_time past
1023, a squelch closure that leaves m_time at or below 70, both signs of the finetune sum across the set, feeds that end on 63 ..
65 and 127 .. 129 outputs of the stream, every bandwidth of LoRaDemodSettings, and a bandwidth whose cutoff does not survive a
float."""
import os

import numpy as np
import pytest

from tests import lora_cases as lc

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lora_golden.npz")
TUNED_UP, TUNED_PLAIN, SHORT_CLOSES, LOCKS, WRAPS = range(5)


@pytest.fixture(scope="module")
def gold():
    g = np.load(GOLD)
    return {k: g[k] for k in g.files}


def lines_of(gold, name):
    return bytes(gold[name + "/text"]).decode("latin-1").split("\n")[:-1]


@pytest.mark.parametrize("case", lc.CASES, ids=[c["name"] for c in lc.CASES])
def test_inputs_are_the_generators(gold, case):
    assert str(gold[case["name"] + "/in_sha256"]) == lc.sha(lc.inputs(case))
    assert gold[case["name"] + "/counts"].size == len(case["splits"]) == gold[case["name"] + "/state"].shape[0]
    assert int(gold[case["name"] + "/counts"].sum()) == gold[case["name"] + "/samples"].reshape(-1, 2).shape[0] == int(gold[case["name"] + "/state"][-1, 4])
    assert case["n"] < 80000


@pytest.mark.parametrize("case", lc.CASES, ids=[c["name"] for c in lc.CASES])
def test_case_has_what_it_is_for(gold, case):
    name, ex = case["name"], case["expect"]
    ev, lines = gold[name + "/events"], lines_of(gold, name)
    assert len(lines) == int(gold[name + "/state"][-1, 5])
    if "locks" in ex:
        assert int(ev[LOCKS]) >= ex["locks"]
    if "lines" in ex:
        assert len(lines) == ex["lines"]
    if ex.get("clip"):
        assert len(lines[0]) == 140 // 2 - 1
    if ex.get("wrap"):
        assert int(ev[WRAPS]) >= 1
    if ex.get("short_close"):
        assert int(ev[SHORT_CLOSES]) >= 1
    if ex.get("silence"):
        assert int(ev[LOCKS]) >= 1 and int(gold[name + "/state"][-1, 0]) == 0
    if ex.get("edges"):
        counts = gold[name + "/counts"]
        assert {63, 64, 65, 127, 128, 129} <= set(np.cumsum(counts).tolist()) and 0 in counts and 1 in counts
    if ex.get("trace"):
        assert gold[name + "/trace"].shape == (int(gold[name + "/state"][-1, 4]) // 64, 261)


def test_the_set_covers_both_finetune_signs_every_bandwidth_and_the_noise_case(gold):
    ev = np.array([gold[c["name"] + "/events"] for c in lc.CASES])
    assert ev[:, TUNED_UP].sum() >= 1 and ev[:, TUNED_PLAIN].sum() >= 1 and ev[:, SHORT_CLOSES].sum() >= 1
    assert {c["cfg"][2] for c in lc.CASES} >= set(lc.BANDWIDTHS)
    assert int(gold["noise/events"][LOCKS]) == 0 and lines_of(gold, "noise") == []
    steps = {c["cfg"][0] / c["cfg"][2] for c in lc.CASES}
    assert 1.0 in steps and 2.0 in steps and any(s != int(s) for s in steps) and any(c["cfg"][1] for c in lc.CASES)


def test_7813s_cutoff_does_not_survive_a_float():
    exact = float(np.float32(7813)) / 1.9
    assert float(np.float32(exact)) != exact
