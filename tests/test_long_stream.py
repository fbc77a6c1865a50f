"""The premise of tests/test_long_stream_gpu.py, proved with the oracle alone (which tests/test_oracle_vs_ref.py pins to the compiled
reference): on the stream P | B | B | B | ... of tests/long_stream_cases.py every chain gives the same output in repetition 3 as in
repetition 2, feed by feed.  If that fails for a case, the case is wrong (its N), not the comparison."""
import numpy as np
import pytest

from tests import long_stream_cases as L
from tests import oracle_py as orc


def assert_periodic(case, order=48):
    assert L.n_ok(case["n"], case["depth"], order), (case["name"], case["n"], case["depth"])
    cuts = case["cuts"]
    assert cuts[0] == 0 and cuts[-1] == case["n"] and case["n"] - case["p"].size // 2 in cuts
    for c, (W, d) in enumerate(zip(case["W"], case["depths"])):
        w1, w2, w3 = W[1:]
        assert len(w2) == len(w3) == len(cuts) - 1
        for k, (a, b) in enumerate(zip(w2, w3)):
            assert a.size == b.size and np.array_equal(a, b), (case["name"], c, d, k)
        per_rep = sum(a.size for a in w2) // 2
        assert per_rep == case["n"] >> d and per_rep >= 46, (case["name"], c, d, per_rep)
        # the prefix is felt: repetition 1 starts from its tail, not from the tail of B (else W1 would prove nothing about W2)
        assert d == 0 or not np.array_equal(np.concatenate(w1), np.concatenate(w2)), (case["name"], c, d)


@pytest.mark.parametrize("name", list(L.BANKS16))
def test_bank16_outputs_repeat(name):
    case = L.bank16(name)
    assert case["depth"] == max(len(orc.chan_plan(case["case"]["in_rate"], r, f)[0]) for r, f in case["case"]["channels"]) <= 12
    assert_periodic(case)


def test_bank24_outputs_repeat():
    case = L.bank24()
    assert tuple(case["depths"]) == L.STAGES24
    assert_periodic(case)


@pytest.mark.parametrize("log2,fcpos,bits", L.DECIM24)
def test_decim24_outputs_repeat(log2, fcpos, bits):
    case = L.decim24(log2, fcpos, bits)
    assert all(c % case["group"] == 0 for c in case["cuts"])
    assert_periodic(case, order=64)
