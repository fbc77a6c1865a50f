"""What the cases of tests/trip_edge_cases.py must reach, asserted on the CPU oracles alone (tests/<family>_oracle.c): the squelch
and the AGC move often enough inside feeds cut at the edges of a lane's four samples, a wave and a trip that the GPU comparison of
tests/test_demod_trip_edges_gpu.py cannot pass on a silent channel."""
import pytest

from tests import am_cases, nfm_cases, ssb_cases, udpsrc_cases, wfm_cases
from tests import trip_edge_cases as tc

CM = {"am": am_cases, "nfm": nfm_cases, "ssb": ssb_cases, "udpsrc": udpsrc_cases, "wfm": wfm_cases}
PAIRS = [(family, case["name"]) for family, cases in tc.CASES.items() for case in cases]


def test_lengths_sit_on_the_edges():
    assert {3, 4, 5} <= set(tc.LENGTHS) and {255, 256, 257} <= set(tc.LENGTHS) and {1023, 1024, 1025} <= set(tc.LENGTHS)
    assert max(tc.LENGTHS) > 4 * 1024 and 1 in tc.LENGTHS
    assert {511, 512, 513} <= set(tc.WFM_LENGTHS)
    assert set(tc.CASES) == set(CM)
    for cases in tc.CASES.values():
        for c in cases:
            assert c["splits"] == (tc.WFM_LENGTHS if c["name"] == "burst_48k" else tc.LENGTHS)


@pytest.mark.parametrize("family,name", PAIRS)
def test_oracle_reaches_the_transitions(family, name):
    case = {c["name"]: c for c in tc.CASES[family]}[name]
    want = tc.run_oracle(family, CM[family].build_oracle(), case)
    tc.check_reach(family, case, want)
