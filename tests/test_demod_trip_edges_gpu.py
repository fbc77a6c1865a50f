"""GPU: every demodulator family fed lengths on either side of a lane's four samples, a wave's 256 and a scan trip's 1024
(tests/trip_edge_cases.py), with the squelch and the AGC moving inside the feeds: the workgroup scans, prefix counts and level
sums of sdrangel_amd/csrc/demod_wg.hpp where a lane's samples are partly present, where a wave or a trip ends with the feed
and where a feed takes several trips.  One single-channel handle per case; every feed's output and the final state against the
family's oracle, by the comparison rules of tests/test_<family>_gpu.py."""
import pytest

from tests import trip_edge_cases as tc
from tests.demod_families import FAMILIES, naming

pytestmark = pytest.mark.gpu

PAIRS = [(family, case["name"]) for family, cases in tc.CASES.items() for case in cases]


@pytest.mark.parametrize("family,name", PAIRS)
def test_feeds_at_the_scan_edges(family, name):
    fam = FAMILIES[family]
    case = {c["name"]: c for c in tc.CASES[family]}[name]
    want = tc.run_oracle(family, fam.cm.build_oracle(), case)
    tc.check_reach(family, case, want)
    bank = fam.Bank([fam.gcfg(case["cfg"])])
    try:
        got = []
        for x in fam.cm.cut(fam.cm.inputs(case), case["splits"]):
            bank.feed([x])
            got.append(fam.read(bank, 0))
        with naming(case, 0, f"{family} {name}"):
            fam.check_feeds(case, got, want, f"{family} {name}")
            fam.check_state(bank, 0, want, f"{family} {name}")
    finally:
        bank.close()
