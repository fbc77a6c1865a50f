"""Banks for the array histories of the lean bank kernel (tree_mx_kernel.hpp: the wave that runs an array's tail job copies its
history, there is no walk), shared by tests/test_chan_tails.py (host: what the lowering marks) and tests/test_bank_tails_gpu.py.

All under the default planner options, so every pass runs the lean kernel.  BANKS: name -> (in_rate, [(rate, centre)]).  NEEDS says
what tests/chan_tail_check.cpp must find in each (tests/test_chan_tails.py holds it to that):
  counts   tail jobs that copy 4, 6, 8, 10, 12 arrays: 4 = one four-arm child, 6 = one six-arm child (a parent with a centre and
           lower/upper children wants the plain and the alternating odd arm), 8 / 10 / 12 = a lower/upper pair
  classes  tail jobs per epilogue class (branch-free pair, arms, sink)
  roots    passes whose root has plain, alternating, both odd kinds"""
import json
import os

from tests import bank_path_cases as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "chan_plan_tables.json")) as _f:
    _GOLDEN = {(c["name"], c["engine"]): c for c in json.load(_f)["cases"]}


def _path_case(name):
    c = next(c for c in B.CASES if c["name"] == name)
    return c["in_rate"], [tuple(ch) for ch in c["channels"]]


def _golden(name):
    c = _GOLDEN[(name, "mfma")]
    return c["in_rate"], [(r, f) for _, r, f in c["channels"]]


BANKS = {
    "two": (61_440_000, [(15_360_000, 15_501_352), (3_840_000, -20_000_000)]),
    "cfg3_32": _golden("cfg3_32"),                  # the benchmark's 32 channels
    "cover7": _path_case("cover7"),
    "cover1": _path_case("cover1"),
    "deep17_61M": _path_case("deep17_61M"),
}

# at least one tail job of each listed kind: counts -> numbers of arrays, classes -> epilogue classes, roots -> "EO" / "EA" / "EOA"
NEEDS = {
    "two": dict(counts=[4], classes=[1, 2], roots=["EA"]),
    "cfg3_32": dict(counts=[4, 8], classes=[0, 1], roots=["EO", "EA"]),
    "cover7": dict(counts=[4, 6, 8, 10], classes=[0, 1, 2], roots=["EO", "EA"]),
    "cover1": dict(counts=[4, 6, 8, 10], classes=[0, 1, 2], roots=["EO", "EA", "EOA"]),
    "deep17_61M": dict(counts=[4, 8, 10], classes=[0, 1, 2], roots=["EO", "EA", "EOA"]),
}


def line(in_rate, channels, engine="mfma", options="default"):
    return B.lister_line(engine, options, in_rate, channels)
