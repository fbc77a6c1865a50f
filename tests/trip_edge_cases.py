"""Cases for the workgroup scans of the demodulator tails (sdrangel_amd/csrc/demod_wg.hpp): feed lengths on either side of a
lane's four samples, a wave's 256 and a trip's 1024, with the squelch and the AGC moving inside them.

The input rate equals the output rate and is low (8000), so a feed of n inputs is a tail feed of n samples and the counters'
opening counts are tens to hundreds of samples.  SSB's front hands over whole blocks of 512 and WFM's tail works in blocks of
512 = WFM_H, so those two take the configurations their own case lists have for that (short_history, burst_48k).

tests/test_demod_trip_edges.py asserts on the oracles alone what these cases must reach; tests/test_demod_trip_edges_gpu.py
compares the GPU with the oracles, feed by feed."""
from __future__ import annotations

import numpy as np

from tests import am_cases, nfm_cases, ssb_cases, udpsrc_cases, wfm_cases

#: a lane's four samples partly present; the wave edge at 256 samples; the trip edge at 1024; several trips
LENGTHS = [1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2049, 4097, 3000]
#: amplitude runs, strong and weak in turn
RUNS = [700, 500, 1500, 300, 900, 1200]
#: WFM: feeds around WFM_H = 512, as wfm_cases._EDGES has them, then whole trips
WFM_LENGTHS = [1, 511, 512, 513, 2, 3, 5, 509, 521, 1021, 1031, 4099, 3000]
RATE = 8000


def _case(name, cfg, sig, splits, seed, **more):
    return dict({"name": name, "cfg": cfg, "sig": sig, "n": sum(splits), "seed": seed, "splits": list(splits)}, **more)


def make_cases() -> dict:
    """family -> its cases; every case has the keys of tests/<family>_cases.CASES"""
    runs = lambda weak: dict(runs=RUNS, amps=[8000.0, weak])
    ssb = {c["name"]: c for c in ssb_cases.CASES}["short_history"]
    wfm = {c["name"]: c for c in wfm_cases.CASES}["burst_48k"]
    return {
        "am": [_case("am", am_cases._cfg(RATE, RATE, nco_freq=-1000), dict({"kind": "am", "f0": 1000.0, "depth": 0.5, "fa": 400.0}, **runs(30.0)), LENGTHS, 71)],
        "nfm": [_case("nfm_gate1", nfm_cases._cfg(RATE, RATE, nco_freq=-1000, gate=1),
                      dict({"kind": "nfm", "f0": 1000.0, "dev": 1500.0, "fa": 400.0}, **runs(30.0)), LENGTHS, 72)],
        "udpsrc": [
            _case("ambpf_agc", udpsrc_cases._cfg(RATE, RATE, fmt=udpsrc_cases.AM_BPF_MONO, sqdb=-30, gate=1, agc=1),
                  dict({"kind": "am", "f0": 0.0, "fa": 400.0}, **runs(20.0)), LENGTHS, 73, agc=True),
            _case("nfm", udpsrc_cases._cfg(RATE, RATE, fmt=udpsrc_cases.NFM, gate=1, nco_freq=-1000),
                  dict({"kind": "nfm", "f0": 1000.0, "dev": 1500.0, "fa": 400.0}, **runs(3.0)), LENGTHS, 74, agc=False),
        ],
        # the front hands over n rounded down to whole blocks of 512: the per-feed audio lengths are multiples of 512
        "ssb": [_case("short_history", ssb["cfg"], ssb["sig"], LENGTHS, 75, reach=ssb["reach"])],
        "wfm": [_case("burst_48k", wfm["cfg"], wfm["sig"], WFM_LENGTHS, 76)],
    }


CASES = make_cases()


def run_oracle(family: str, L, case: dict) -> dict:
    """<family>_cases.run_oracle over the case's feeds"""
    return {"am": am_cases, "nfm": nfm_cases, "ssb": ssb_cases, "udpsrc": udpsrc_cases, "wfm": wfm_cases}[family].run_oracle(L, case)


def check_reach(family: str, case: dict, want: dict):
    """what the oracle must show, so that no comparison passes on a silent channel"""
    if family in ("am", "nfm", "udpsrc"):
        assert [f.shape[0] for f in want["feeds"]] == case["splits"]        # in rate = out rate: a tail feed of n samples
        assert want["probe"]["transitions"] >= 8, want["probe"]
        if case.get("agc"):
            assert want["probe"]["agc_mode_changes"] >= 8, want["probe"]
    elif family == "ssb":
        p = want["probe"]
        assert p["gate_full"] >= 1 and p["up_to_down"] >= 1 and p["down_to_up"] >= 1, p
        sizes = {a.shape[0] for a in want["audio"]}
        assert 0 in sizes and len(sizes - {0}) >= 3 and all(s % 512 == 0 for s in sizes), sizes
    else:
        # WFM's oracle has no probe.  A closed squelch gives the resampler zeros, so its audio is exactly 0 from a few taps
        # behind a closure to the next opening: a stretch of more than 64 zeros between two non-zero samples is a closure
        # followed by an opening
        at = np.flatnonzero(np.concatenate(want["feeds"]))
        assert at.size and int((np.diff(at) > 64).sum()) >= 2, at.size
