"""CPU: sdrangel_amd/csrc/bfm_rds.hpp, the header the device's RDS walk runs, built for the host (tests/bfm_rds_check.cpp) and
driven with what the reference's own RDSDemod and RDSDecoder were given (tests/golden/bfm_rds_golden.npz):
  - frameSync on the synthetic bit streams: every step's group_ready, group and synced() equal the reference's;
  - RDSDemod::process + frameSync on the recorded resampler output of one case: subcarr_bb of every sample, bits, report and
    the whole state equal the recording bit for bit;
  - frameSync on the long case's recorded bits: the groups of the reference's own run through NO_SYNC, presync and sync;
  - the probe: every branch of the clock recovery, of biphase and of frameSync is taken over these inputs.
Also the random draw of bfm_rds_cases.random_cases() as tests/golden/bfm_rds_random_golden.npz recorded it (tests/test_bfm_rds_random_gpu.py
runs it on the GPU): the generator still gives the recorded inputs, the draw keeps its shares, at most two draws were set aside."""
import os
import subprocess

import numpy as np
import pytest

from tests import bfm_cases as bc
from tests import bfm_rds_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_STATE = [f for f in rc.STATE_FIELDS if f not in ("distance_remain", "mix_phase", "n_rds")]
PROBES = {}


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("bfm_rds") / "bfm_rds_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-I" + os.path.join(ROOT, "sdrangel_amd", "csrc"),
                           os.path.join(ROOT, "tests", "bfm_rds_check.cpp"), "-o", out])
    return out


@pytest.fixture(scope="module")
def gold():
    return rc.golden()


def _run(exe, mode, data: np.ndarray, tmp_path, tag):
    fin, fout = str(tmp_path / f"{tag}.in"), str(tmp_path / f"{tag}.out")
    with open(fin, "wb") as f:
        f.write(np.ascontiguousarray(data).tobytes())
    txt = subprocess.check_output([exe, mode, fin, fout], text=True)
    PROBES[tag] = {k: int(v) for k, v in (p.split("=") for p in txt.split())}
    return open(fout, "rb").read()


def _framesync(exe, bits, tmp_path, tag):
    raw = np.frombuffer(_run(exe, "framesync", np.asarray(bits, np.uint8), tmp_path, tag), np.uint8).reshape(-1, 10)
    out = np.empty((raw.shape[0], 6), np.uint16)
    out[:, 0], out[:, 1] = raw[:, 0], raw[:, 1]
    out[:, 2:] = raw[:, 2:].copy().view(np.uint16)
    return out


@pytest.mark.parametrize("name", sorted(rc.framesync_streams()))
def test_framesync_equals_the_reference_step_by_step(exe, gold, tmp_path, name):
    bits = rc.framesync_streams()[name]
    want = gold[f"fs/{name}/out"]
    got = _framesync(exe, bits, tmp_path, "fs_" + name)
    assert got.shape == want.shape == (bits.size, 6)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, (name, "first differing step", int(bad[0]), got[bad[0]], want[bad[0]])


def test_framesync_fixtures_hold_what_they_are_for(gold):
    o = {n: gold[f"fs/{n}/out"] for n in rc.framesync_streams()}
    assert int(o["valid"][:, 0].sum()) == 9 and int(o["cprime"][:, 0].sum()) == 4
    assert (o["bad_35_of_50"][:, 1] == 1).all() and (o["bad_36_of_50"][:, 1] == 0).any()        # the threshold, from both sides
    for n in ("lose_and_resync", "presync_dropped", "bad_36_of_50"):
        un = np.flatnonzero(o[n][:, 1] == 0)
        assert un.size and o[n][-1, 1] == 1 and o[n][un[-1]:, 0].sum() >= 3, n                  # out of sync, back, groups behind that
    assert o["random"][:, 0].sum() == 0


def test_demod_and_decoder_equal_the_recording_on_its_resampler_output(exe, gold, tmp_path):
    case = {c["name"]: c for c in rc.CASES}[rc.CR_CASE]
    want = rc.golden_case(gold, case)
    cr = gold[f"{rc.CR_CASE}/cr"]
    n = sum(want["n_rds"])
    assert cr.size == n
    raw = _run(exe, "demod", cr, tmp_path, "demod")
    pos = 0

    def take(dtype, k):
        nonlocal pos
        a = np.frombuffer(raw, dtype, k, pos).copy()
        pos += a.nbytes
        return a

    assert int(take(np.int64, 1)[0]) == n
    bb = take(np.float32, n)
    bits = take(np.uint8, int(take(np.int64, 1)[0]))
    groups = take(np.uint16, 4 * int(take(np.int64, 1)[0])).reshape(-1, 4)
    report, state = take(np.uint32, 5), take(np.uint64, len(HOST_STATE))
    assert pos == len(raw)
    assert np.array_equal(bits, np.concatenate(want["bits"])) and np.array_equal(groups, np.concatenate(want["groups"]))
    ends = np.cumsum(want["n_rds"])
    for i, (a, b) in enumerate(zip(np.split(bb, ends[:-1]), want["n_rds"])):
        assert rc.sha_f32(a) == want["bb_sha"][i], ("subcarr_bb of feed", i)
    for k in range(4):
        assert rc.same_float_bits(int(report[k]), int(want["report"][-1][k])), ("report", k)
    assert report[4] == want["report"][-1][4]
    cols = [rc.STATE_FIELDS.index(f) for f in HOST_STATE]
    diff = [f for f, g, w in zip(HOST_STATE, state, want["state"][-1][cols]) if g != w]
    assert not diff, diff
    # the case is there for the frame flip: the reference ended it on the other reading frame
    assert int(want["state"][-1][rc.STATE_FIELDS.index("reading_frame")]) == 1


def test_framesync_on_the_long_cases_bits_gives_the_reference_groups(exe, gold, tmp_path):
    case = {c["name"]: c for c in rc.CASES}["long_288k"]
    want = rc.golden_case(gold, case)
    sync = [int(s[rc.STATE_FIELDS.index("sync")]) for s in want["state"]]
    assert 0 in sync and sync[-1] == 1, "the reference's own decoder left SYNC and came back"
    first_unsynced = sync.index(0)
    assert sum(g.shape[0] for g in want["groups"][first_unsynced + 1:]) >= 3, "and completed at least three groups behind that"
    out = _framesync(exe, np.concatenate(want["bits"]), tmp_path, "fs_long")
    assert np.array_equal(out[out[:, 0] == 1][:, 2:], np.concatenate(want["groups"]))
    ends = np.cumsum([b.size for b in want["bits"]])
    assert [int(out[e - 1, 1]) for e in ends] == sync


def test_every_branch_was_taken(exe, gold, tmp_path):
    """runs every input of this module itself: the counts do not depend on which other tests ran"""
    PROBES.clear()
    for name, bits in rc.framesync_streams().items():
        _framesync(exe, bits, tmp_path, "fs_" + name)
    _framesync(exe, gold["long_288k/bits"], tmp_path, "fs_long")
    _run(exe, "demod", gold[f"{rc.CR_CASE}/cr"], tmp_path, "demod")
    assert len(PROBES) == len(rc.framesync_streams()) + 2
    total = {}
    for p in PROBES.values():
        for k, v in p.items():
            total[k] = total.get(k, 0) + v
    print(total)
    never = [k for k, v in total.items() if v == 0]
    assert not never and len(total) == 24, never


# ---------------------------------------------------------------- the random draw
@pytest.fixture(scope="module")
def rgold():
    return rc.load_random_golden()


def test_the_random_recording_has_every_case_and_its_inputs(rgold):
    cases = rc.random_cases()
    assert [k for k in rgold if k not in ("host", "unsure_skipped")] == [c["name"] for c in cases]
    assert rgold["host"].startswith("glibc 2.") and rgold["host"].endswith("fma=1")
    assert os.path.getsize(rc.RANDOM_GOLDEN) < 547302
    for c in cases:
        want = rgold[c["name"]]
        assert bc.sha(rc.inputs(c)) == want["in_sha"], c
        assert len(want["n_rds"]) == len(c["splits"]) == len(want["bits"]) == len(want["groups"]) == len(want["state"]), c
        assert int(want["state"][-1][rc.STATE_FIELDS.index("numsamples")]) == sum(want["n_rds"]), c


def test_the_random_draw_keeps_its_shares(rgold):
    cases = rc.random_cases()
    s = rc.assert_random_shares(cases, rgold)
    print(s)
    assert all(c["rds"] == 1 and c["cfg"]["audio_rate"] in (48000, 44100) for c in cases) and {c["cfg"]["audio_rate"] for c in cases} == {48000, 44100}
    assert all(c["cfg"]["rf"] >= min(180000.0, np.float32(0.9 * c["cfg"]["in_rate"])) for c in cases if "runs" not in c["sig"])
    assert all(300 <= c["sig"]["rds"] <= 5000 and 0 <= c["sig"]["rds_phi"] < 2 * np.pi and 0 <= c["sig"]["lead"] <= 4000 for c in cases if c["sig"]["kind"] == "mpx")
    # every input emits on the clamped schedule, fewer above it
    for c in cases:
        n_rds, blocks = sum(rgold[c["name"]]["n_rds"]), c["n"] // 512 * 512
        assert n_rds == blocks if rc.rds_step(c) <= 1 else blocks / rc.rds_step(c) - 2 <= n_rds <= blocks / rc.rds_step(c) + 2, (c, n_rds)
    short = [c for c in cases if c["n"] <= rc.WIDE_N]
    assert len(short) >= 10 and any(rc.rds_step(c) < 1 for c in short) and any(rc.rds_step(c) > 1 for c in short)


def test_at_most_two_draws_were_set_aside(rgold):
    """a cap, not a measurement: a sample the enclosure of rds_mix.hpp does not pin comes about once in 2^27"""
    assert len(rc.RANDOM_SKIP) <= 2 and rgold["unsure_skipped"] == len(rc.RANDOM_SKIP)
    kept, left = rc.random_draws()
    assert len(kept) == 40 and [c["name"] for c in left] == [f"rds_random{j}" for j in sorted(rc.RANDOM_SKIP)]
