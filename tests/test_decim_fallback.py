"""CPU: the oracle's stage-range probe (oracle/sdro.c, sdro_decim_probe) and the stated properties of the inputs that
tests/test_decim_fallback_gpu.py feeds the decimator's FAST / EXACT kernel pair (tests/decim_edge_cases.py).

The probe says which values a pipeline that keeps stages 1 and 2 in int16 cannot hold and in which 4096-sample chunk the oracle
emits them, without any of the kernels' code.  Here it is pinned to sdro_decim_process (same outputs, same state), it restates
which existing full-scale GPU tests are answered by the EXACT kernel alone, and it checks every condition the builders promise."""
import numpy as np
import pytest

from tests import decim_edge_cases as ec
from tests import oracle_py as orc
from tests import test_oracle_golden as gold

ALL_FC = (ec.FC_INF, ec.FC_SUP, ec.FC_CEN)
CFG = [(log2, fc) for log2 in range(2, 7) for fc in ALL_FC]


def n_chunks(n):
    return (n + ec.CHUNK - 1) // ec.CHUNK


def stored_range(log2, lo, hi):
    """(min, max) over the stages whose outputs the FAST kernel keeps as int16"""
    st = [0] if log2 == 2 else [0, 1] if log2 >= 3 else []
    return (min(int(lo[s].min()) for s in st), max(int(hi[s].max()) for s in st)) if st else (0, 0)


# ---------------------------------------------------------------------------------------------------------------- the probe itself
def test_probe_outputs_equal_process_on_the_golden_inputs():
    meta, cases = gold.decim_inputs()
    cuts = meta["cuts_int16"]
    n = 0
    for name, bits in (("b12", 12), ("b8", 8), ("b16", 16), ("wrap", 16)):
        for log2 in range(0, 7):
            for fc in ALL_FC:
                a, b = orc.Decim(log2, fc, bits), orc.Decim(log2, fc, bits)
                for c0, c1 in zip(cuts[:-1], cuts[1:]):
                    seg = cases[name][c0:c1]
                    out, lo, hi, bad = a.probe(seg)
                    assert np.array_equal(out, b.process(seg)), (name, log2, fc, c0)          # same outputs, same state carried on
                    consumed = out.size // 2 << log2
                    assert bad.size == n_chunks(consumed)
                    if log2 >= 2 and out.size:
                        rl, rh = stored_range(log2, lo, hi)
                        assert bool(bad.any()) == (rl < -32768 or rh > 32767), (name, log2, fc, c0, rl, rh)
                    else:
                        assert not bad.any()
                n += 1
    assert n == 4 * 7 * 3


def test_probe_u8_outputs_equal_process():
    meta, _ = gold.decim_inputs()
    cuts, N = meta["cuts_int16"], meta["recipe"]["N"]
    xu = gold.decimu_input(N)
    for log2 in range(0, 7):
        for fc in ALL_FC:
            a, b = orc.DecimU(log2, fc, 127), orc.DecimU(log2, fc, 127)
            for c0, c1 in zip(cuts[:-1], cuts[1:]):
                out, lo, hi, bad = a.probe(xu[c0:c1])
                assert np.array_equal(out, b.process(xu[c0:c1])), (log2, fc, c0)
                # 8-bit data: |x << pre| <= 128 << pre, gain <= 3.49 per stage: nothing can leave int16
                assert not bad.any(), (log2, fc, c0)


def test_probe_chunk_is_that_of_the_emitting_sample():
    """a lone full-scale pair at the even sample m and its odd neighbour: stage 1 emits 32767 + 0.63 * 32767 when sample m + 31 arrives"""
    for m, want in ((4096 - 32, 0), (4096 - 30, 1), (3 * 4096 - 32, 2), (3 * 4096 - 30, 3)):
        x = np.zeros(2 * 5 * 4096, np.int16)
        x[2 * m] = 32767; x[2 * (m + 1)] = 32767
        _, lo, hi, bad = orc.Decim(2, ec.FC_CEN, 16).probe(x)          # log2 = 2: stage 1 is the only int16-stored stage
        assert hi[0][0] > 32767 and list(np.nonzero(bad)[0]) == [want], (m, hi[0].tolist(), bad.tolist())


# ------------------------------------------------------------------------------------------ what the existing full-scale tests exercise
def test_full_scale_cases_of_the_older_gpu_tests_are_all_flagged():
    """Every chunk of these inputs overflows an int16-stored stage: the EXACT kernel answers those tests (they are the all-flagged end of
    the fallback; tests/test_decim_fallback_gpu.py holds the other end and the middle).  The 12-bit flavour of the same input stays clean."""
    # test_decim_centre_gpu.py::test_centre_fold_ragged_calls
    n = 5 * 16384 + 3 * 1024 + 77
    for log2 in (2, 3, 6):
        for fc in ALL_FC:
            for nw in (1, 4):
                x = orc.synth_iq(n, seed=900 + 11 * log2 + 3 * fc + nw, amp=32767, tone=(0.0031, 20000))
                bad = orc.Decim(log2, fc, 16).probe(x)[3]
                assert (int(bad.sum()), bad.size) == (21, 21), (log2, fc, nw)
    # test_decim_centre_gpu.py::test_centre_fold_full_scale
    n = 3 * 32768 + 500
    x = np.empty(2 * n, np.int16)
    x[0::2] = np.where(np.arange(n) % 3 == 0, -32768, 32767)
    x[1::2] = np.where(np.arange(n) % 5 < 2, 32767, -32768)
    for log2 in (3, 6):
        bad = orc.Decim(log2, ec.FC_CEN, 16).probe(x)[3]
        assert (int(bad.sum()), bad.size) == (25, 25), log2
    # test_decim_gpu.py::test_decim_matches_oracle_split_calls
    n = 3 * 32768 + 4096 + 200
    for log2 in (2, 6):
        for fc in ALL_FC:
            for bits, amp, want in ((16, 32767, 26), (12, 2047, 0)):
                x = orc.synth_iq(n, seed=100 + log2 * 9 + fc * 3 + bits, amp=amp, tone=(0.0021, 0.5 * amp))
                bad = orc.Decim(log2, fc, bits).probe(x)[3]
                assert (int(bad.sum()), bad.size) == (want, 26), (log2, fc, bits)


# ---------------------------------------------------------------------------------------------------------------- builder A
@pytest.mark.parametrize("log2,fcpos", [(1, ec.FC_CEN)] + CFG)
@pytest.mark.parametrize("ragged", (False, True))
def test_full_range_input_is_in_contract_and_reaches_every_extreme(log2, fcpos, ragged):
    lengths = ec.ragged_lengths(log2, fcpos) if ragged else [ec.SPARSE_N]
    x, groups = ec.full_range_stream(log2, fcpos, lengths)
    o = orc.Decim(log2, fcpos, 16)
    a = 0
    for ln in lengths:                                       # condition: the probe reports 0 chunks, call by call
        out, lo, hi, bad = o.probe(x[2 * a: 2 * (a + ln)])
        assert out.size // 2 << log2 == ln and bad.size == n_chunks(ln) and not bad.any(), (a, ln, np.nonzero(bad)[0].tolist())
        a += ln
    full = {k: (True, True) for k in ((0, 0), (0, 1), (1, 0), (1, 1))}
    a = 0
    for ln in lengths:                                       # condition: all four arms hold both extremes in ...
        assert ec.arm_extremes(x, a, a + 32) == full, ("first block", a)                # ... the first block's window of every call
        assert ec.arm_extremes(x, a + ln - 32, a + ln) == full, ("last block", a + ln)  # ... its last (partial) block's
        a += ln
    tail = [b for b in range(1024, sum(lengths), 1024) if ec.arm_extremes(x, b - 32, b) == full]
    assert len(tail) >= 8 and any(b % ec.CHUNK == 0 for b in tail), tail               # ... the last block of a sub-chunk / of a chunk
    assert any(ec.arm_extremes(x, b, b + 32) == full for b in range(ec.CHUNK, sum(lengths) - 32, ec.CHUNK))
    if not ragged:
        # the calls of the ragged run keep the consumed stream: the dropped tails are full scale and shorter than a group
        calls = ec.with_dropped_tails(x, [ec.SPARSE_N], log2, fcpos)
        assert np.array_equal(orc.Decim(log2, fcpos, 16).process(calls[0]), orc.Decim(log2, fcpos, 16).process(x))


# ---------------------------------------------------------------------------------------------------------------- builder B
@pytest.mark.parametrize("log2,fcpos", CFG)
def test_edge_landing_hits_each_target_exactly(log2, fcpos):
    stages = [1] if log2 == 2 else [1, 2]
    x, events = ec.edge_landing(log2, fcpos, ec.INSIDE)
    assert len(events) == 4 * len(stages)
    _, lo, hi, bad = orc.Decim(log2, fcpos, 16).probe(x)
    assert not bad.any()                                     # the two inside targets: 0 chunks ...
    for s in stages:
        for c in (0, 1):                                     # ... and the peaks ARE the ends of the int16 range
            assert (int(lo[s - 1][c]), int(hi[s - 1][c])) == (-32768, 32767), (s, c)
    x, events = ec.edge_landing(log2, fcpos, ec.OUTSIDE)
    _, lo, hi, bad = orc.Decim(log2, fcpos, 16).probe(x)
    chunks = sorted(e[3] for e in events)
    assert len(set(chunks)) == len(chunks) == 4 * len(stages)
    assert np.nonzero(bad)[0].tolist() == chunks             # the two outside targets: exactly the chunk that holds each event
    for s in stages:
        for c in (0, 1):                                     # one step over the edge, no further
            assert (int(lo[s - 1][c]), int(hi[s - 1][c])) == (-32769, 32768), (s, c)
    if log2 >= 3:
        assert int(lo[0].min()) >= -32769 and int(hi[0].max()) <= 32768


# ---------------------------------------------------------------------------------------------------------------- builder C
@pytest.mark.parametrize("log2,fcpos", CFG)
@pytest.mark.parametrize("case", ("before", "around", "ends"))
def test_sparse_events_flag_their_chunks_and_leave_most_clean(log2, fcpos, case):
    x, pos = ec.sparse_events(log2, fcpos, case)
    assert x.size == 2 * ec.SPARSE_N and ec.SPARSE_N % ec.group_cplx(log2, fcpos) == 0
    _, lo, hi, bad = orc.Decim(log2, fcpos, 16).probe(x)
    assert bad.size == n_chunks(ec.SPARSE_N) == 41
    want = {p // ec.CHUNK for p in pos}
    got = set(np.nonzero(bad)[0].tolist())
    # every event flags the chunk of its emitting sample; a stage-1 event under an even stage-2 index may also carry on into stage 2,
    # 62 samples later
    assert want <= got <= want | {(p + 62) // ec.CHUNK for p in pos}, (sorted(got), sorted(want))
    assert 2 * len(got) <= bad.size                          # condition: at least half of the chunks are clean
    rl, rh = stored_range(log2, lo, hi)
    assert rl >= -32769 - 4000 and rh <= 32768 + 4000        # single steps over the edge (and their stage-2 echo), not full-scale garbage
    # the positions are what the issue lists, relative to the pinned segment starts
    f = 2 * ec.SEG
    if case == "before":
        assert pos[0] == f - 4097
    if case == "ends":
        assert pos[0] // ec.CHUNK == 0 and pos[-1] // ec.CHUNK == 40 and pos[-2] // ec.CHUNK == 39


# ---------------------------------------------------------------------------------------------------------------- builder D
@pytest.mark.parametrize("log2,fcpos", CFG)
def test_noise_levels_sit_between_clean_and_all_flagged(log2, fcpos):
    for amp in ec.NOISE_AMPS[log2]:
        bad = orc.Decim(log2, fcpos, 16).probe(ec.noise(amp))[3]
        assert bad.size == 64 and 0.02 * bad.size <= int(bad.sum()) <= 0.5 * bad.size, (amp, int(bad.sum()))
    if log2 == 6 and fcpos == ec.FC_CEN:
        counts = [int(orc.Decim(6, ec.FC_CEN, 16).probe(ec.noise(a))[3].sum()) for a in (6000, 8000, 10000)]
        assert counts == [0, 5, 63], counts


def test_allowed_flags_bound():
    bad = np.zeros(12, np.uint8); bad[5] = 1
    plain = ec.allowed_flags(bad, 6, skewed=False)
    assert np.nonzero(plain)[0].tolist() == [5, 6, 7]                         # to the end of its segment, nothing else
    assert np.nonzero(ec.allowed_flags(bad, 6, skewed=True))[0].tolist() == [4, 5, 6, 7]
    bad[:] = 0; bad[7] = 1
    assert np.nonzero(ec.allowed_flags(bad, 3, skewed=True))[0].tolist() == [6, 7, 8, 9, 10, 11]     # its own tail + the next segment's warm-up
    assert np.nonzero(ec.allowed_flags(np.zeros(6, np.uint8), 3, False, warm_event=True))[0].tolist() == [0, 1, 2, 3]
