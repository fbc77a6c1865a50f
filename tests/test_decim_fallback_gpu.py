"""GPU: the decimator's FAST kernel and its EXACT fallback where they share a call (sdrangel_amd/csrc/sdrx_decim.hip, launch_batch).

The FAST kernel (decim_fast_kernel.hpp) keeps the outputs of stages 1 and 2 as int16 when a later stage reads them, flags every
4096-sample chunk from the first value that does not fit to the end of the wave's segment, and the EXACT kernel (decim_kernel.hpp)
recomputes the flagged chunks.  The older full-scale tests flag every chunk (tests/test_decim_fallback.py counts them), so there the
EXACT kernel answers alone; the 8 / 12-bit tests flag none and never show the FAST kernel a large operand.  These cases sit in between:

  * full-range data that stays in contract, and outputs landing exactly ON the ends of the int16 range: no flag, outputs kept from FAST;
  * outputs one step OVER the edge, sparse events at the segment / warm-up / sub-chunk boundaries, noise at the level where a few
    chunks overflow: flags must cover what the oracle's probe reports (nothing missed) and stay inside what the flag rule allows
    (nothing extra: a kernel that flags everything computes the right samples with the speed work switched off);
  * the same across calls, in a batch, on the pinned ring, over get_state / set_state, and for the unsigned 8-bit flavour.

Everything is bit-exact against the CPU oracle; the inputs and their properties are tests/decim_edge_cases.py (checked on the CPU).
Both engines, both flavours (one wave / four waves per segment, segment pinned to 16384 samples), log2 = 2 .. 6, the three fcpos."""
import functools

import numpy as np
import pytest

import sdrangel_amd as sa
from tests import decim_edge_cases as ec
from tests import oracle_py as orc

pytestmark = pytest.mark.gpu

CFG = [(log2, fc) for log2 in range(2, 7) for fc in (sa.FC_CEN, sa.FC_INF, sa.FC_SUP)]
FLAVOURS = [(e, nw) for e in ("mfma", "valu") for nw in (1, 4)]


@pytest.fixture(params=FLAVOURS, ids=lambda p: f"{p[0]}-nw{p[1]}")
def flavour(request, monkeypatch):
    eng, nw = request.param
    monkeypatch.setenv("SDRX_DECIM_ENGINE", eng)
    monkeypatch.setenv("SDRX_DECIM_NW", str(nw))
    monkeypatch.setenv("SDRX_DECIM_SPW", ec.SPW_ENV[nw])
    monkeypatch.delenv("SDRX_DECIM_PATH", raising=False)
    return eng, nw


def skewed(flavour):
    """the single-wave matrix-core flavour runs stage 1 ahead of the flag writer (decim_fast_kernel.hpp, skewed loop)"""
    return flavour == ("mfma", 1)


def chunks_of(n):
    return (n + ec.CHUNK - 1) // ec.CHUNK


@functools.lru_cache(maxsize=None)
def reference(kind, log2, fcpos):
    """the calls of one case with the oracle's answer to each: [(call buffer, outputs, probe bytes)], one oracle object across the calls"""
    if kind == "A":
        calls = [ec.full_range_stream(log2, fcpos, [ec.SPARSE_N])[0]]
    elif kind == "A-ragged":
        lengths = ec.ragged_lengths(log2, fcpos)
        calls = ec.with_dropped_tails(ec.full_range_stream(log2, fcpos, lengths)[0], lengths, log2, fcpos)
    elif kind == "B-inside":
        calls = [ec.edge_landing(log2, fcpos, ec.INSIDE)[0]]
    elif kind == "B-outside":
        calls = [ec.edge_landing(log2, fcpos, ec.OUTSIDE)[0]]
    elif kind.startswith("C-"):
        calls = [ec.sparse_events(log2, fcpos, kind[2:])[0]]
    elif kind.startswith("D-"):
        calls = [ec.noise(ec.NOISE_AMPS[log2][int(kind[2:])])]
    else:
        raise KeyError(kind)
    o = orc.Decim(log2, fcpos, 16)
    out = []
    for c in calls:
        want, _lo, _hi, bad = o.probe(c)
        out.append((c, want, bad))
    return out


def run_calls(ref, log2, fcpos, tag):
    """a fresh handle over the calls of `ref`: outputs must equal the oracle's; returns last_fallback() of every call"""
    g = sa.Decimators(log2, fcpos, 16)
    reports = []
    for i, (x, want, bad) in enumerate(ref):
        got = g.decimate(x)
        assert got.size == want.size, (tag, i, got.size, want.size)
        if not np.array_equal(got, want):
            d = np.nonzero(got != want)[0]
            raise AssertionError((tag, i, "first differing int16", int(d[0]), "of", int(d.size), "chunk", int(d[0] // 2 << log2) // ec.CHUNK))
        rep = g.last_fallback()
        assert rep["total"] == bad.size == chunks_of(want.size // 2 << log2), (tag, i, rep["total"], bad.size)
        assert rep["flagged"] == int(rep["flags"].sum())
        reports.append(rep)
    return reports


def check_flags(flags, bad, log2, flav, tag, warm_event=False):
    missed = np.nonzero((bad != 0) & (flags == 0))[0]
    assert missed.size == 0, (tag, "overflowing chunks the FAST kernel did not flag", missed.tolist())
    extra = np.nonzero((flags != 0) & ~ec.allowed_flags(bad, log2, skewed(flav), warm_event))[0]
    assert extra.size == 0, (tag, "chunks flagged without an event in reach", extra.tolist(), "probe", np.nonzero(bad)[0].tolist())


# ------------------------------------------------------------------------------------------------------------ FAST alone, full range
@pytest.mark.parametrize("log2,fcpos", CFG)
def test_fast_kernel_alone_on_full_range_data(log2, fcpos, flavour, monkeypatch):
    """Kept FAST outputs meet window entries at both ends of the int16 range (inputs A: all four arms, ragged call ends included) and
    outputs that ARE the ends (inputs B, inside targets).  Auto mode must flag nothing; SDRX_DECIM_PATH=fast (no fallback) must agree
    with the oracle just the same."""
    for kind in ("A", "A-ragged", "B-inside"):
        ref = reference(kind, log2, fcpos)
        assert not any(bad.any() for _, _, bad in ref)
        for rep in run_calls(ref, log2, fcpos, (kind, "auto")):
            assert rep["flagged"] == 0, (kind, np.nonzero(rep["flags"])[0].tolist())
    monkeypatch.setenv("SDRX_DECIM_PATH", "fast")
    for kind in ("A", "A-ragged", "B-inside"):
        for rep in run_calls(reference(kind, log2, fcpos), log2, fcpos, (kind, "fast")):
            assert rep["flagged"] == 0, kind


def test_full_range_log2_1_has_nothing_to_flag(flavour):
    """log2 = 1 stores no stage as int16: the report counts the chunks and flags none"""
    for fcpos in (sa.FC_CEN, sa.FC_INF):
        x = ec.full_range_stream(1, fcpos, [ec.SPARSE_N])[0]
        g = sa.Decimators(1, fcpos, 16)
        assert np.array_equal(g.decimate(x), orc.Decim(1, fcpos, 16).process(x))
        rep = g.last_fallback()
        assert (rep["flagged"], rep["total"]) == (0, chunks_of(ec.SPARSE_N))


# ------------------------------------------------------------------------------------------------------------ nothing missed, nothing extra
@pytest.mark.parametrize("log2,fcpos", CFG)
def test_flags_cover_the_events_and_nothing_out_of_reach(log2, fcpos, flavour):
    for kind in ("B-outside", "C-before", "C-around", "C-ends", "D-0", "D-1"):
        ref = reference(kind, log2, fcpos)
        assert ref[0][2].any() and 2 * int(ref[0][2].sum()) <= ref[0][2].size
        (rep,) = run_calls(ref, log2, fcpos, kind)
        check_flags(rep["flags"], ref[0][2], log2, flavour, kind)
        if int(ec.allowed_flags(ref[0][2], log2, skewed(flavour)).sum()) < rep["total"]:
            assert rep["flagged"] < rep["total"], kind      # kept FAST outputs and recomputed ones side by side


# ------------------------------------------------------------------------------------------------------------ across calls
N1 = 9 * ec.CHUNK + 11 * 128         # call N: a partial last chunk
N2 = 5 * ec.CHUNK


@functools.lru_cache(maxsize=None)
def two_calls(log2, fcpos, where):
    x = ec.quiet_base(N1 + N2, 7300 + 10 * log2 + fcpos)
    gc = ec.group_cplx(log2, fcpos)
    junk = np.zeros(2 * (gc - 1), np.int16)
    if where == "inside":                # the event and everything it can see lie in the last 3906 samples of call N
        stage = 2 if log2 >= 3 else 1
        ec.add_event(x, log2, fcpos, stage, N1 - 2000 - (2 if stage == 2 else 0), 1, 32768)
    elif where == "outside":             # emitted 4597 samples before the end: call N + 1's warm-up never sees it
        ec.add_event(x, log2, fcpos, 1, N1 - 4628, 0, -32769)
    else:                                # "dropped": full scale in the tail that the group rule drops; nothing of it may be seen
        junk = np.tile(np.array([32767, 32767], np.int16), gc - 1)
    x = ec.finish(x)
    calls = [np.concatenate([x[: 2 * N1], junk]), x[2 * N1:]]
    o = orc.Decim(log2, fcpos, 16)
    out = []
    for c in calls:
        want, _lo, _hi, bad = o.probe(c)
        out.append((c, want, bad))
    return out


@pytest.mark.parametrize("where", ("inside", "outside", "dropped"))
@pytest.mark.parametrize("log2,fcpos", CFG)
def test_event_in_the_tail_of_a_call_reaches_the_next_through_the_history(log2, fcpos, where, flavour):
    ref = two_calls(log2, fcpos, where)
    assert bool(ref[0][2].any()) == (where != "dropped") and not ref[1][2].any()
    rep = run_calls(ref, log2, fcpos, where)
    check_flags(rep[0]["flags"], ref[0][2], log2, flavour, (where, "call N"))
    check_flags(rep[1]["flags"], ref[1][2], log2, flavour, (where, "call N + 1"), warm_event=(where == "inside"))
    # the first chunk of call N + 1 is flagged exactly when the event lies inside its warm-up window (the history's 4096 samples)
    assert bool(rep[1]["flags"][0]) == (where == "inside"), (where, rep[1]["flags"].tolist())
    if where == "dropped":
        assert rep[0]["flagged"] == 0 and rep[1]["flagged"] == 0


@pytest.mark.parametrize("log2,fcpos", [(3, sa.FC_INF), (6, sa.FC_CEN)])
def test_state_saved_right_after_a_spike_carries_it_to_another_handle(log2, fcpos, flavour):
    ref = two_calls(log2, fcpos, "inside")
    g = sa.Decimators(log2, fcpos, 16)
    assert np.array_equal(g.decimate(ref[0][0]), ref[0][1])
    assert g.last_fallback()["flags"][(N1 - 1909) // ec.CHUNK] == 1
    h = sa.Decimators(log2, fcpos, 16)
    h.set_state(g.get_state())
    assert np.array_equal(h.decimate(ref[1][0]), ref[1][1])
    rep = h.last_fallback()
    assert rep["flags"][0] == 1 and rep["total"] == chunks_of(N2)
    check_flags(rep["flags"], ref[1][2], log2, flavour, "set_state", warm_event=True)


# ------------------------------------------------------------------------------------------------------------ other entry points
def test_batch_reports_every_stream_on_its_own_handle(flavour):
    torch = pytest.importorskip("torch")
    log2, fcpos = 5, sa.FC_INF
    refs = [reference("A", log2, fcpos)[0], reference("C-around", log2, fcpos)[0], reference("B-inside", log2, fcpos)[0]]
    hs = [sa.Decimators(log2, fcpos, 16) for _ in refs]
    d_in = [torch.from_numpy(np.concatenate([x, np.zeros(8, np.int16)])).cuda() for x, _, _ in refs]
    d_out = [torch.zeros(x.size + 64, dtype=torch.int16, device="cuda") for x, _, _ in refs]
    torch.cuda.synchronize()
    n_out = sa.decimate_dev_batch(hs, [t.data_ptr() for t in d_in], [x.size for x, _, _ in refs], [t.data_ptr() for t in d_out])
    hs[0].sync()
    for i, (x, want, bad) in enumerate(refs):
        assert np.array_equal(d_out[i][: 2 * n_out[i]].cpu().numpy(), want), i
        rep = hs[i].last_fallback()
        assert rep["total"] == bad.size, (i, rep["total"])
        if i == 1:
            check_flags(rep["flags"], bad, log2, flavour, "batch, spiky stream")
            assert 0 < rep["flagged"] < rep["total"]
        else:
            assert rep["flagged"] == 0, (i, np.nonzero(rep["flags"])[0].tolist())      # a neighbour's overflow is not this stream's


def test_ring_slot_with_a_spike_between_clean_ones(flavour):
    log2, fcpos = 4, sa.FC_SUP
    slot = 5 * ec.CHUNK
    x = ec.quiet_base(4 * slot, 7400)
    ec.add_event(x, log2, fcpos, 2, 2 * slot - 2002, 0, -32769)             # in the tail of slot 1: slot 2 warms up over it
    x = ec.finish(x)
    g = sa.Decimators(log2, fcpos, 16)
    o = orc.Decim(log2, fcpos, 16)
    g.ring_create(2 * slot, 4, 1)                                            # flush = 1: every slot is a call of its own
    for k in range(4):
        seg = x[2 * k * slot: 2 * (k + 1) * slot]
        g.ring_acquire()[:] = seg
        g.ring_submit(seg.size)
        want, _, _, bad = o.probe(seg)
        rep = g.last_fallback()
        assert np.array_equal(g.ring_retire(), want), k
        assert rep["total"] == 5
        check_flags(rep["flags"], bad, log2, flavour, ("ring", k), warm_event=(k == 2))
        assert bool(bad.any()) == (k == 1) and bool(rep["flags"][0]) == (k == 2), (k, rep["flags"].tolist())
        if k in (0, 3):
            assert rep["flagged"] == 0


@pytest.mark.parametrize("fcpos", (sa.FC_CEN, sa.FC_INF, sa.FC_SUP))
def test_unsigned_8_bit_data_can_never_flag(fcpos, flavour):
    """DecimatorsU: |(byte - shift) << pre| <= 128 << pre; with 3.49 per stage nothing comes near int16, whatever the bytes"""
    n = 24 * ec.CHUNK + 640
    rng = np.random.Generator(np.random.PCG64(77))
    x = rng.integers(0, 256, size=2 * n, dtype=np.int64).astype(np.uint8)
    x[2000:6000] = 0; x[6000:10000] = 255; x[10000:14000:2] = 0; x[10001:14000:2] = 255
    x[20000:24000] = np.where(np.arange(4000) % 4 < 2, 0, 255)
    for log2 in range(1, 7):
        g = sa.DecimatorsU(log2, fcpos, 127)
        want, _, _, bad = orc.DecimU(log2, fcpos, 127).probe(x)
        assert not bad.any()
        assert np.array_equal(g.decimate(x), want), log2
        rep = g.last_fallback()
        assert (rep["flagged"], rep["total"]) == (0, chunks_of(n)), (log2, rep["flagged"], rep["total"])


def test_report_is_empty_when_no_fast_launch_ran(flavour, monkeypatch):
    x = ec.noise(8000, 8 * ec.CHUNK)
    g = sa.Decimators(0, sa.FC_CEN, 16)
    g.decimate(x)
    assert (g.last_fallback()["flagged"], g.last_fallback()["total"]) == (0, 0)       # log2 = 0: no half-band at all
    g = sa.Decimators(6, sa.FC_CEN, 16)
    g.decimate(x)
    assert g.last_fallback()["total"] == 8
    g.decimate(x[:2])                                                                  # shorter than a group: nothing launched
    assert g.last_fallback()["total"] == 0
    monkeypatch.setenv("SDRX_DECIM_PATH", "exact")
    g = sa.Decimators(6, sa.FC_CEN, 16)
    assert np.array_equal(g.decimate(x), orc.Decim(6, sa.FC_CEN, 16).process(x))
    assert (g.last_fallback()["flagged"], g.last_fallback()["total"]) == (0, 0)
