"""Inputs for the decimator's FAST / EXACT boundary (tests/test_decim_fallback.py on the CPU, tests/test_decim_fallback_gpu.py on
the device).  Plain numpy, deterministic.  Every property stated here is CHECKED by the oracle's stage-range probe
(oracle_py.Decim.probe) in tests/test_decim_fallback.py: the builders construct, the probe decides.

The FAST kernel keeps the outputs of stages 1 and 2 as int16 when a later stage reads them (stage 1 for log2 >= 2, stage 2 for
log2 >= 3) and flags, per 4096-sample chunk, the ones that do not fit; the EXACT kernel recomputes the flagged chunks.

Facts about one half-band stage the builders lean on (oracle/sdro.c, hb_push):
  * a stage emits an output when its input with an ODD index n arrives; the 32 taps read the odd inputs n, n - 2, .. n - 62 and
    the centre tap (2^11, gain exactly 1) reads the EVEN input n - 31.  An even input therefore reaches exactly one output, through
    the centre tap, with gain exactly 1: adding d to it adds d to that output and to nothing else of the stage;
  * the inf / sup rotations only swap or negate the components of an input before it is stored (SRC below);
  * output k of stage 1 is input k of stage 2.  An even input sample m of the chain reaches stage-1 output k = m / 2 + 15 (emitted
    by input sample m + 31); when k is even (m = 2 mod 4) that output is the centre sample of the stage-2 output emitted by input
    sample m + 93.
All positions are indices of complex samples in the CONSUMED stream (what the group rule keeps), counted from the last reset."""
import functools

import numpy as np

from tests import oracle_py as orc

FC_INF, FC_SUP, FC_CEN = 0, 1, 2
CHUNK = 4096
SEG = 4 * CHUNK                 # the GPU tests pin the FAST kernel's segment to this: SDRX_DECIM_SPW = 16 (one wave) / 4 (four waves)
SPW_ENV = {1: "16", 4: "4"}


def stage_modes(log2, fcpos):
    """0 centre, 1 inf, 2 sup per stage (decimateK_inf: Inf, Sup, .., Sup, Cen; _sup: Sup, Inf, .., Inf, Cen; K = 4: the pair)"""
    if fcpos == FC_CEN:
        return [0] * log2
    first = 1 if fcpos == FC_INF else 2
    return [first if s == 0 else 0 if (log2 >= 3 and s == log2 - 1) else 3 - first for s in range(log2)]


def group_cplx(log2, fcpos):
    """complex samples per loop iteration of decimateK_x: calls consume whole groups"""
    if log2 == 0:
        return 1
    g = (4 << log2) if log2 <= 2 else ((2 << log2) if fcpos == FC_CEN else (4 << log2))
    return g // 2


# SRC[mode][phase][c] = (component of the raw sample, sign): stored component c of input n (phase n & 3) = sign * raw[component]
_ID = ((0, 1), (1, 1))
_NEG = ((0, -1), (1, -1))
SRC = {
    0: (_ID, _ID, _ID, _ID),
    1: (((1, -1), (0, 1)), _NEG, ((1, 1), (0, -1)), _ID),      # inf: (-y, x) (-x, -y) (y, -x) (x, y)
    2: (((1, 1), (0, -1)), _NEG, ((1, -1), (0, 1)), _ID),      # sup: (y, -x) (-x, -y) (-y, x) (x, y)
}


def put(x, mode, n, c, v):
    """make the STORED component c of stage-1 input n equal v (x: interleaved int64 work array)"""
    sc, sg = SRC[mode][n & 3][c]
    x[2 * n + sc] = sg * v


def stored_of_raw(mode, n, rc):
    """(stored component, sign) that the raw component rc of input n lands in"""
    for c in (0, 1):
        sc, sg = SRC[mode][n & 3][c]
        if sc == rc:
            return c, sg
    raise AssertionError


def finish(x):
    assert x.min() >= -32768 and x.max() <= 32767, (int(x.min()), int(x.max()))
    return x.astype(np.int16)


def quiet_base(n, seed, amp=300):
    """low-level noise: with the worst-case gain of 3.49 per stage nothing of it comes near the int16 range"""
    rng = np.random.Generator(np.random.PCG64(seed))
    return rng.integers(-amp, amp + 1, size=2 * n, dtype=np.int64)


# ---------------------------------------------------------------------------------------------------------------- events (B, C)
BURST = 3000


def write_event(x, modes, stage, m, c, sgn, d):
    """Zero the samples the targeted output can see, then write the event: the centre sample d and, on the two inputs of the
    targeted stage next to it, sgn * BURST (both meet the largest tap, which is positive), all on stored component c of that stage.
    stage 1: inputs m - 1, m, m + 1 of the chain.  stage 2: its inputs k - 1, k, k + 1 (k = m / 2 + 15) are the stage-1 outputs that
    the chain's even inputs m - 2, m, m + 2 alone produce (everything odd around them is zero)."""
    lo = max(m - 96, 0)
    x[2 * lo: 2 * (m + 97)] = 0
    if stage == 1:
        assert m % 2 == 0 and m >= 1
        for n, v in ((m - 1, sgn * BURST), (m, d), (m + 1, sgn * BURST)):
            put(x, modes[0], n, c, v)
    else:
        assert m % 4 == 2 and m >= 2 and len(modes) >= 2
        k = m // 2 + 15
        for kk, v in ((k - 1, sgn * BURST), (k, d), (k + 1, sgn * BURST)):
            sc, sg = SRC[modes[1]][kk & 3][c]          # stage 2 stores sg * (component sc of stage-1 output kk) ...
            put(x, modes[0], 2 * kk - 30, sc, sg * v)  # ... which is the stored component sc of the chain's even input 2 kk - 30


def emit_pos(stage, m):
    """input sample whose arrival emits the targeted output"""
    return m + 31 if stage == 1 else m + 93


@functools.lru_cache(maxsize=None)
def centre_value(log2, fcpos, stage, c, target, m_mod8):
    """the centre sample that lands the event's output exactly on `target`: measured once on a short all-zero stream with the probe
    (the centre tap has gain exactly 1, so the miss of a first guess is the correction)"""
    sgn = 1 if target > 0 else -1
    modes = stage_modes(log2, fcpos)
    z = np.zeros(2 * 1024, np.int64)
    m = 512 + m_mod8
    d0 = sgn * 20000
    write_event(z, modes, stage, m, c, sgn, d0)
    _out, lo, hi, _bad = orc.Decim(log2, fcpos, 16).probe(finish(z))
    peak = int(hi[stage - 1][c]) if sgn > 0 else int(lo[stage - 1][c])
    d = d0 + target - peak
    assert abs(d) <= 32767, d
    return d


def add_event(x, log2, fcpos, stage, m, c, target):
    d = centre_value(log2, fcpos, stage, c, target, m % 8)
    write_event(x, stage_modes(log2, fcpos), stage, m, c, 1 if target > 0 else -1, d)
    return emit_pos(stage, m)


INSIDE, OUTSIDE = (32767, -32768), (32768, -32769)


def edge_landing(log2, fcpos, targets):
    """B.  One stream holding, for each int16-stored stage, each component and each of the two `targets`, one event whose output is
    exactly the target; every event sits in the middle of a chunk of its own, in segments apart.  Stage-1 events use m = 0 mod 4:
    their output is then an ODD input of stage 2 (taps only, gain < 0.64), so the event stays a stage-1 event.
    Returns (x, [(stage, component, target, chunk of the emitting sample)])."""
    stages = [1] if log2 == 2 else [1, 2]
    n = 36 * CHUNK + 5 * 128
    x = quiet_base(n, 7000 + 10 * log2 + fcpos)
    events = []
    i = 0
    for stage in stages:
        for c in (0, 1):
            for t in targets:
                chunk = 1 + 4 * i + (i % 3)            # spread over the segments, at different places inside them
                m = chunk * CHUNK + 2000 + (0 if stage == 1 else 2)
                p = add_event(x, log2, fcpos, stage, m, c, t)
                assert p // CHUNK == chunk
                events.append((stage, c, t, chunk))
                i += 1
    return finish(x), events


def sparse_positions(n):
    """C.  Emission positions of the three sparse cases, relative to the starts f of segments 2, 4, 6, 8 (SEG samples each).
    Stage outputs are emitted by odd input samples only: the even positions of the list f - 4096, f - 3906, f, f + 1024, f + 4096
    stand as the next odd sample."""
    f = [j * SEG for j in range(16)]
    last_full = (n // CHUNK - 1) * CHUNK
    return {
        "before": [f[2] - 4097, f[4] - 4095, f[6] - 3907, f[8] - 3905],
        "around": [f[2] - 1, f[4] + 1, f[6] + 1023, f[8] + 1025],
        "ends": [131, f[2] + 4095, f[4] + 4097, last_full + 2047, (n // CHUNK) * CHUNK + 703],
    }


SPARSE_N = 40 * CHUNK + 11 * 128                      # ten segments and a partial last chunk


def sparse_events(log2, fcpos, case):
    """C.  A clean base plus single over-the-edge events (32768 / -32769) at the listed emission positions.  Every second event is a
    stage-2 event where log2 >= 3 and the position allows one (stage 2 emits at samples 3 mod 4).  Returns (x, [positions])."""
    n = SPARSE_N
    x = quiet_base(n, 7100 + 10 * log2 + fcpos)
    pos = sparse_positions(n)[case]
    for i, p in enumerate(pos):
        stage = 2 if (log2 >= 3 and i % 2 == 1 and (p - 93) % 4 == 2) else 1
        m = p - (31 if stage == 1 else 93)
        got = add_event(x, log2, fcpos, stage, m, i % 2, OUTSIDE[(i // 2) % 2])
        assert got == p
    return finish(x), pos


# amplitudes of plain uniform noise (orc.synth_iq, seed 5) whose flagged share the probe puts inside [2 %, 50 %] for every fcpos:
# 8000 for log2 >= 3 (stage 2 decides); stage 1 alone (log2 = 2) needs more.  The second entry is the per-log2 choice.
NOISE_AMPS = {2: (13000, 13200), 3: (8000, 8500), 4: (8000, 8500), 5: (8000, 8500), 6: (8000, 8500)}
NOISE_N = 64 * CHUNK


def noise(amp, n=NOISE_N):
    return orc.synth_iq(n, seed=5, amp=amp)


# ---------------------------------------------------------------------------------------------------------------- A: full range
PULL_ODD, PULL_EVEN = 6000, 12000
GROUP_SPAN = 30                                       # a group of extremes occupies samples g - 1 .. g + 26


def put_extremes(x, mode, g):
    """All eight raw extremes (both int16 ends on the even and the odd arm of I and of Q) inside 28 samples, in contract:
      even arm  g: (32767, 32767)   g + 8: (-32768, -32768)     odd arm  g + 17: (32767, 32767)   g + 25: (-32768, -32768)
    An even-arm extreme reaches one stage-1 output with gain 1; its two odd neighbours carry PULL_ODD of the opposite (stored) sign and
    pull that output 7600 inside.  An odd-arm extreme reaches two outputs with gain 0.63; the even samples under their centre taps
    carry PULL_EVEN of the opposite sign.  Whatever the rotation does to a raw -32768 (a negated one is stored as +32768), the pulls
    follow the stored sign."""
    assert g % 2 == 0 and g >= 1
    x[2 * (g - 1): 2 * (g + 27)] = 0
    for n, v in ((g, 32767), (g + 8, -32768), (g + 17, 32767), (g + 25, -32768)):
        x[2 * n] = v; x[2 * n + 1] = v
        for rc in (0, 1):
            c, sg = stored_of_raw(mode, n, rc)
            pull = -(1 if sg * v > 0 else -1) * (PULL_ODD if n % 2 == 0 else PULL_EVEN)
            put(x, mode, n - 1, c, pull)
            put(x, mode, n + 1, c, pull)


def full_range_stream(log2, fcpos, lengths):
    """A.  A quiet stream cut into calls of `lengths` consumed samples, with a group of extremes
      * in the first 32 samples of every call (the window of its first block of 16 stage-1 outputs),
      * in the last 32 samples of every call (its last block, partial when the length is no multiple of 32),
      * in front of every 1024-sample boundary that has room (the last block of a sub-chunk: the tile whose second K-step and
        extra centre read reach the end of the array) and behind every 4096-sample one.
    Returns (x, [g of every group])."""
    n = sum(lengths)
    x = quiet_base(n, 7200 + 10 * log2 + fcpos, amp=200)
    mode = stage_modes(log2, fcpos)[0] if log2 else 0
    edges, inner = [], []
    a = 0
    for ln in lengths:
        assert ln >= 2 * GROUP_SPAN
        edges += [a + 2, a + ln - 28]
        a += ln
    for b in range(1024, n, 1024):
        inner.append(b - 28)
        if b % CHUNK == 0:
            inner.append(b + 2)
    groups = []
    for g in edges + inner:                            # the calls' edges first; a boundary group only where it shares no sample with another
        if g - 1 >= 0 and g + 27 <= n and all(abs(g - h) >= 28 for h in groups):
            put_extremes(x, mode, g)
            groups.append(g)
    groups.sort()
    return finish(x), groups


def ragged_lengths(log2, fcpos):
    """consumed samples per call of the ragged A case: whole groups, otherwise as uneven as the group allows"""
    gc = group_cplx(log2, fcpos)
    return [max(t // gc, 1) * gc for t in (1000, 3111, 4096 + 15 + 35906, 92395)]


def with_dropped_tails(x, lengths, log2, fcpos):
    """the calls of a ragged run: each piece of the consumed stream followed by full-scale samples short of one group, which the
    group rule drops (a kernel that consumed them would overflow at once)"""
    gc = group_cplx(log2, fcpos)
    calls, a = [], 0
    for i, ln in enumerate(lengths):
        junk = np.tile(np.array([32767, -32768], np.int16), (gc - 1) if i % 2 == 0 else gc // 2)
        calls.append(np.concatenate([x[2 * a: 2 * (a + ln)], junk]))
        a += ln
    return calls


def arm_extremes(x, a, b):
    """{(arm parity, component): (holds -32768, holds 32767)} over consumed samples [a, b)"""
    out = {}
    for par in (0, 1):
        idx = np.arange(a + ((par - a) % 2), b, 2)
        for c in (0, 1):
            v = x[2 * idx + c]
            out[(par, c)] = (bool((v == -32768).any()), bool((v == 32767).any()))
    return out


# ---------------------------------------------------------------------------------------------------------------- flag bounds
def allowed_flags(bad, log2, skewed, warm_event=False, seg_chunks=SEG // CHUNK):
    """Upper bound of the FAST kernel's flags for one call, from the probe's per-chunk bytes `bad`: a chunk may be flagged only if
    its segment holds an event at or before it, or the 4096 samples in front of its segment do (`warm_event`: the previous call's
    tail, for segment 0).  skewed (single-wave matrix-core flavour): stage 1 runs log2 - 1 sub-chunks of 1024 ahead of the flag
    writer, so an event up to that far behind the chunk, in the same segment, also counts (at chunk granularity: (log2 + 2) // 4
    chunks)."""
    n = bad.size
    ok = np.zeros(n, bool)
    ahead = (log2 + 2) // 4 if skewed else 0
    for c in range(n):
        s0 = (c // seg_chunks) * seg_chunks
        s1 = min(s0 + seg_chunks, n)
        warm = bool(bad[s0 - 1]) if s0 > 0 else warm_event
        ok[c] = warm or bad[s0: c + 1].any() or bad[c + 1: min(c + 1 + ahead, s1)].any()
    return ok
