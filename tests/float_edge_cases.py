"""Inputs from the regimes where a GPU build and a strict-IEEE x86 build of the float paths can part company, and the
comparisons that go with them: float -> integer conversions outside the int32 range, silence after signal in the
per-stream recurrences, subnormals, signed zeros and non-finite values.  Shared by tests/test_float_edges.py (CPU:
the oracle alone, and the oracle against the compiled reference) and tests/test_float_edges_gpu.py.

GPU-free and free of the product: numpy and tests/synth.py only.  Every input is built from the integer generator of
tests/synth.py and from bit patterns, so the same float32 bits come out on every platform -- tests/golden/
fdecim_edges_golden.npz records the reference's outputs on them."""
import numpy as np

from tests import synth

FC_INF, FC_SUP, FC_CEN = 0, 1, 2


# ------------------------------------------------------------------------------------------------ comparisons
def same_bits(a, b) -> bool:
    """raw-bit equality of float32 arrays, except that a NaN on both sides counts as equal (x86 produces the negative
    default NaN, the GPU the positive one: not a difference in the operation).  The sign of zero, subnormals and
    infinities must match exactly."""
    a = np.ascontiguousarray(a, np.float32); b = np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape:
        return False
    return bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


def first_difference(a, b):
    """index, bits of a, bits of b at the first place same_bits() objects to (for assertion messages)"""
    a = np.ascontiguousarray(a, np.float32); b = np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape:
        return ("shape", a.shape, b.shape)
    bad = np.flatnonzero((a.view(np.uint32) != b.view(np.uint32)) & ~(np.isnan(a) & np.isnan(b)))
    if bad.size == 0:
        return None
    i = int(bad[0])
    return (i, hex(int(a.view(np.uint32)[i])), hex(int(b.view(np.uint32)[i])), int(bad.size))


def subnormal_count(y) -> int:
    """number of non-zero subnormal float32 values in y"""
    u = np.ascontiguousarray(y, np.float32).view(np.uint32)
    return int(np.count_nonzero(((u & 0x7F800000) == 0) & ((u & 0x007FFFFF) != 0)))


def ulp_diff(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """distance in float32 ulps (equal values, zeros of either sign included, and equal infinities: 0; NaN or unequal
    infinities: huge)"""
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    ia = a.view(np.int32).astype(np.int64)
    ib = b.view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia)
    ib = np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    d = np.abs(ia - ib)
    d = np.where(a == b, 0, d)
    d = np.where(np.isinf(a) | np.isinf(b), np.where(a == b, 0, 1 << 40), d)
    d = np.where(np.isnan(a) | np.isnan(b), 1 << 40, d)
    return d


def _f32(u) -> np.ndarray:
    return np.ascontiguousarray(u, np.uint32).view(np.float32)


def uniform_pm1(n: int, seed: int) -> np.ndarray:
    """n float32 uniform in [-1, 1], multiples of 2^-15 (exact)"""
    return (synth.noise_iq((n + 1) // 2, seed, 32767)[:n].astype(np.float32) / np.float32(32768.0)).astype(np.float32)


def subnormals(n: int, seed: int, scale_ulps: int) -> np.ndarray:
    """n float32 of either sign, |x| = k * 2^-149 with k uniform in [0, scale_ulps]; scale_ulps < 2^23 keeps every one
    of them subnormal.  Built from bit patterns: no arithmetic that a flush-to-zero mode could touch."""
    assert 0 < scale_ulps < (1 << 23)
    u = synth.lcg_u32(2 * n, seed)
    return _f32((u[:n] % np.uint32(scale_ulps + 1)) | ((u[n:] & np.uint32(1)) << np.uint32(31)))


# ------------------------------------------------------------------------------------------------ float decimators
FD_CASES = [(0, FC_CEN), (1, FC_INF), (1, FC_SUP), (3, FC_CEN), (6, FC_INF), (6, FC_CEN)]
FD_BLOCKS = (2 * 9000 + 6, 2 * 4100)          # floats per call: a dropped tail, carried state, more than one sub-chunk
FD_N = sum(FD_BLOCKS)
FD_GOLDEN_CASES = [(0, FC_CEN), (1, FC_CEN), (6, FC_CEN), (1, FC_INF)]       # tests/golden/fdecim_edges_golden.npz
FD_SUBNORMAL_ULPS = 713623                     # 1e-39 / 2^-149

# the values no int32 holds once multiplied by 32768 (and NaN); each is written into one float of the stream
FD_SPECIALS = _f32([0x4788B800, 0xC788B800,    # +-7e4
                    0x49742400, 0xC9742400,    # +-1e6
                    0x7F61B1E6, 0xFF61B1E6,    # +-3e38
                    0x7F800000, 0xFF800000,    # +-inf
                    0x7FC00000])               # NaN
FD_SPECIAL_AT = [2 * (311 + 331 * i) + (i & 1) for i in range(len(FD_SPECIALS))]     # float index: >= 300 samples apart, I and Q in turn


def fd_blocks(x):
    out, p = [], 0
    for n in FD_BLOCKS:
        out.append(x[p: p + n]); p += n
    return out


def fd_wrap(seed: int = 31) -> np.ndarray:
    """uniform in +-3.99: times 32768 stays inside int32, the low 16 bits wrap"""
    return (synth.noise_iq(FD_N // 2, seed, 32686).astype(np.float32) / np.float32(8192.0)).astype(np.float32)


def fd_overflow(seed: int = 32) -> np.ndarray:
    """|x| < 0.5: a constant, tones at +-fs/4 (so the band that every (log2, fcpos) keeps holds signal) and a little noise,
    with the isolated FD_SPECIALS at FD_SPECIAL_AT, all in the first quarter: the half-band histories (62 * 63 input samples
    at log2 = 6) have flushed long before the last quarter, where every output is non-zero again."""
    n = FD_N // 2
    t = synth.tone_iq(n, 500, 4) + synth.tone_iq(n, 500, 12)
    v = synth.noise_iq(n, seed, 50).astype(np.int64)
    v[0::2] += t[0::2] - t[1::2] // 2 + 600          # the tones turned by atan(1/2): off the axes after any quarter turn of the
    v[1::2] += t[1::2] + t[0::2] // 2 - 250          # _inf / _sup front ends, so neither component of an output sits at 0
    x = (v.astype(np.float32) / np.float32(4096.0)).astype(np.float32)
    assert FD_SPECIAL_AT[-1] < FD_N // 4
    x[FD_SPECIAL_AT] = FD_SPECIALS
    return x


def fd_subnormal(seed: int = 33) -> np.ndarray:
    """uniform +-1e-39: every input, every partial sum and nearly every output is subnormal"""
    return subnormals(FD_N, seed, FD_SUBNORMAL_ULPS)


def fd_signed_zero(seed: int = 34) -> np.ndarray:
    """a block of -0.0, then pairs of samples (a, b), (-a, -b): the sums of the filters and of the _inf / _sup front ends
    cancel to zeros of both signs"""
    x = np.zeros(FD_N, np.float32)
    g = FD_N // 4
    v = uniform_pm1(2 * g, seed)
    x[0: 4 * g: 4] = v[0::2]; x[1: 4 * g: 4] = v[1::2]; x[2: 4 * g: 4] = -v[0::2]; x[3: 4 * g: 4] = -v[1::2]
    x[: 2 * 3000] = -0.0
    x[2 * 8000: 2 * 8400] = 0.0
    return x


FD_INPUTS = {"wrap": fd_wrap, "overflow": fd_overflow, "subnormal": fd_subnormal, "signed_zero": fd_signed_zero}
FD_KIND_INPUTS = {"fi": ("wrap", "overflow"), "ff": ("wrap", "overflow", "subnormal", "signed_zero")}


# ------------------------------------------------------------------------------------------------ I/Q imbalance
IQ_N = 6000
IQ_GAP = (1500, 4000)
IQ_SETTLED = IQ_GAP[1] + 200                   # "stuck" / "recovers" is judged from here on
IQ_CUTS = [0, 63, 63 + 64, 63 + 64 + 65, 2500, IQ_N]      # the kernel moves 64 samples at a time; 2500 lies inside the gap
IQ_STUCK_SEED, IQ_RECOVER_SEED = 100, 101      # chosen on the oracle, asserted by tests/test_float_edges.py


def iq_gap_stream(seed: int, both: bool = False) -> np.ndarray:
    """amplitude 20000 noise, Q (or I and Q) exactly 0 over IQ_GAP: the float moving totals come out of the gap as a small
    residue of either sign"""
    x = synth.noise_iq(IQ_N, seed, 20000)
    x[2 * IQ_GAP[0] + 1: 2 * IQ_GAP[1]: 2] = 0
    if both:
        x[2 * IQ_GAP[0]: 2 * IQ_GAP[1]: 2] = 0
    return x


def iq_streams():
    """name -> int16 I/Q of the six streams that share one handle"""
    n = IQ_N
    const = np.empty(2 * n, np.int16); const[0::2] = 1234; const[1::2] = -567          # x becomes exactly 0 after 1024 samples
    full = np.empty(2 * n, np.int16)                                                    # I at full scale, Q a seventh of it:
    full[0::2] = np.where(synth.lcg_u32(n, 77) & 1, 32767, -32767)                      # the amplitude correction pushes Q
    full[1::2] = synth.noise_iq(n // 2 + 1, 78, 8000)[:n]                               # past +-32767 (the low 16 bits wrap)
    return {"stuck": iq_gap_stream(IQ_STUCK_SEED), "recovers": iq_gap_stream(IQ_RECOVER_SEED), "gap_both": iq_gap_stream(105, both=True),
            "constant": const, "full_scale": full, "control": synth.mix(n, 106, 12000, 6000, 1)}


def iq_feeds(x):
    return [x[2 * a: 2 * b] for a, b in zip(IQ_CUTS[:-1], IQ_CUTS[1:])]


# ------------------------------------------------------------------------------------------------ IIR bank
IIR_PARTS = (200, 3000, 200)                   # signal, silence, signal
IIR_CUT = 200 + 2600                           # inside the subnormal stretch
IIR_UNSTABLE = (2, [1.0, 2.5, -1.0], [0.5, 0.25, 0.125])     # poles at 2 and 0.5: overflows to inf, then inf - inf


def iir_input(seed: int) -> np.ndarray:
    a, z, b = IIR_PARTS
    x = np.zeros(a + z + b, np.float32)
    x[:a] = uniform_pm1(a, seed) * np.float32(1024.0)
    x[a + z:] = uniform_pm1(b, seed + 1000) * np.float32(1024.0)
    return x


# ------------------------------------------------------------------------------------------------ FIR bank
FIR_SPECS = [(0, 301, 48000.0, 250.0, 0.0), (1, 301, 48000.0, 300.0, 3000.0), (0, 64, 48000.0, 3000.0, 0.0), (1, 21, 8000.0, 300.0, 2500.0)]
FIR_N = 1500
FIR_FEEDS = (0, 700, 701, FIR_N)
# input scale per spec in units of 2^-149: 1e-38 (7136238), halved until at least half of the oracle's outputs are subnormal
# (the band pass of spec 1 is normalised by its tiny sum of taps, so its gain is large); tests/test_float_edges.py asserts it
FIR_SUBNORMAL_ULPS = (7136238, 111503, 7136238, 7136238)


def fir_subnormal(c: int, seed: int = 50) -> np.ndarray:
    return subnormals(FIR_N, seed + c, FIR_SUBNORMAL_ULPS[c])


def fir_huge(seed: int = 60) -> np.ndarray:
    """+-3e38: the pair sums overflow to +-inf, the accumulator then meets inf - inf"""
    u = synth.lcg_u32(FIR_N, seed)
    return _f32(np.uint32(0x7F61B1E6) | ((u & np.uint32(1)) << np.uint32(31)))


def fir_signed_zero(seed: int = 61) -> np.ndarray:
    """signal, a block of -0.0, a block of +0.0, then x, -x pairs"""
    x = uniform_pm1(FIR_N, seed)
    x[1::2] = -x[0::2]
    x[:400] = uniform_pm1(400, seed + 1)
    x[400:800] = -0.0
    x[800:1100] = 0.0
    return x


# ------------------------------------------------------------------------------------------------ silence after signal
def with_gap(head, gap_cplx: int, tail) -> np.ndarray:
    """interleaved complex streams: head, gap_cplx samples of exact zeros, tail"""
    head = np.ascontiguousarray(head); tail = np.ascontiguousarray(tail)
    return np.concatenate([head, np.zeros(2 * gap_cplx, head.dtype), tail])


def ragged(x, cuts_cplx):
    c = [0] + list(cuts_cplx) + [x.size // 2]
    return [x[2 * a: 2 * b] for a, b in zip(c[:-1], c[1:])]


AT_BURST, AT_GAP, AT_GAP_LONG = 9000, 8000, 14000      # the gap outlasts every agc_nb_samples in use (12288: the long one)
BE_PART = 6000                                          # back-end: signal, zeros, signal
BE_CUTS = (5000, 11001)                                 # three feeds, none aligned to the parts
BE_SEEDS = (800, 806)                                   # data seeds of the discri = 2 channels, see test_float_edges.py


def be_input(seed: int) -> np.ndarray:
    return with_gap(synth.mix(BE_PART, seed, 12000, 6000, 1), BE_PART, synth.mix(BE_PART, seed + 1, 12000, 6000, 2))
