"""Configurations at the limits that the float back-end (sdrx_backend_*), the audio tails (sdrx_audiotail_*), the FIR bank
(sdrx_firbank_*) and the IIR bank (sdrx_iir_*) accept.  GPU-free: tests/test_float_limits.py pins the oracle to the compiled
reference at these, tests/test_float_limits_gpu.py runs the kernels against the oracle at the same ones.

What each back-end row is for (sdrangel_amd/csrc/backend_kernels.hpp):
  taps per phase  be_fir_kernel stages the tap table in LDS for ntaps <= BE_FIR_NT_MAX (80), reads it from global memory above;
                  be_fir_taps<*, true> walks four taps per step and finishes a count that is no multiple of 4 in a scalar loop;
                  256 taps make the input window start at history index 1
  nco_freq        be_mix_kernel's masked phase product with increments of +-2048, beyond +-4096 and below -2 * 4096
  ratio           the closed-form schedule with q = 10 (1024 start-up emissions), the input window on both sides of
                  BE_FIR_XCAP (384) in one launch, windows of 1000+ inputs, one schedule wave with steps from 1.00002 to 2930
"""
import functools

import numpy as np


def _be(nco_freq, in_rate, out_rate, cutoff, tpp, ntaps, nco_inc=None, q10=False):
    return dict(nco_freq=nco_freq, in_rate=in_rate, out_rate=out_rate, interp_cutoff=float(cutoff), taps_per_phase=float(tpp),
                ntaps=ntaps, nco_inc=nco_inc, q10=q10)


# (nco_freq, in_rate, out_rate, cutoff, taps_per_phase) -> taps per phase: (int)(tpp * 16), made even (interpolator.cpp)
BE_TAPS = [
    _be(-4567, 60000, 48000, 5000, 0.1, 2),
    _be(100, 60000, 48000, 5000, 0.4, 6),
    _be(100, 60000, 48000, 5000, 4.4, 70),
    _be(100, 60000, 48000, 5000, 5.0, 80),
    _be(100, 60000, 48000, 5000, 6.0, 96),
    _be(100, 120000, 48000, 5000, 16.0, 256),
]
# NCO::setFreq: (int)((freq * 4096) / rate) in float, truncated
BE_NCO = [
    _be(70000, 60000, 48000, 5000, 4.5, 72, nco_inc=4778),
    _be(-130000, 60000, 48000, 5000, 2.0, 32, nco_inc=-8874),
    _be(30000, 60000, 48000, 5000, 4.5, 72, nco_inc=2048),
    _be(-30000, 60000, 48000, 5000, 2.0, 32, nco_inc=-2048),
]
BE_RATIOS = [
    _be(-1234, 46125, 46080, 5000, 4.5, 72, q10=True),       # step 1 + 1/1024: closed form, q = 10
    _be(2345, 32800, 32768, 5000, 4.5, 72, q10=True),        # the same step from another pair of rates
    _be(-20000, 768000, 48000, 5000, 4.5, 72),               # ratio 16, q = 0
    _be(31000, 1137600, 48000, 5000, 4.5, 72),               # ratio 23.7, serial walk
    _be(-777, 48001, 48000, 5000, 4.5, 72),                  # step 1.00002, serial walk
    _be(888, 95999, 48000, 5000, 4.5, 72),                   # step 1.99998, serial walk
    _be(-9100, 238080, 48000, 5000, 4.5, 72),                # step 4.96: 64 outputs span 312 or 313 inputs, + 72 taps = 384 | 385
    _be(150000, 3000000, 1024, 300, 4.5, 72),                # step 2929.6875: closed form, q = 4
    _be(-150000, 2999999, 1024, 300, 4.5, 72),               # step 2929.6865: step * 1024 >= 2^20, so the serial walk takes it
]
BACKEND = BE_TAPS + BE_NCO + BE_RATIOS
WINDOW_CASE = BACKEND.index(BE_RATIOS[6])
# three channels pass their resampler output on: fftfilt (and a discriminator) behind a high ratio
BE_MODES = {
    BACKEND.index(BE_RATIOS[2]): dict(filt_mode=2, f1=300 / 48000, f2=3000 / 48000, discri=1, fm_scaling=24.0),
    BACKEND.index(BE_RATIOS[3]): dict(filt_mode=4, f1=0.0, f2=2 * 3000 / 48000, discri=0, fm_scaling=1.0),
    BACKEND.index(BE_RATIOS[6]): dict(filt_mode=1, f1=0.0, f2=0.1, discri=0, fm_scaling=1.0),
}
BE_PLAIN = dict(filt_mode=0, f1=0.0, f2=0.0, discri=0, fm_scaling=1.0)


def be_step(k):
    """(Real) inRate / (Real) outRate"""
    return float(np.float32(k["in_rate"]) / np.float32(k["out_rate"]))


def be_ref_len(k):
    """input length of the one-feed oracle-to-reference comparison"""
    return int(min(400000, max(30000, 40 * be_step(k))))


def be_cfg(k, modes=None, nco_freq=None):
    """keyword arguments of sdrangel_amd.BackendCfg"""
    d = {f: k[f] for f in ("in_rate", "nco_freq", "out_rate", "interp_cutoff", "taps_per_phase")}
    d.update(modes or BE_PLAIN)
    if nco_freq is not None:
        d["nco_freq"] = nco_freq
    return d


def be_feed_lengths(k, seed, modes=None):
    """ragged feed lengths of one channel: 0, 1, floor(step), floor(step) + 1, then to a total of max(6000, 200 * step)
    inputs (at most 300000) in four uneven pieces; a q = 10 channel is also cut at inputs 700, 1024 and 1025 (inside the
    1024-emission start-up of the closed form, at its last emission, one past it); a channel with an fftfilt gets
    at least one and a half blocks of resampler outputs, so that its output is not empty"""
    step = be_step(k)
    total = max(6000.0, 200 * step)
    if modes and modes["filt_mode"]:
        total = max(total, 1.5 * (1024 if modes["filt_mode"] >= 4 else 512) * step)
    total = int(min(300000, total))
    f = int(np.floor(step))
    head = [0, 1, f, f + 1]
    pos = sum(head)
    rng = np.random.default_rng(seed)
    cuts = {total} | {int(v) for v in rng.integers(pos + 1, total, size=3)}
    if k["q10"]:
        cuts |= {700, 1024, 1025}
    out = list(head)
    for c in sorted(cuts):
        out.append(c - pos); pos = c
    return out


def emission_inputs(k, lengths):
    """Interpolator::decimate's distance bookkeeping, input by input in float32 (interpolator.h:23-36 and the caller's
    `distance += step`): per feed, the index (within the feed) of the input that completes each output.  Used to prove
    which FIR tiles fall on which side of the window rule -- never as an expected output."""
    step = np.float32(k["in_rate"]) / np.float32(k["out_rate"])
    one, d, out = np.float32(1.0), np.float32(0.0), []
    for n in lengths:
        ks = []
        for i in range(n):
            d = np.float32(d - one)
            if d < one:
                ks.append(i); d = np.float32(d + step)
        out.append(np.asarray(ks, np.int64))
    return out


def fir_windows(k, lengths, tile=64):
    """kmax - kmin + ntaps of every tile of `tile` consecutive outputs of every feed (be_fir_kernel's `win`), full tiles only"""
    wins = []
    for ks in emission_inputs(k, lengths):
        for o in range(0, ks.size - tile + 1, tile):
            wins.append(int(ks[o + tile - 1] - ks[o]) + k["ntaps"])
    return wins


# ---------------------------------------------------------------- audio tails
# (audio_rate, squelch_gate, af_bandwidth); NFM_DL = 24000: the gate at and one past the delay line's length
NFM_TAILS = [(48000, 1, 3000.0), (48000, 24000, 3000.0), (48000, 24001, 3000.0), (44100, 441, 3000.0), (8000, 80, 3000.0), (24000, 240, 300.5)]
# (agc_nb_samples, threshold, threshold_enable, agc_gate, clamping); SSB_DL = 96000: 98304 and 96001 take the delay clamp,
# 2 and 3 give step length 1
SSB_TAILS = [(2, 1e5, 1, 0, 0), (3, 1e5, 1, 2, 1), (98304, 1e5, 1, 0, 0), (96000, 1e5, 1, 10, 1), (96001, 1e5, 1, 0, 0), (49152, 1e5, 1, 48, 0)]
TAIL_N = 260_000
TAIL_CALLS = ((0, 5), (5, 40_000), (40_000, TAIL_N))


def tail_cfgs():
    """keyword arguments of oracle_py.AudioTailOracle / fields of sdrangel_amd.AudioTailCfg"""
    nfm = [dict(kind=0, audio_rate=r, volume=2.0, fm_scaling=r / 10000, squelch_level=1e-6, squelch_gate=g, af_bandwidth=bw) for r, g, bw in NFM_TAILS]
    ssb = [dict(kind=1, audio_rate=48000, volume=2.0, agc_active=1, agc_nb_samples=n, agc_threshold=t, agc_threshold_enable=e, agc_gate=g, agc_clamping=c)
           for n, t, e, g, c in SSB_TAILS]
    return nfm + ssb


@functools.lru_cache(maxsize=None)
def tail_input(i):
    from tests.test_audiotail_gpu import bursts
    x = bursts(TAIL_N, 500 + i, period=15000 if i % 2 else 9000)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def tail_expected(i):
    """the oracle's qint16 audio of configuration i over TAIL_CALLS, one array per call; computed once per process"""
    from tests import oracle_py as orc
    o = orc.AudioTailOracle(**tail_cfgs()[i])
    x = tail_input(i)
    out = [o.feed(x[2 * a: 2 * b]).copy() for a, b in TAIL_CALLS]
    for y in out:
        y.setflags(write=False)
    return tuple(out)


# ---------------------------------------------------------------- FIR / IIR
FIR_SPECS = [(kind, nt, 48000.0, 300.0, 3000.0) for kind in (0, 1) for nt in (3, 4, 4095, 4096)]


def fir_calls(ntaps):
    return [1, 2, ntaps - 1, ntaps, ntaps + 1, 9000]


def iir_extra():
    """orders 5, 6, 7 with the coefficients tests/test_oracle_vs_ref.py::test_iir_filter_vs_reference_template draws"""
    rng = np.random.default_rng(12)
    return [(o, list(rng.uniform(-0.2, 0.2, o + 1)), [1.0] + list(rng.uniform(-0.3, 0.3, o))) for o in (5, 6, 7)]
