"""GPU: the float back-end, the audio tails, the FIR bank and the IIR bank at the limits their create calls accept
(tests/float_limit_cases.py), against the oracle that tests/test_float_limits.py pins to the compiled reference at the same
configurations.  Bar as in tests/test_backend_gpu.py: equal sizes and 0 ulp (every case has discri 0 or 1, so no atan2f);
qint16 audio bit-exact."""
import numpy as np
import pytest

import sdrangel_amd as sa
from tests import float_limit_cases as flc
from tests import oracle_py as orc
from tests import synth
from tests.test_audiotail_gpu import IIR_SPECS, cfg_struct
from tests.test_backend_gpu import mk, ulp_diff

pytestmark = pytest.mark.gpu


def run_backend_bank(cfgs, lengths, seeds):
    """one handle, channel c fed lengths[c] one after the other (channels with fewer feeds end with empty ones); after every
    feed every channel's output has the oracle's size and bits.  Returns the number of output floats per channel."""
    pairs = [mk(c) for c in cfgs]
    bank = sa.BackendBank([p[0] for p in pairs])
    for c, (_, o) in enumerate(pairs):
        nt, taps, _, inc = bank.design(c)
        ont, otaps = o.taps()
        assert nt == ont and np.array_equal(taps.view(np.uint32), otaps.view(np.uint32)), c
        assert inc == orc.lib().sdro_nco_inc(float(cfgs[c]["nco_freq"]), float(cfgs[c]["in_rate"])), c
    xs = [synth.noise_iq(sum(L), s, 20000) for L, s in zip(lengths, seeds)]
    pos = [0] * len(cfgs)
    total = [0] * len(cfgs)
    for f in range(max(len(L) for L in lengths)):
        segs = []
        for c, L in enumerate(lengths):
            n = L[f] if f < len(L) else 0
            segs.append(xs[c][2 * pos[c]: 2 * (pos[c] + n)]); pos[c] += n
        bank.feed(segs)
        for c, (_, o) in enumerate(pairs):
            want = o.feed(segs[c])
            got = bank.read(c)
            assert got.size == want.size, (c, f, got.size, want.size)
            assert ulp_diff(got, want) == 0, (c, f)
            total[c] += got.size
    bank.close()
    return total


@pytest.mark.parametrize("i", range(len(flc.BACKEND)))
def test_backend_corner_alone(i):
    """one design per handle, so every FIR tile is of one design: the tap table comes from LDS up to 80 taps per phase and
    from global memory above.  Channel 0 hands the resampler output out as it is; channel 1 has the same design, another NCO
    frequency and other data, and for three of the cases an fftfilt behind it.  The window case runs 17 such channels: a full
    tile of 16 columns keeps all four waves of a FIR workgroup busy, so a window that outgrew its 384 LDS slots would land in
    a neighbour's window while that one is in use."""
    k = flc.BACKEND[i]
    modes = flc.BE_MODES.get(i)
    n_ch = 17 if i == flc.WINDOW_CASE else 2
    cfgs = [flc.be_cfg(k)] + [flc.be_cfg(k, modes if c == 1 else None, nco_freq=-k["nco_freq"] - 321 * c) for c in range(1, n_ch)]
    lengths = [flc.be_feed_lengths(k, 100 * (c + 1) + i, modes if c == 1 else None) for c in range(n_ch)]
    total = run_backend_bank(cfgs, lengths, [300 + 100 * c + i for c in range(n_ch)])
    assert min(total) > 0, total
    if i == flc.WINDOW_CASE:
        wins = [flc.fir_windows(k, L) for L in lengths]
        print("window case: kmax - kmin + ntaps of the full tiles", sorted(set(sum(wins, []))))
        assert all(min(w) <= 384 < max(w) for w in wins)     # BE_FIR_XCAP: tiles on both sides of `win <= 384` in every channel


def test_backend_corners_in_one_handle():
    """all of them at once: FIR tiles of 16 columns straddle designs (global tap table, per-column tap counts), one
    schedule wave holds serial lanes with steps from 1.00002 to 2930 next to closed-form ones, and the fftfilt blocks of the
    three filtered channels fill over several feeds"""
    cfgs = [flc.be_cfg(k, flc.BE_MODES.get(i)) for i, k in enumerate(flc.BACKEND)]
    lengths = [flc.be_feed_lengths(k, 500 + i, flc.BE_MODES.get(i)) for i, k in enumerate(flc.BACKEND)]
    steps = [flc.be_step(k) for k in flc.BACKEND]
    assert min(steps) < 1.00003 and max(steps) > 2929
    for k, L in zip(flc.BACKEND, lengths):
        if k["q10"]:
            assert {700, 1024, 1025} <= set(int(v) for v in np.cumsum(L))
    wins = flc.fir_windows(flc.BACKEND[flc.WINDOW_CASE], lengths[flc.WINDOW_CASE])
    assert min(wins) <= 384 < max(wins)
    total = run_backend_bank(cfgs, lengths, [600 + i for i in range(len(cfgs))])
    assert min(total) > 0, total


def test_audio_tail_corners_two_workgroups():
    """the NFM and SSB corner configurations, repeated to 36 channels (two workgroups of 32 lanes, both kinds in each):
    the three ragged calls of the reference pin and an empty one, qint16 bit-exact; then reset() and a fresh start"""
    cfgs = flc.tail_cfgs()
    n_cfg = len(cfgs)
    order = list(range(n_cfg)) * 2 + [1, 7, 2, 8, 3, 9, 4, 10, 5, 11, 0, 6]
    assert len(order) > 32 and {cfgs[i]["kind"] for i in order[32:]} == {0, 1}
    g = sa.AudioTail([cfg_struct(cfgs[i]) for i in order])
    calls = list(flc.TAIL_CALLS[:2]) + [(40_000, 40_000)] + list(flc.TAIL_CALLS[2:])
    part = {0: 0, 1: 1, 3: 2}                                 # call -> entry of tail_expected
    for q, (a, b) in enumerate(calls):
        got = g.feed([flc.tail_input(i)[2 * a: 2 * b] for i in order])
        for c, i in enumerate(order):
            want = flc.tail_expected(i)[part[q]] if q in part else np.zeros(0, np.int16)
            assert got[c].size == want.size and np.array_equal(got[c], want), (c, i, a, b, int((got[c] != want).sum()))
    for i in range(n_cfg):
        nonzero = sum(int((y != 0).sum()) for y in flc.tail_expected(i))
        print("tail", i, "non-zero samples", nonzero)
        assert nonzero > 0, i                                 # the squelch opened, the AGC stepped up
    g.reset()
    again = g.feed([flc.tail_input(i)[: 2 * 6000] for i in order])
    fresh = [orc.AudioTailOracle(**k).feed(flc.tail_input(i)[: 2 * 6000]) for i, k in enumerate(cfgs)]
    for c, i in enumerate(order):
        assert np.array_equal(again[c], fresh[i]), (c, i)
    g.close()


def test_fir_bank_shortest_and_longest():
    """3, 4 (made 5), 4095 and 4096 (made 4097) taps, low pass and band pass: taps and outputs bit-identical over calls
    shorter than, equal to and longer than the history"""
    bank = sa.FirBank([sa.FirCfg(*s) for s in flc.FIR_SPECS])
    oras = [orc.Fir(*s) for s in flc.FIR_SPECS]
    for c, (o, s) in enumerate(zip(oras, flc.FIR_SPECS)):
        t = bank.taps(c)
        assert t.size == (s[1] | 1) // 2 + 1 and np.array_equal(t.view(np.uint32), o.taps().view(np.uint32)), c
    rng = np.random.default_rng(21)
    sizes = [flc.fir_calls(s[1]) for s in flc.FIR_SPECS]
    for q in range(len(sizes[0])):
        xs = [rng.standard_normal(sz[q]).astype(np.float32) for sz in sizes]
        got = bank.feed(xs)
        for c, o in enumerate(oras):
            want = o.run(xs[c])
            assert got[c].size == want.size and np.array_equal(got[c].view(np.uint32), want.view(np.uint32)), (c, q)
    bank.close()


def test_iir_orders_5_6_7_next_to_2_and_8():
    """the generic template at orders 5, 6 and 7 (only the oracle-to-reference pin ran them), next to orders 2 and 8, 70
    channels: more than one wave"""
    specs = ([IIR_SPECS[0]] + flc.iir_extra() + [IIR_SPECS[4], IIR_SPECS[1]] + flc.iir_extra()[::-1]) * 8
    specs = specs[:70]
    assert {s[0] for s in specs[64:]} >= {5, 6, 7}
    g = sa.IirBank(specs)
    os_ = [orc.Iir(*s) for s in specs]
    rng = np.random.default_rng(6)
    for n in (1, 0, 33, 5000):
        xs = [(rng.standard_normal(n) * 1000).astype(np.float32) for _ in specs]
        got = g.feed(xs)
        for c in range(len(specs)):
            want = os_[c].run(xs[c])
            assert np.isfinite(want).all(), c                # NaN payloads are not part of the bar
            assert got[c].size == want.size and np.array_equal(got[c].view(np.uint32), want.view(np.uint32)), (c, n)
    g.close()
