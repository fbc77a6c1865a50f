"""GPU parity of the float kernels on the inputs of tests/float_edge_cases.py: float -> integer conversions outside the int32
range, silence after signal in the per-stream recurrences, subnormals, signed zeros, inf and NaN.  tests/test_float_edges.py
shows on the CPU that the committed inputs do reach those regimes, and pins the oracle to the compiled reference on them.
Bar: bit-identical to the oracle (floats through same_bits: a NaN for a NaN, everything else bit for bit), except the atan2
discriminator, which keeps the <= 3 ulp bound of include/sdrx.h.  profiles/r12_pytest_gpu.txt records which of these fail
with a plain (int) in the DecimatorsFI store and which with a library built to flush subnormals."""
import os

import numpy as np
import pytest

import sdrangel_amd as sa
from tests import float_edge_cases as fe
from tests import oracle_py as orc
from tests.test_audiotail_gpu import IIR_SPECS, NFM, SSB, cfg_struct
from tests.test_float_edges import audiotail_input, backend_channels, backend_oracle, fd_oracle

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fdecim_edges_golden.npz")


# ------------------------------------------------------------------------------------------------ float decimators
@pytest.fixture(scope="module")
def fd_inputs():
    return {name: make() for name, make in fe.FD_INPUTS.items()}


@pytest.mark.parametrize("L,fc", fe.FD_CASES)
@pytest.mark.parametrize("kind", ("fi", "ff"))
def test_float_decimators_edge_inputs(fd_inputs, kind, L, fc):
    golden = np.load(GOLDEN)
    for name in fe.FD_KIND_INPUTS[kind]:
        x = fd_inputs[name]
        g = sa.FloatDecimators(kind, L, fc)
        got = np.concatenate([g.decimate(b) for b in fe.fd_blocks(x)])
        want = fd_oracle(kind, L, fc, x)
        if kind == "fi":
            bad = np.flatnonzero(got != want) if got.size == want.size else None
            assert got.size == want.size and bad.size == 0, (name, got.size, want.size, bad[:5], got[bad[:5]], want[bad[:5]])
            key = f"fi_{name}_L{L}_fc{fc}"
            if (L, fc) in fe.FD_GOLDEN_CASES:
                assert np.array_equal(got, golden[key]), (name, "differs from the recorded reference")
        else:
            assert fe.same_bits(got, want), (name, fe.first_difference(got, want))


# ------------------------------------------------------------------------------------------------ I/Q imbalance
def test_iq_imbalance_gaps_constant_and_full_scale():
    xs = fe.iq_streams()
    names = list(xs)
    g = sa.IqImbalance(len(names))
    oras = [orc.IqImb() for _ in names]
    for a, b in zip(fe.IQ_CUTS[:-1], fe.IQ_CUTS[1:]):
        segs = [xs[k][2 * a: 2 * b] for k in names]
        got = g.process(segs)
        for c, k in enumerate(names):
            want = oras[c].process(segs[c])
            bad = np.flatnonzero(got[c] != want)
            assert bad.size == 0, (k, a, b, bad.size, a + bad[:4] // 2, got[c][bad[:4]], want[bad[:4]])
    g.reset()
    again = g.process([xs[k][: 2 * 1000] for k in names])
    for c, k in enumerate(names):
        assert np.array_equal(again[c], orc.IqImb().process(xs[k][: 2 * 1000])), k


# ------------------------------------------------------------------------------------------------ IIR bank
def test_iir_bank_through_subnormals_inf_and_nan():
    specs = IIR_SPECS * 13 + [fe.IIR_UNSTABLE]                # 66 channels: more than one wave
    xs = [fe.iir_input(70 + c % len(IIR_SPECS)) for c in range(len(specs) - 1)] + [fe.iir_input(99)]
    g = sa.IirBank(specs)
    oras = [orc.Iir(*s) for s in specs]
    subnormal = 0
    for a, b in ((0, fe.IIR_CUT), (fe.IIR_CUT, xs[0].size)):
        got = g.feed([x[a:b] for x in xs])
        for c in range(len(specs)):
            want = oras[c].run(xs[c][a:b])
            assert fe.same_bits(got[c], want), (c, a, b, fe.first_difference(got[c], want))
            subnormal += fe.subnormal_count(got[c])
    assert subnormal >= 13 * 3 * 1000                         # what the device itself emitted


# ------------------------------------------------------------------------------------------------ FIR bank
@pytest.mark.parametrize("name", ("subnormal", "huge", "signed_zero"))
def test_fir_bank_edge_inputs(name):
    n_ch = len(fe.FIR_SPECS)
    xs = [fe.fir_subnormal(c) if name == "subnormal" else fe.fir_huge() if name == "huge" else fe.fir_signed_zero() for c in range(n_ch)]
    bank = sa.FirBank([sa.FirCfg(k, n, r, a, b) for k, n, r, a, b in fe.FIR_SPECS])
    oras = [orc.Fir(*s) for s in fe.FIR_SPECS]
    for a, b in zip(fe.FIR_FEEDS[:-1], fe.FIR_FEEDS[1:]):
        got = bank.feed([x[a:b] for x in xs])
        for c in range(n_ch):
            want = oras[c].run(xs[c][a:b])
            assert fe.same_bits(got[c], want), (name, c, a, b, fe.first_difference(got[c], want))
            if name == "subnormal" and b - a > 1:
                assert fe.subnormal_count(got[c]) > 0


# ------------------------------------------------------------------------------------------------ audio tail
def test_audio_tails_across_a_gap_of_exact_zeros():
    cfgs = NFM + SSB
    xs, gaps = zip(*[audiotail_input(i, k) for i, k in enumerate(cfgs)])
    g = sa.AudioTail([cfg_struct(c) for c in cfgs])
    oras = [orc.AudioTailOracle(**c) for c in cfgs]
    outs = [[] for _ in cfgs]
    # ragged: one cut in the first burst, one inside the gap, one in the second burst (different per channel)
    cuts = [(0, 4000 + 7 * c, fe.AT_BURST + 1234 + c, fe.AT_BURST + gaps[c] + 3001, x.size // 2) for c, x in enumerate(xs)]
    for f in range(4):
        segs = [x[2 * cuts[c][f]: 2 * cuts[c][f + 1]] for c, x in enumerate(xs)]
        got = g.feed(segs)
        for c in range(len(cfgs)):
            want = oras[c].feed(segs[c])
            bad = np.flatnonzero(got[c] != want) if got[c].size == want.size else None
            assert got[c].size == want.size and bad.size == 0, (c, f, bad.size, cuts[c][f] + bad[:4], got[c][bad[:4]], want[bad[:4]])
            outs[c].append(got[c])
    for c in range(len(cfgs)):
        y = np.concatenate(outs[c])
        print(f"audio tail channel {c}: audio before the gap {bool(np.any(y[: fe.AT_BURST] != 0))}, "
              f"in it {int(np.count_nonzero(y[fe.AT_BURST: fe.AT_BURST + gaps[c]]))} samples, after it {bool(np.any(y[fe.AT_BURST + gaps[c]:] != 0))}")


# ------------------------------------------------------------------------------------------------ back-end
def test_backend_signal_silence_signal():
    chans = backend_channels()
    bank = sa.BackendBank([sa.BackendCfg(**cfg) for cfg, _ in chans])
    oras = [backend_oracle(cfg) for cfg, _ in chans]
    feeds = [fe.ragged(fe.be_input(seed), fe.BE_CUTS) for _, seed in chans]
    for f in range(len(fe.BE_CUTS) + 1):
        bank.feed([feeds[c][f] for c in range(len(chans))])
        for c, (cfg, seed) in enumerate(chans):
            want = oras[c].feed(feeds[c][f])
            got = bank.read(c)
            assert got.size == want.size, (c, f, got.size, want.size)
            d = fe.ulp_diff(got, want)
            worst = int(d.max()) if d.size else 0
            # discri = 2: std::arg -> atan2f of two math libraries on bit-identical arguments, <= 3 ulp apart (include/sdrx.h,
            # tests/test_backend_gpu.py); a wrong sign of zero in front of it shows as a jump of fm_scaling, far outside
            bound = 3 if cfg["discri"] == 2 else 0
            print(f"back-end channel {c} (discri {cfg['discri']}, nco {cfg['nco_freq']}, seed {seed}) feed {f}: max ulp distance {worst}")
            assert worst <= bound, (c, f, worst, int(np.argmax(d)), got[np.argmax(d)], want[np.argmax(d)])
            if cfg["discri"] != 2:
                assert fe.same_bits(got, want), (c, f, fe.first_difference(got, want))
