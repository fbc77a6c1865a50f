"""Chains of calls for the handles of the stream front end (decimators, DC and I/Q-imbalance correction, channelizer banks,
spectrum sink, audio tail): what tests/test_frontend_queued_gpu.py queues on the device without a synchronising call in
between, and what tests/test_frontend_chains.py checks on the oracle alone so that a chain cannot pass for the wrong reason.

GPU-free: numpy, tests/synth.py, tests/oracle_py.py and the case modules of the handles.  A chain is its configuration, its
inputs (tests/synth.py, fixed seeds), its spans and a function that runs the oracle over the same spans.  Every oracle used
here is pinned to the compiled reference by tests/test_oracle_vs_ref.py, tests/test_spectrum_golden.py and the golden suites.

A chain has ten rounds (the pipeline six).  Its first nine spans are SPANS(unit): short spans, an empty one, a one-element one
and one at least 4.5 times as long as any before it, where every power-of-two work buffer grows; the tenth is sized per handle
so that it produces enough outputs that depend on everything carried."""
import functools

import numpy as np

from tests import float_edge_cases as fe
from tests import oracle_py as orc
from tests import spectrum_cases as sc
from tests import synth

FC_INF, FC_SUP, FC_CEN = 0, 1, 2
#: the HEAD of tests/test_demod_queued_gpu.py
HEAD = (1300, 700, 0, 2000, 1, 900, 9000, 1100, 513)
BIG = 6
#: outputs the last span has to produce at the least, per channel or stream (the deepest bank channel: DEEP_OUT)
LAST_OUT, DEEP_OUT = 512, 64


def SPANS(unit, last):
    """ten span lengths: HEAD in parts of `unit` (the empty and the one-element span stay what they are), then `last`"""
    return [m if m <= 1 else unit * m for m in HEAD] + [int(last)]


def swapped(spans):
    """the same spans with the empty and the one-element one exchanged, so that they do not coincide in all streams"""
    s = list(spans)
    s[2], s[4] = s[4], s[2]
    return s


class Chain:
    """name, cfg, xs (one read-only array per stream), spans (per stream, in ELEMENTS of xs[s]; `per` elements make one unit of
    the entry point's count argument) and make(first) -> feed(r, segs): a fresh oracle in the configuration it has before
    round `first`, fed round by round; feed returns one array per stream (or channel)."""

    def __init__(self, name, cfg, xs, spans, per, make, **extra):
        self.name, self.cfg, self.per, self.make = name, cfg, per, make
        self.xs = [np.ascontiguousarray(x) for x in xs]
        self.spans = [list(s) for s in spans]
        for x, s in zip(self.xs, self.spans):
            assert x.size >= sum(s), (name, x.size, sum(s))
            x.setflags(write=False)
        self.rounds = len(self.spans[0])
        assert all(len(s) == self.rounds for s in self.spans)
        self.offs = [np.concatenate(([0], np.cumsum(s))).tolist() for s in self.spans]
        self.__dict__.update(extra)

    def segs(self, r):
        return [x[o[r]: o[r + 1]] for x, o in zip(self.xs, self.offs)]

    def counts(self, r):
        return [s[r] // self.per for s in self.spans]

    def run(self, first=0):
        feed = self.make(first)
        return [feed(r, self.segs(r)) for r in range(first, self.rounds)]

    @functools.cached_property
    def want(self):
        """the oracle's outputs of every round of the chain, computed once"""
        res = self.run()
        for outs in res:
            for y in outs:
                y.setflags(write=False)
        return res

    def __repr__(self):
        return f"{self.name}: cfg={self.cfg} spans={self.spans}"


# ---------------------------------------------------------------- DC and I/Q imbalance correction
@functools.lru_cache(maxsize=None)
def chain_dccorr():
    """DC on both arms, noise, and a stretch at full scale across two span borders: re - avg wraps through int16"""
    spans = SPANS(8, 4096)
    n = sum(spans)
    x = synth.mix(n, 301, 20000, 3000, 1).astype(np.int64)
    x[0::2] += 1500; x[1::2] -= 900
    x = x.clip(-32768, 32767).astype(np.int16)
    x[2 * 9000: 2 * 31000: 2] = 32767; x[2 * 9000 + 1: 2 * 31000: 2] = -32768

    def make(first):
        o = orc.DcCorr()
        return lambda r, segs: [o.process(segs[0])]
    return Chain("dccorr", (), [x], [[2 * m for m in spans]], 2, make)


@functools.lru_cache(maxsize=None)
def chain_iqimb():
    """three streams in one handle: the stuck-after-a-gap, the constant and the control stream of tests/float_edge_cases.py"""
    spans = SPANS(8, 4096)
    n = sum(spans)
    base = fe.iq_streams()
    xs = [np.concatenate([base[k], synth.mix(n - fe.IQ_N, 310 + i, 12000, 6000, 1 + i)]) for i, k in enumerate(("stuck", "constant", "control"))]
    per_stream = [spans, swapped(spans), spans]

    def make(first):
        os_ = [orc.IqImb() for _ in xs]
        return lambda r, segs: [o.process(s) for o, s in zip(os_, segs)]
    return Chain("iqimb", (3,), xs, [[2 * m for m in s] for s in per_stream], 2, make)


# ---------------------------------------------------------------- integer decimators
def _ragged(spans):
    """int16 (or byte) counts that are no whole groups: the tail of every call is dropped, as the header says"""
    return [m if m <= 1 else m + 6 for m in spans]


def _decim_input(n_elems, bits, seed):
    n = (n_elems + 1) // 2
    if bits == 16:
        x = synth.noise_iq(n, seed, 32767)                 # full scale: chunks overflow the FAST kernel and are recomputed
        x[::9] = -32768
        return x[:n_elems]
    amp = (1 << (bits - 1)) - 1
    return synth.mix(n, seed, 2 * amp // 3, amp // 3, 1)[:n_elems]


DECIM_CASES = [(6, FC_CEN, 12), (4, FC_INF, 16), (1, FC_SUP, 8), (0, FC_CEN, 12)]


def _decim_last(log2):
    return 2 * ((LAST_OUT + 90) << log2) + 6


@functools.lru_cache(maxsize=None)
def chain_decim(log2, fcpos, bits):
    spans = _ragged(SPANS(8, _decim_last(log2)))
    x = _decim_input(sum(spans), bits, 320 + log2)

    def make(first):
        o = orc.Decim(log2, fcpos, bits)
        return lambda r, segs: [o.process(segs[0])]
    return Chain(f"decim_log{log2}_fc{fcpos}_b{bits}", (log2, fcpos, bits), [x], [spans], 1, make)


#: the variant that ran before the hand-over, and how many int16 it saw
LOAD_FROM, LOAD_PRE = (3, FC_INF, 12), 2 * 6000
HANDOVER = 4096                                            # samples a handle walks serially after sdrx_decim_load_stages


@functools.lru_cache(maxsize=None)
def chain_decim_after_load():
    """(6, CEN, 12) continuing on the stage states another variant left: the first spans add up to fewer than 4096 samples,
    so the serial hand-over runs across several queued calls before the parallel kernels take over inside the big span"""
    log2, fcpos, bits = 6, FC_CEN, 12
    spans = _ragged(SPANS(1, _decim_last(log2)))
    x = _decim_input(LOAD_PRE + sum(spans), bits, 331)
    pre, body = x[:LOAD_PRE], x[LOAD_PRE:]

    def make(first):
        if first:                                          # not the chain's own start: a plain fresh object
            o = orc.Decim(log2, fcpos, bits)
        else:
            o = orc.Decim(*LOAD_FROM)
            o.process(pre)
            orc.lib().sdro_decim_switch(o.h, log2, fcpos); o.log2 = log2
        return lambda r, segs: [o.process(segs[0])]
    return Chain("decim_after_load_stages", (log2, fcpos, bits), [body], [spans], 1, make, pre=pre)


@functools.lru_cache(maxsize=None)
def chain_decim_u8():
    log2, fcpos, shift = 5, FC_INF, 127
    spans = _ragged(SPANS(8, _decim_last(log2)))
    x = (synth.lcg_u32(sum(spans), 340) & 0xff).astype(np.uint8)

    def make(first):
        o = orc.DecimU(log2, fcpos, shift)
        return lambda r, segs: [o.process(segs[0])]
    return Chain("decim_u8", (log2, fcpos, shift), [x], [spans], 1, make)


BATCH = 4


@functools.lru_cache(maxsize=None)
def chain_decim_batch():
    """four handles in one launch per round; in every round the lengths differ per handle and one of them is empty"""
    log2, fcpos, bits = 6, FC_CEN, 12
    base = SPANS(8, 3 * _decim_last(log2))
    per = [[0 if i == r % BATCH else max(base[r], 9) // (1 + (i + r) % 3) + 2 * i for r in range(len(base))] for i in range(BATCH)]
    xs = [_decim_input(sum(s), bits, 350 + i) for i, s in enumerate(per)]

    def make(first):
        os_ = [orc.Decim(log2, fcpos, bits) for _ in xs]
        return lambda r, segs: [o.process(s) for o, s in zip(os_, segs)]
    return Chain("decim_batch", (log2, fcpos, bits), xs, per, 1, make)


# ---------------------------------------------------------------- float decimators
FDECIM_CASES = [("ff", 6, FC_CEN, 16), ("fi", 3, FC_INF, 16), ("if", 6, FC_SUP, 12)]


@functools.lru_cache(maxsize=None)
def chain_fdecim(kind, log2, fcpos, bits):
    spans = _ragged(SPANS(8, _decim_last(log2)))
    n = (sum(spans) + 1) // 2
    x = (synth.mix(n, 360 + log2, 1300, 700, 1) if kind == "if" else synth.fdecim_input(kind, n, 360 + log2))[: sum(spans)]

    def make(first):
        o = orc.FDecim(kind, log2, fcpos, bits)
        return lambda r, segs: [o.process(segs[0])]
    return Chain(f"fdecim_{kind}_log{log2}_fc{fcpos}", (kind, log2, fcpos, bits), [x], [spans], 1, make)


# ---------------------------------------------------------------- 24-bit decimator
DECIM24_CASES = [(6, FC_CEN, 16), (3, FC_INF, 12)]


@functools.lru_cache(maxsize=None)
def chain_decim24(log2, fcpos, bits):
    """the device call takes any number of samples and carries the phase, so the oracle sees the stream from round `first` on
    in one piece (padded to whole groups: the filters are causal) and its outputs are dealt out by the sample count"""
    spans = [m if m <= 1 else m + 3 for m in SPANS(8, ((LAST_OUT + 90) << log2) + 3)]
    x = _decim_input(2 * sum(spans), bits, 370 + log2)
    offs = np.concatenate(([0], np.cumsum(spans))).tolist()

    def make(first):
        body = x[2 * offs[first]:]
        y = orc.Decim24(log2, fcpos, bits).process(np.concatenate([body, np.zeros(-body.size % 2048, np.int16)]))
        t0 = offs[first]

        def feed(r, segs):
            a, b = (offs[r] - t0) >> log2, (offs[r + 1] - t0) >> log2
            return [y[2 * a: 2 * b]]
        return feed
    return Chain(f"decim24_log{log2}_fc{fcpos}_b{bits}", (log2, fcpos, bits), [x], [[2 * m for m in spans]], 2, make)


# ---------------------------------------------------------------- channelizer bank
FS = 2_400_000
QUEUE0 = 16384                                             # initial queue size of a channel in sdrx_chan.hip, samples


def bank_input(n, seed):
    x = synth.noise_iq(n, seed, 32767)
    x[::9] = -32768
    return x


class BankModel:
    """oracle chains and Python queues, as in tests/test_bank_fuzz_gpu.py"""

    def __init__(self, cfgs):
        self.ch = []
        for rate, fc in cfgs:
            self.add(rate, fc)

    def add(self, rate, fc):
        self.ch.append({"q": np.zeros(0, np.int16)})
        self.configure(len(self.ch) - 1, rate, fc)

    def configure(self, c, rate, fc):
        modes, out_rate, ofs = orc.chan_plan(FS, rate, fc)
        self.ch[c].update(modes=modes, out_rate=out_rate, ofs=ofs, chain=orc.Chain(modes) if len(modes) else None)

    def feed(self, seg):
        outs = []
        for ch in self.ch:
            y = ch["chain"].feed(seg) if ch["chain"] is not None else seg.copy()
            ch["q"] = np.concatenate([ch["q"], y])
            outs.append(y)
        return outs

    def skip(self, c, n=-1):
        q = self.ch[c]["q"]
        self.ch[c]["q"] = q[2 * n:] if 0 <= n < q.size // 2 else q[:0]

    def apply(self, op):
        getattr(self, op[0])(*op[1:])


def _bank_chain(name, cfgs, unit, last, seed, ops=()):
    """ops: (round, when, method of BankModel, arguments), when = "before" or "after" that round's feed.  A run that starts at
    round `first` applies the configuration changes that came before it, not the skips."""
    spans = SPANS(unit, last)
    x = bank_input(sum(spans), seed)

    def make(first):
        m = BankModel(cfgs)
        for r, when, *op in ops:
            if (r < first or (r == first and when == "before" and first)) and op[0] in ("configure", "add"):
                m.apply(op)

        def feed(r, segs):
            for rr, when, *op in ops:
                if rr == r and when == "before" and not (first and r == first):
                    m.apply(op)
            outs = m.feed(segs[0])
            for rr, when, *op in ops:
                if rr == r and when == "after":
                    m.apply(op)
            feed.model = m
            return outs
        feed.model = m
        return feed
    return Chain(name, tuple(cfgs), [x], [[2 * m for m in spans]], 2, make, ops=tuple(ops))


@functools.lru_cache(maxsize=None)
def bank_model(chain):
    """the model after the whole chain: what is left in every queue"""
    feed = chain.make(0)
    for r in range(chain.rounds):
        feed(r, chain.segs(r))
    return feed.model


#: pass-through, 1, 3, 5, 8 and 11 stages (each request is the centre and width of its mode string, see band_of); channels 4
#: and 5 share seven stages, channels 2 and 3 three
BANK_STAGES = (0, 1, 3, 5, 8, 11)
BANK_CFGS = ((FS, 0), (1_200_000, 600_000), (300_000, 450_000), (75_000, 487_500), (9_375, -703_125), (1_171, -701_953))


@functools.lru_cache(maxsize=None)
def chain_bank():
    return _bank_chain("bank", BANK_CFGS, 16, (DEEP_OUT + 8) << 11, 380)


@functools.lru_cache(maxsize=None)
def chain_bank_reconf():
    """three channels in one group; before feed 3 one is reconfigured and one added, each into a group of its own: eight
    queued feeds with three groups take 24 slots of the ring of 4 pinned tables"""
    cfgs = BANK_CFGS[2:5]
    ops = ((2, "before", "configure", 1, 300_000, -300_000), (2, "before", "add", 37_500, 900_000))
    return _bank_chain("bank_reconfigure_add", cfgs, 8, (LAST_OUT + 8) << 8, 381, ops)


@functools.lru_cache(maxsize=None)
def chain_bank_skip():
    """a partial skip after feed 4 (the queue is compacted on the stream), a whole skip of another channel after feed 6"""
    cfgs = (BANK_CFGS[1], BANK_CFGS[3], BANK_CFGS[4])
    plain = _bank_chain("bank_skip_plain", cfgs, 8, (LAST_OUT + 8) << 8, 382)
    have = sum(plain.want[r][1].size // 2 for r in range(4))
    ops = ((3, "after", "skip", 1, have // 3), (5, "after", "skip", 0))
    return _bank_chain("bank_skip", cfgs, 8, (LAST_OUT + 8) << 8, 382, ops)


# ---------------------------------------------------------------- 24-bit bank
FS24 = 1 << 22
BANK24_STAGES = [0, 1, 6, 7, 12, 13]


def band_of(in_rate, modes):
    """(rate, fc) that DownChannelizer's bisection (downchannelizer.cpp:250-287) turns into this mode string"""
    lo, hi = -in_rate / 2.0, in_rate / 2.0
    for m in modes:
        mid = (lo + hi) / 2
        if m == 1: hi = mid
        elif m == 2: lo = mid
        else: lo, hi = lo + (hi - lo) / 4, hi - (hi - lo) / 4
    return in_rate >> len(modes), int(round((lo + hi) / 2))


@functools.lru_cache(maxsize=None)
def chain_bank24():
    """the plan of tests/test_wide24_gpu.py::test_bank24_mixed_depths"""
    rng = np.random.default_rng(5)
    plans = [band_of(FS24, rng.integers(0, 3, size=k)) for k in BANK24_STAGES]
    spans = SPANS(4, (DEEP_OUT + 8) << 13)
    x = synth.noise24(sum(spans), 390)
    modes = [orc.chan_plan(FS24, rate, fc)[0] for rate, fc in plans]

    def make(first):
        chains = [orc.Chain24(m) if len(m) else None for m in modes]
        return lambda r, segs: [c.feed(segs[0]) if c is not None else segs[0].copy() for c in chains]
    return Chain("bank24_mixed_depths", tuple(plans), [x], [[2 * m for m in spans]], 2, make, modes=modes)


# ---------------------------------------------------------------- spectrum sink
SPECTRUM_CASES = [(1024, 25, 3, sc.MOVING, sc.BH, 1), (256, 10, 5, sc.FIXED, 4, 0)]
SPECTRUM_QUEUE0 = 64 * 4096                                # initial frame queue of sdrx_spectrum.hip, floats


@functools.lru_cache(maxsize=None)
def spectrum_oracle():
    return sc.build_oracle()


@functools.lru_cache(maxsize=None)
def chain_spectrum(cfg, log2_double=False):
    """positive_only toggles per span; the last span is the largest and overflows the initial frame queue while frames of the
    earlier spans are still queued.  A round's output is its frames, (k, N) float32."""
    n = cfg[0]
    fresh = n - 2 * (n * cfg[1] // 100)
    spans = SPANS(2, fresh * (SPECTRUM_QUEUE0 // n if cfg[3] != sc.FIXED else 700))
    x = synth.mix(sum(spans), 400 + n, 20000, 9000, 3)

    def make(first):
        o = sc.OracleSpectrum(spectrum_oracle(), cfg, log2_double=log2_double)
        return lambda r, segs: [o.feed(segs[0], bool(r % 2))]
    return Chain(f"spectrum_n{n}", cfg, [x], [[2 * m for m in spans]], 2, make)


# ---------------------------------------------------------------- audio tail
@functools.lru_cache(maxsize=None)
def chain_audiotail():
    """the NFM + SSB configurations and the burst signal of tests/test_audiotail_gpu.py; spans in complex floats"""
    from tests import test_audiotail_gpu as at
    cfgs = at.NFM + at.SSB
    spans = SPANS(6, 6000)
    per = [swapped(spans) if c % 2 else spans for c in range(len(cfgs))]
    xs = [at.bursts(sum(s), 10 + c, period=15000 if c % 2 == 0 else 7000) for c, s in enumerate(per)]

    def make(first):
        os_ = [orc.AudioTailOracle(**c) for c in cfgs]
        return lambda r, segs: [o.feed(s).copy() for o, s in zip(os_, segs)]
    return Chain("audiotail", tuple(c["kind"] for c in cfgs), xs, [[2 * m for m in s] for s in per], 2, make, cfgs=cfgs)


# ---------------------------------------------------------------- one pipeline, in the order of DSPDeviceSourceEngine::work
PIPE_SPANS = (20_001, 33_000, 7, 41_003, 26_000, 48_000)
PIPE_FCS = (-900_000, -123_456, 0, 777_777)
PIPE_SPECTRUM = (1024, 0, 0, sc.NONE, sc.BH, 1)


def pipe_backend_cfg(out_rate, ofs):
    """the NFM front with the SSB filter and discriminator 1 of tests/test_backend_gpu.py::test_cfg4_pipeline_bank_to_backend_on_device"""
    return dict(in_rate=out_rate, nco_freq=-ofs, out_rate=48000, interp_cutoff=12500 / 2.2, taps_per_phase=4.5,
                filt_mode=2, f1=300 / 48000, f2=5000 / 48000, discri=1, fm_scaling=48000 / 2000)


@functools.lru_cache(maxsize=None)
def chain_pipeline():
    """DC correction -> spectrum of the corrected span -> bank -> back-end -> skip, six spans of a 2.4 MS/s stream with DC on
    it, four channels at 48000.  A round's output: [corrected span, spectrum frames, back-end output of channel 0 .. 3]."""
    x = synth.mix(sum(PIPE_SPANS), 410, 9000, 4000, 1).astype(np.int64)
    x[0::2] += 700; x[1::2] -= 400
    x = x.astype(np.int16)
    plans = [orc.chan_plan(FS, 48000, fc) for fc in PIPE_FCS]

    def make(first):
        dc = orc.DcCorr()
        sp = sc.OracleSpectrum(spectrum_oracle(), PIPE_SPECTRUM)
        chains = [orc.Chain(p[0]) for p in plans]
        bes = []
        for p in plans:
            k = pipe_backend_cfg(p[1], p[2])
            bes.append(orc.Backend(k["in_rate"], k["nco_freq"], k["out_rate"], k["interp_cutoff"], k["taps_per_phase"], k["filt_mode"], k["f1"], k["f2"], k["discri"], k["fm_scaling"]))

        def feed(r, segs):
            y = dc.process(segs[0])
            return [y, sp.feed(y, False)] + [be.feed(ch.feed(y)) for be, ch in zip(bes, chains)]
        return feed
    return Chain("pipeline", (PIPE_FCS, PIPE_SPECTRUM), [x], [[2 * m for m in PIPE_SPANS]], 2, make, plans=plans)


def all_chains():
    """every chain of tests/test_frontend_queued_gpu.py"""
    out = [chain_dccorr(), chain_iqimb()]
    out += [chain_decim(*c) for c in DECIM_CASES] + [chain_decim_after_load(), chain_decim_u8(), chain_decim_batch()]
    out += [chain_fdecim(*c) for c in FDECIM_CASES] + [chain_decim24(*c) for c in DECIM24_CASES]
    out += [chain_bank(), chain_bank_reconf(), chain_bank_skip(), chain_bank24()]
    out += [chain_spectrum(c) for c in SPECTRUM_CASES] + [chain_audiotail(), chain_pipeline()]
    return out
