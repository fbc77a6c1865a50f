"""GPU: the handles of the stream front end with their device calls queued back to back, the way bench.py times them.  Every
other test of these handles has a host-pointer call, a read, a sync or a torch.cuda.synchronize() between two calls; here the
chains of tests/frontend_chains.py (ten spans: short ones, an empty one, a one-element one, one that makes every work buffer
grow, and a last one whose outputs depend on everything carried) run without any call that synchronises between the first
and the last, so the double-buffered histories, the pinned per-call tables with their events, the growth of work buffers and
queues under earlier calls and the host-side bookkeeping are ten calls deep when the results are looked at.

  own     on the handle's own stream, every span in a device tensor of its own, uploaded and synchronised before the chain;
  caller  on a torch.cuda.Stream handed over with set_stream: every span is copied from pinned memory on that stream right
          before its call, every result is copied back on it after the chain.  Decimators24, ChannelizerBank24 and AudioTail
          have no set_stream and run `own` only.

After the last call: one sync, then every sample is compared bit for bit with the oracle over the same spans (float
decimators: float_edge_cases.same_bits; spectrum sink: the rule of tests/test_spectrum_gpu.py).  What the chains' shapes reach
is asserted on the oracle alone by tests/test_frontend_chains.py."""
import numpy as np
import pytest

import sdrangel_amd as sa
from tests import float_edge_cases as fe
from tests import frontend_chains as fc
from tests.test_spectrum_gpu import _compare

pytestmark = pytest.mark.gpu

WHERE = ("own", "caller")
ENGINES = ("mfma", "valu")


def caller_stream(where):
    import torch
    return torch.cuda.Stream() if where == "caller" else None


class Dev:
    """the spans of a chain on the device, one tensor each, and one output tensor per round and stream, all allocated before
    the chain starts"""

    def __init__(self, chain, stream, outputs=True):
        import torch
        self.torch, self.chain, self.stream = torch, chain, stream
        self.pinned, self.dev, self.out, self.back = [], [], [], []
        for r in range(chain.rounds):
            segs = chain.segs(r)
            if stream is None:
                self.dev.append([self._upload(s) for s in segs])
            else:
                self.pinned.append([torch.from_numpy(s.copy()).pin_memory() if s.size else None for s in segs])
                with torch.cuda.stream(stream):
                    self.dev.append([torch.zeros(s.size + 8, dtype=self._dtype(s), device="cuda") for s in segs])
            if outputs:
                with torch.cuda.stream(stream) if stream is not None else _null():
                    self.out.append([torch.zeros(w.size + 64, dtype=self._dtype(w), device="cuda") for w in chain.want[r]])
                if stream is not None:
                    self.back.append([torch.zeros(t.shape, dtype=t.dtype).pin_memory() for t in self.out[-1]])
        torch.cuda.synchronize()                            # once, before the first call: none of this is on the handle's stream

    def _dtype(self, a):
        return self.torch.from_numpy(np.zeros(1, a.dtype)).dtype

    def _upload(self, seg):
        t = self.torch.zeros(seg.size + 8, dtype=self._dtype(seg), device="cuda")
        if seg.size:
            t[: seg.size].copy_(self.torch.from_numpy(seg.copy()))
        return t

    def stage(self, r):
        """caller's stream: this round's spans come from pinned memory on that stream, right before the call"""
        if self.stream is None:
            return
        with self.torch.cuda.stream(self.stream):
            for d, p in zip(self.dev[r], self.pinned[r]):
                if p is not None:
                    d[: p.numel()].copy_(p, non_blocking=True)

    def ins(self, r):
        return [t.data_ptr() for t in self.dev[r]]

    def outs(self, r):
        return [t.data_ptr() for t in self.out[r]]

    def collect(self, sync):
        """after the last call: the results come back (on the caller's stream where there is one), one sync"""
        if self.stream is None:
            sync()
            return [[t.cpu().numpy() for t in row] for row in self.out]
        with self.torch.cuda.stream(self.stream):
            for row, hrow in zip(self.out, self.back):
                for t, h in zip(row, hrow):
                    h.copy_(t, non_blocking=True)
        sync()
        return [[h.numpy() for h in hrow] for hrow in self.back]


class _null:
    def __enter__(self): return self
    def __exit__(self, *a): return False


def same(got, want):
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    return fe.same_bits(got, want) if want.dtype == np.float32 else bool(np.array_equal(got, want))


def check_rounds(chain, got, where):
    """every output of every round; what lies behind an output in its tensor is still zero"""
    for r, (grow, wrow) in enumerate(zip(got, chain.want)):
        for s, (g, w) in enumerate(zip(grow, wrow)):
            what = f"{chain.name} ({where}): round {r}, stream {s}, spans {[sp[r] for sp in chain.spans]} of {chain!r}"
            assert same(g[: w.size], w), (what, int(np.count_nonzero(g[: w.size] != w)), fe.first_difference(g[: w.size], w) if w.dtype == np.float32 else None)
            assert not g[w.size:].any(), what + ": wrote behind its outputs"


def run_chain(chain, handle, call, where, stream):
    """the chain on one handle: call(r, in pointers, counts, out pointers) is the entry point under test"""
    if stream is not None:
        handle.set_stream(stream.cuda_stream)
    d = Dev(chain, stream)
    ret = []
    for r in range(chain.rounds):
        d.stage(r)
        ret.append(call(r, d.ins(r), chain.counts(r), d.outs(r)))
    got = d.collect(handle.sync)
    check_rounds(chain, got, where)
    return ret, d


# ---------------------------------------------------------------- DC and I/Q imbalance correction
@pytest.mark.parametrize("where", WHERE)
def test_dccorr_chain(where):
    c, h, stream = fc.chain_dccorr(), sa.DcCorrection(), caller_stream(where)
    run_chain(c, h, lambda r, i, n, o: h.process_dev(i[0], o[0], n[0]), where, stream)
    h.close()


@pytest.mark.parametrize("where", WHERE)
def test_iqimb_chain_in_is_not_out(where):
    c, stream = fc.chain_iqimb(), caller_stream(where)
    h = sa.IqImbalance(len(c.xs))
    run_chain(c, h, lambda r, i, n, o: h.process_dev(i, o, n), where, stream)
    h.close()


# ---------------------------------------------------------------- integer decimators
def check_decim(chain, ret, handle, engine):
    for r, n in enumerate(ret):
        assert [k * 2 for k in (n if isinstance(n, list) else [n])] == [w.size for w in chain.want[r]], (chain.name, r, n)
    kernel = handle.last_launch()["kernel"]
    if chain.cfg[0] == 0:
        assert kernel == "decim1_kernel", kernel               # decimate1 has no half-band: one kernel under either engine
    else:
        assert kernel.endswith("+mfma") == (engine == "mfma"), (engine, kernel)


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("log2,fcpos,bits", fc.DECIM_CASES)
def test_decim_chain(log2, fcpos, bits, engine, where, monkeypatch):
    monkeypatch.setenv("SDRX_DECIM_ENGINE", engine)
    c, stream = fc.chain_decim(log2, fcpos, bits), caller_stream(where)
    h = sa.Decimators(log2, fcpos, bits)
    ret, _ = run_chain(c, h, lambda r, i, n, o: h.decimate_dev(i[0], n[0], o[0]), where, stream)
    check_decim(c, ret, h, engine)
    h.close()


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("engine", ENGINES)
def test_decim_chain_right_after_load_stages(engine, where, monkeypatch):
    """the serial hand-over (the first 4096 samples after load_stages) runs across the first seven queued calls and ends
    inside the big span, where the parallel kernels take over"""
    monkeypatch.setenv("SDRX_DECIM_ENGINE", engine)
    c, stream = fc.chain_decim_after_load(), caller_stream(where)
    other, stages = sa.Decimators(*fc.LOAD_FROM), sa.DecimStages()
    other.decimate(c.pre)
    other.save_stages(stages)
    h = sa.Decimators(*c.cfg)
    if stream is not None:
        h.set_stream(stream.cuda_stream)
    h.load_stages(stages)
    ret, _ = run_chain(c, h, lambda r, i, n, o: h.decimate_dev(i[0], n[0], o[0]), where, stream)
    check_decim(c, ret, h, engine)
    h.close(); other.close(); stages.close()


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("engine", ENGINES)
def test_decim_u8_chain(engine, where, monkeypatch):
    monkeypatch.setenv("SDRX_DECIM_ENGINE", engine)
    c, stream = fc.chain_decim_u8(), caller_stream(where)
    h = sa.DecimatorsU(*c.cfg)
    ret, _ = run_chain(c, h, lambda r, i, n, o: h.decimate_dev(i[0], n[0], o[0]), where, stream)
    check_decim(c, ret, h, engine)
    h.close()


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("engine", ENGINES)
def test_decim_batch_chain(engine, where, monkeypatch):
    """four handles, one launch per round, ten rounds queued on handles[0]'s stream"""
    monkeypatch.setenv("SDRX_DECIM_ENGINE", engine)
    c, stream = fc.chain_decim_batch(), caller_stream(where)
    hs = [sa.Decimators(*c.cfg) for _ in c.xs]
    ret, _ = run_chain(c, hs[0], lambda r, i, n, o: sa.decimate_dev_batch(hs, i, n, o), where, stream)
    check_decim(c, ret, hs[0], engine)
    for h in hs:
        h.close()


# ---------------------------------------------------------------- float and 24-bit decimators
@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("kind,log2,fcpos,bits", fc.FDECIM_CASES)
def test_fdecim_chain(kind, log2, fcpos, bits, where):
    c, stream = fc.chain_fdecim(kind, log2, fcpos, bits), caller_stream(where)
    h = sa.FloatDecimators(kind, log2, fcpos, bits)
    ret, _ = run_chain(c, h, lambda r, i, n, o: h.decimate_dev(i[0], n[0], o[0]), where, stream)
    assert [2 * n for n in ret] == [w[0].size for w in c.want]
    h.close()


@pytest.mark.parametrize("log2,fcpos,bits", fc.DECIM24_CASES)
def test_decim24_chain(log2, fcpos, bits):
    c = fc.chain_decim24(log2, fcpos, bits)
    h = sa.Decimators24(log2, fcpos, bits)
    ret, _ = run_chain(c, h, lambda r, i, n, o: h.decimate_dev(i[0], n[0], o[0]), "own", None)
    assert [2 * n for n in ret] == [w[0].size for w in c.want]
    h.close()


# ---------------------------------------------------------------- channelizer bank
def bank_op(bank, op):
    kind, args = op[0], op[1:]
    if kind == "configure":
        bank.reconfigure(*args)
    elif kind == "add":
        bank.add_channel(*args)
    else:
        bank.skip(*args)


def run_bank(chain, engine, where):
    """feed_dev ten times, the chain's operations where it has them (skip inside the chain; reconfigure and add_channel
    before feed 3, not between two feeds of interest), then one sync and every queue against the model's"""
    stream = caller_stream(where)
    bank = sa.ChannelizerBank(fc.FS, [k[0] for k in chain.cfg], [k[1] for k in chain.cfg])
    if stream is not None:
        bank.set_stream(stream.cuda_stream)
    d = Dev(chain, stream, outputs=False)
    for r in range(chain.rounds):
        for rr, when, *op in chain.ops:
            if rr == r and when == "before":
                bank_op(bank, op)
        d.stage(r)
        bank.feed_dev(d.ins(r)[0], chain.counts(r)[0])
        for rr, when, *op in chain.ops:
            if rr == r and when == "after":
                bank_op(bank, op)
    bank.sync()
    model = fc.bank_model(chain)
    assert bank.last_launch()["kernel"] == f"tree_kernel<{engine}>"
    for ch, m in enumerate(model.ch):
        what = f"{chain.name} ({where}, {engine}): channel {ch} of {chain!r}"
        modes, rate, ofs = bank.info(ch)
        assert list(modes) == list(m["modes"]) and (rate, ofs) == (m["out_rate"], m["ofs"]), what
        assert bank.available(ch) == m["q"].size // 2, (what, bank.available(ch), m["q"].size // 2)
        got = bank.read(ch)
        assert got.size == m["q"].size and np.array_equal(got, m["q"]), (what, int(np.count_nonzero(got != m["q"])), int(np.flatnonzero(got != m["q"])[0]) // 2)
    bank.close()


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("engine", ENGINES)
def test_bank_chain(engine, where, monkeypatch):
    """pass-through, 1, 3, 5, 8 and 11 stages: the queues hold all ten feeds' outputs and grow while they hold samples"""
    monkeypatch.setenv("SDRX_CHAN_ENGINE", engine)
    run_bank(fc.chain_bank(), engine, where)


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("engine", ENGINES)
def test_bank_chain_three_groups_wrap_the_table_ring(engine, where, monkeypatch):
    """reconfigure and add_channel before feed 3, then eight queued feeds (one of them HEAD's empty span, which takes no
    table) with three groups alive: 21 group-feeds in flight on a ring of four pinned tables"""
    monkeypatch.setenv("SDRX_CHAN_ENGINE", engine)
    c = fc.chain_bank_reconf()
    run_bank(c, engine, where)


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("engine", ENGINES)
def test_bank_chain_with_skips_inside(engine, where, monkeypatch):
    monkeypatch.setenv("SDRX_CHAN_ENGINE", engine)
    run_bank(fc.chain_bank_skip(), engine, where)


def test_bank24_chain():
    """only the last feed's outputs exist (out_dev)"""
    c = fc.chain_bank24()
    bank = sa.ChannelizerBank24(fc.FS24, [k[0] for k in c.cfg], [k[1] for k in c.cfg])
    for ch, modes in enumerate(c.modes):
        assert list(bank.info(ch)[0]) == list(modes), ch
    d = Dev(c, None, outputs=False)
    for r in range(c.rounds):
        bank.feed_dev(d.ins(r)[0], c.counts(r)[0])
    bank.sync()
    for ch, want in enumerate(c.want[-1]):
        ptr, cnt = bank.out_dev(ch)
        assert ptr and 2 * cnt == want.size, (ch, cnt, want.size)
        out = np.empty(2 * cnt, np.int32)
        assert sa.lib().sdrx_chan24_bank_read(bank._h, ch, out.ctypes.data, cnt) == cnt
        assert np.array_equal(out, want), (c.name, ch, int(np.count_nonzero(out != want)), repr(c))
    bank.close()


# ---------------------------------------------------------------- spectrum sink
@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("cfg", fc.SPECTRUM_CASES, ids=lambda k: f"n{k[0]}")
def test_spectrum_chain(cfg, where):
    """positive_only toggles per span; all frames are read at the end, so the frame queue grows with frames in it"""
    c, c2, stream = fc.chain_spectrum(cfg), fc.chain_spectrum(cfg, log2_double=True), caller_stream(where)
    g = sa.SpectrumVis(*cfg)
    if stream is not None:
        g.set_stream(stream.cuda_stream)
    d = Dev(c, stream, outputs=False)
    for r in range(c.rounds):
        d.stage(r)
        g.feed_dev(d.dev[r][0][: c.spans[0][r]], bool(r % 2))
    g.sync()
    want = np.concatenate([w[0] for w in c.want])
    want2 = np.concatenate([w[0] for w in c2.want])
    assert g.available() == want.shape[0], (g.available(), [w[0].shape[0] for w in c.want])
    stats = [0, 0, 0, 0]
    _compare(g.read(), want, want2, cfg[5], f"{c.name} ({where}) of {c!r}", stats)
    assert g.available() == 0
    g.close()


# ---------------------------------------------------------------- audio tail
def test_audiotail_chain():
    c = fc.chain_audiotail()
    from tests.test_audiotail_gpu import cfg_struct
    h = sa.AudioTail([cfg_struct(k) for k in c.cfgs])
    run_chain(c, h, lambda r, i, n, o: h.feed_dev(i, n, o), "own", None)
    assert sum(int(np.count_nonzero(w)) for row in c.want for w in row) > 100_000     # squelches opened, AGCs passed audio
    h.close()


# ---------------------------------------------------------------- the pipeline
def test_pipeline_on_one_caller_stream():
    """DSPDeviceSourceEngine::work per span, all on one torch stream: the span comes from pinned memory, DC correction, the
    spectrum of the corrected span, the bank, the back-end taking the bank's queues on the device, skip.  Nothing is looked at
    before the end: the corrected spans, all spectrum frames and the back-end's outputs for the last span."""
    import torch
    from tests.test_backend_gpu import ulp_diff
    c = fc.chain_pipeline()
    stream = torch.cuda.Stream()
    dc, spec = sa.DcCorrection(), sa.SpectrumVis(*fc.PIPE_SPECTRUM)
    bank = sa.ChannelizerBank(fc.FS, [48000] * len(fc.PIPE_FCS), list(fc.PIPE_FCS))
    cfgs = []
    for ch, plan in enumerate(c.plans):
        modes, rate, ofs = bank.info(ch)
        assert list(modes) == list(plan[0]) and (rate, ofs) == plan[1:]
        cfgs.append(sa.BackendCfg(**fc.pipe_backend_cfg(rate, ofs)))
    be = sa.BackendBank(cfgs)
    for h in (dc, spec, bank):
        h.set_stream(stream.cuda_stream)
    d = Dev(c, stream, outputs=False)
    with torch.cuda.stream(stream):
        ys = [torch.zeros(c.spans[0][r] + 8, dtype=torch.int16, device="cuda") for r in range(c.rounds)]
        back = [torch.zeros(y.shape, dtype=y.dtype).pin_memory() for y in ys]
    torch.cuda.synchronize()
    for r in range(c.rounds):
        n = c.counts(r)[0]
        d.stage(r)
        dc.process_dev(d.ins(r)[0], ys[r].data_ptr(), n)
        spec.feed_dev(ys[r][: 2 * n], False)
        bank.feed_dev(ys[r].data_ptr(), n)
        be.feed_bank(bank)
        for ch in range(len(cfgs)):
            bank.skip(ch)
    with torch.cuda.stream(stream):
        for y, h in zip(ys, back):
            h.copy_(y, non_blocking=True)
    spec.sync()                                             # the caller's stream; the back-end's own stream is waited for by its read
    for r in range(c.rounds):
        want = c.want[r][0]
        assert np.array_equal(back[r].numpy()[: want.size], want), (r, repr(c))
    frames = np.concatenate([w[1] for w in c.want])
    assert spec.available() == frames.shape[0]
    _compare(spec.read(), frames, frames, True, "pipeline spectrum", [0, 0, 0, 0])
    produced = 0
    for ch in range(len(cfgs)):
        want = c.want[-1][2 + ch]
        got = be.read(ch)
        assert got.size == want.size and ulp_diff(got, want) == 0, (ch, got.size, want.size)
        assert bank.available(ch) == 0
        produced += got.size
    assert produced >= 4 * fc.LAST_OUT
    for h in (be, bank, spec, dc):
        h.close()
