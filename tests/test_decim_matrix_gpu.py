"""GPU: every instantiation of the integer decimator's kernels, each launched under its own name and compared bit for bit with the
CPU oracle: (log2 1..6) x (fcpos) x (input_bits 8 / 12 / 16) of Decimators and (log2) x (fcpos) of the unsigned 8-bit DecimatorsU, and
for each the five kernels of its ChainEntry (sdrangel_amd/csrc/sdrx_decim.hip): the EXACT kernel, and the FAST kernel on either
engine (valu, mfma) with one and with four waves per segment.

Two calls on one handle: the first spans three chunks of 4096 samples (three workgroups in every flavour: asserted), the second is
shorter than one chunk and starts from the first one's history; neither is a whole number of chunks.  The EXACT kernel gets full
scale for its bit depth; the FAST kernels get data inside their contract (no stage output leaves int16: the oracle's probe says so)
with SDRX_DECIM_PATH unset, and last_fallback() must report no flagged chunk, so what is compared is the named kernel's own output.
last_launch() must name the instantiation as the library spells it."""
import functools

import numpy as np
import pytest

import sdrangel_amd as sa
from tests import oracle_py as orc
from tests import synth

pytestmark = pytest.mark.gpu

CHUNK = 4096
N1 = 2 * CHUNK + 1800         # whole groups of it: 9984 (group 128 samples) .. 9992 -- three chunks, the last one partial
N2 = 1500                     # less than one chunk
FULL = {8: 127, 12: 2047, 16: 32767}
#: noise and tone amplitude of the FAST kernels' data: the stored int16 stages gain at most 3.49 each on (value << pre)
CONTRACT = {8: (96, 31), 12: (1400, 600), 16: (2400, 800)}
PRE12 = (4, 3, 2, 1, 0, 0, 0)

KERNELS = [("exact", None, None)] + [("fast", e, nw) for e in ("valu", "mfma") for nw in (1, 4)]
KERNEL_IDS = ["exact"] + [f"{e}-nw{nw}" for _, e, nw in KERNELS[1:]]
CONFIGS = [(False, log2, fc, bits) for bits in (8, 12, 16) for log2 in range(1, 7) for fc in (sa.FC_CEN, sa.FC_INF, sa.FC_SUP)] + \
          [(True, log2, fc, 8) for log2 in range(1, 7) for fc in (sa.FC_CEN, sa.FC_INF, sa.FC_SUP)]
CONFIG_IDS = [f"{'u8' if u8 else 'i' + str(bits)}-log2_{log2}-fc{fc}" for u8, log2, fc, bits in CONFIGS]


def pre_shift(u8, log2, bits):
    """decimation_shifts<16, bits>::pre of the reference, the kernels' PRE template argument"""
    return 8 - log2 if (u8 or bits == 8) else PRE12[log2] if bits == 12 else 0


def kernel_name(path, engine, nw, u8, log2, fc, bits):
    args = f"{log2},{fc},{pre_shift(u8, log2, bits)},{int(u8)}"
    if path == "exact":
        return f"decim_chain_kernel<{args}>"
    return f"decim_fast_kernel<{args},{nw}>" + ("+mfma" if engine == "mfma" else "")


@functools.lru_cache(maxsize=None)
def reference(u8, log2, fc, bits, full_scale):
    """[(call buffer, oracle outputs, probe bytes)]: the two calls, one oracle object across them, then the second buffer from fresh
    state; shared by the kernels of a config"""
    seed = 4000 + 100 * bits + 10 * log2 + fc + (50 if u8 else 0)
    n = N1 + N2
    if u8:
        x = (synth.lcg_u32(2 * n, seed) & 0xff).astype(np.uint8)
        x[2 * 700: 2 * 900] = 0; x[2 * 900: 2 * 1100] = 255                 # the byte range's ends, every kernel: DecimatorsU cannot flag
        x[2 * 9000: 2 * 9400: 2] = 0; x[2 * 9000 + 1: 2 * 9400: 2] = 255
        o = orc.DecimU(log2, fc, 127)
    elif full_scale:
        amp = FULL[bits]
        x = orc.synth_iq(n, seed=seed, amp=amp)
        x[2 * 700: 2 * 900] = -amp - 1; x[2 * 900: 2 * 1100] = amp          # runs of both extremes, and an alternating stretch across the calls' seam
        x[2 * 9800: 2 * 10200] = np.where(np.arange(800) % 4 < 2, amp, -amp - 1)
        o = orc.Decim(log2, fc, bits)
    else:
        amp, tone = CONTRACT[bits]
        x = orc.synth_iq(n, seed=seed, amp=amp, tone=(0.0019, tone))
        o = orc.Decim(log2, fc, bits)
    group = sa.lib().sdrx_decim_group_int16(log2, fc)
    cut = 2 * N1 // group * group                                            # the first call's ragged tail is dropped, as the reference drops it
    calls = [x[: 2 * N1], x[cut: cut + 2 * N2]]
    out = []
    for c in calls:
        want, _lo, _hi, bad = o.probe(c)
        out.append((c, want, bad))
    fresh = orc.DecimU(log2, fc, 127) if u8 else orc.Decim(log2, fc, bits)   # the short buffer again, as a stream of its own
    want, _lo, _hi, bad = fresh.probe(calls[1])
    out.append((calls[1], want, bad))
    return out


def pin(monkeypatch, path, engine, nw):
    for var in ("SDRX_DECIM_PATH", "SDRX_DECIM_ENGINE", "SDRX_DECIM_NW", "SDRX_DECIM_SPW", "SDRX_DECIM_CPS"):
        monkeypatch.delenv(var, raising=False)
    if path == "exact":
        monkeypatch.setenv("SDRX_DECIM_PATH", "exact")
    else:
        monkeypatch.setenv("SDRX_DECIM_ENGINE", engine)
        monkeypatch.setenv("SDRX_DECIM_NW", str(nw))


@pytest.mark.parametrize("path,engine,nw", KERNELS, ids=KERNEL_IDS)
@pytest.mark.parametrize("u8,log2,fc,bits", CONFIGS, ids=CONFIG_IDS)
def test_instantiation_alone(u8, log2, fc, bits, path, engine, nw, monkeypatch):
    pin(monkeypatch, path, engine, nw)
    ref = reference(u8, log2, fc, bits, path == "exact")
    name = kernel_name(path, engine, nw, u8, log2, fc, bits)
    g = sa.DecimatorsU(log2, fc, 127) if u8 else sa.Decimators(log2, fc, bits)
    for i, (x, want, bad) in enumerate(ref[:2]):
        assert x.size % (2 * CHUNK) and want.size, (i, x.size)
        got = g.decimate(x)
        assert got.size == want.size, (name, i, got.size, want.size)
        if not np.array_equal(got, want):
            d = np.nonzero(got != want)[0]
            raise AssertionError((name, "call", i, "first differing int16", int(d[0]), "of", int(d.size), "in", int(want.size)))
        ll = g.last_launch()
        assert ll["kernel"] == name, (ll, name)
        assert ll["block"] == (256 if path == "exact" or nw == 4 else 64), ll
        assert ll["grid"] >= 3 if i == 0 else ll["grid"] == 1, (name, i, ll)
        rep = g.last_fallback()
        if path == "exact":
            assert (rep["flagged"], rep["total"]) == (0, 0), (name, i, rep)
        else:
            assert not bad.any(), (name, i, "the data leave the FAST kernel's contract", np.nonzero(bad)[0].tolist())
            assert (rep["flagged"], rep["total"]) == (0, bad.size), (name, i, rep["flagged"], rep["total"], bad.size)
    g.close()


@pytest.mark.parametrize("path,engine,nw", KERNELS, ids=KERNEL_IDS)
@pytest.mark.parametrize("u8,log2,fc,bits", CONFIGS, ids=CONFIG_IDS)
def test_instantiation_in_a_batch_of_two(u8, log2, fc, bits, path, engine, nw, monkeypatch):
    """sdrx_decim_process_dev_batch: the kernels take their stream from blockIdx.y.  Two fresh handles in one launch, the three-chunk
    buffer and the short one: the second row of the grid has fewer units than the grid is wide."""
    torch = pytest.importorskip("torch")
    pin(monkeypatch, path, engine, nw)
    ref = reference(u8, log2, fc, bits, path == "exact")
    streams = [ref[0], ref[2]]
    name = kernel_name(path, engine, nw, u8, log2, fc, bits)
    hs = [sa.DecimatorsU(log2, fc, 127) if u8 else sa.Decimators(log2, fc, bits) for _ in streams]
    d_in = [torch.from_numpy(np.concatenate([x, np.zeros(16, x.dtype)])).cuda() for x, _, _ in streams]
    d_out = [torch.zeros(x.size + 64, dtype=torch.int16, device="cuda") for x, _, _ in streams]
    torch.cuda.synchronize()
    n_out = sa.decimate_dev_batch(hs, [t.data_ptr() for t in d_in], [x.size for x, _, _ in streams], [t.data_ptr() for t in d_out])
    hs[0].sync()
    ll = hs[0].last_launch()
    assert ll["kernel"] == name and ll["grid"] >= 2 * 3, (ll, name)
    for i, (x, want, bad) in enumerate(streams):
        got = d_out[i].cpu().numpy()
        assert 2 * n_out[i] == want.size and np.array_equal(got[: want.size], want), (name, "stream", i, n_out[i], want.size)
        assert not got[2 * ((x.size // 2) >> log2):].any(), (name, "stream", i, "wrote behind what the caller's buffer must hold")
        rep = hs[i].last_fallback()
        assert (rep["flagged"], rep["total"]) == ((0, 0) if path == "exact" else (0, bad.size)), (name, i, rep["flagged"], rep["total"])
    for h in hs:
        h.close()
