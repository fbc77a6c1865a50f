"""Matrix-core decimator with the centre tap inside the tile (hb_mfma.hpp, CTR): bit-exact against the CPU oracle.

A centre-mode stage takes 15 of a block's 16 centre samples from the even arm's aligned window slots and output 15's from one
extra read merged into slot 0.  These cases pin both flavours of the FAST kernel and hit that output at ragged call ends, in
chains that mix centre and rotated stages, and with full-scale data (the even arm is stored biased, like the odd arm)."""
import numpy as np
import pytest

import sdrangel_amd as sa
from tests import oracle_py as orc

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _mx_engine(monkeypatch):
    monkeypatch.setenv("SDRX_DECIM_ENGINE", "mfma")


def _mx_lds_bytes(log2, nw):
    """LDS of decim_fast_kernel<log2, ..., nw, MX = true>: four arrays per stage (DfLay<MXT, PAD = true>) + the tail's zero block"""
    s_len = 1024 * nw
    mxt = nw == 1 and log2 >= 4
    words = 0
    for s in range(1, log2 + 1):
        words += 4 * ((16 + (s_len >> (s + 1)) + 16) if s <= 3 else (32 + (s_len >> s) + (0 if mxt else 1)))
    return 4 * (words + (4 if mxt else 0))


@pytest.mark.parametrize("nw", ("1", "4"))
@pytest.mark.parametrize("fcpos", (sa.FC_CEN, sa.FC_INF, sa.FC_SUP))
@pytest.mark.parametrize("log2", range(1, 7))
def test_centre_fold_ragged_calls(log2, fcpos, nw, monkeypatch):
    monkeypatch.setenv("SDRX_DECIM_NW", nw)
    n = 5 * 16384 + 3 * 1024 + 77                 # ragged at every stage: the last block of every stage is partial
    x = orc.synth_iq(n, seed=900 + 11 * log2 + 3 * fcpos + int(nw), amp=32767, tone=(0.0031, 20000))
    g = sa.Decimators(log2, fcpos, 16)
    o = orc.Decim(log2, fcpos, 16)
    cuts = [0, 2 * 1, 2 * 1000, 2 * 4096 + 2 * 15, 2 * 40017, 2 * n]
    for a, b in zip(cuts[:-1], cuts[1:]):
        got, want = g.decimate(x[a:b]), o.process(x[a:b])
        assert got.size == want.size and np.array_equal(got, want), (log2, fcpos, nw, a, b, int((got != want).sum()))
    launch = g.last_launch()
    assert launch["kernel"].endswith("+mfma"), launch
    assert launch["lds_bytes"] == _mx_lds_bytes(log2, int(nw)), launch


@pytest.mark.parametrize("nw", ("1", "4"))
@pytest.mark.parametrize("log2", (3, 6))
def test_centre_fold_full_scale(log2, nw, monkeypatch):
    """int16 extremes in both components.  This is the ALL-FLAGGED end of the FAST / EXACT pair: every one of the 25 chunks overflows an
    int16-stored stage (tests/test_decim_fallback.py counts them with the oracle's probe), so the outputs compared here are the EXACT
    kernel's; what the matrix-core FAST kernel contributes is the flag of every chunk, with full-scale entries in its biased even arm
    and extra centre term.  The FAST outputs that are KEPT on full-range data are pinned by tests/test_decim_fallback_gpu.py."""
    monkeypatch.setenv("SDRX_DECIM_NW", nw)
    n = 3 * 32768 + 500
    x = np.empty(2 * n, np.int16)
    x[0::2] = np.where(np.arange(n) % 3 == 0, -32768, 32767)
    x[1::2] = np.where(np.arange(n) % 5 < 2, 32767, -32768)
    g = sa.Decimators(log2, sa.FC_CEN, 16)
    o = orc.Decim(log2, sa.FC_CEN, 16)
    got, want = g.decimate(x), o.process(x)
    assert got.size == want.size and np.array_equal(got, want), (log2, nw, int((got != want).sum()))
    rep = g.last_fallback()
    assert rep["flagged"] == rep["total"] == 25, (log2, nw, rep["flagged"], rep["total"])
