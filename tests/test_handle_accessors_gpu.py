"""GPU: the stream, timing and launch-record accessors behave the same in every handle family that has the full set
(sdrx_{decim,fdecim,chan_bank,spectrum,wfm,am}_*), each at the smallest shape that still launches a kernel."""
import numpy as np
import pytest

import sdrangel_amd as sa
from tests import am_cases as ac
from tests import synth
from tests import wfm_cases as wc

pytestmark = pytest.mark.gpu


def _decim():
    d = sa.Decimators(1, sa.FC_CEN, 12)
    x = synth.mix(sa.lib().sdrx_decim_group_int16(1, sa.FC_CEN) // 2, 3, 2047)          # one group
    return d, lambda: d.decimate(x).copy()


def _fdecim():
    d = sa.FloatDecimators("fi", 1, sa.FC_CEN)
    x = synth.mix(sa.lib().sdrx_fdecim_group(1, sa.FC_CEN) // 2, 4, 2047).astype(np.float32) / 32768.0
    return d, lambda: d.decimate(x).copy()


def _chan():
    b = sa.ChannelizerBank(61_440_000, [48000], [1_234_567])
    x = synth.mix(8192, 5, 2047, 500)

    def feed():
        b.feed(x)
        return b.read(0).copy()
    return b, feed


def _spectrum():
    g = sa.SpectrumVis(fft_size=64)
    x = synth.mix(2 * 64, 6, 2047, 500)                    # two frames of the smallest transform

    def feed():
        g.feed(x)
        return g.read().copy()
    return g, feed


def _wfm():
    cfg = wc.CASES[0]["cfg"]
    b = sa.WfmDemodBank([sa.WfmCfg(in_rate=int(cfg[0]), nco_freq=int(cfg[1]), audio_rate=int(cfg[2]), rf_bandwidth=float(cfg[3]),
                                   af_bandwidth=float(cfg[4]), volume=float(cfg[5]), squelch_db=float(cfg[6]), audio_mute=int(cfg[7]))])
    x = wc.inputs(wc.CASES[0])[: 2 * 5000]

    def feed():
        b.feed([x])
        return b.read(0)
    return b, feed


def _am():
    cfg = ac.CASES[0]["cfg"]
    b = sa.AmDemodBank([sa.AmCfg(in_rate=int(cfg[0]), nco_freq=int(cfg[1]), audio_rate=int(cfg[2]), rf_bandwidth=float(cfg[3]),
                                 volume=float(cfg[4]), squelch_db=float(cfg[5]), audio_mute=int(cfg[6]), bandpass_enable=int(cfg[7]))])
    x = ac.inputs(ac.CASES[0])[: 2 * 5000]

    def feed():
        b.feed([x])
        return b.read(0)
    return b, feed


FAMILIES = {"Decimators": _decim, "FloatDecimators": _fdecim, "ChannelizerBank": _chan, "SpectrumVis": _spectrum,
            "WfmDemodBank": _wfm, "AmDemodBank": _am}


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_accessors(family):
    import torch
    h, feed = FAMILIES[family]()
    assert type(h).__name__ == family
    # timing off: a feed is not counted
    h.reset()
    own_out = feed()
    assert own_out.size > 0
    assert h.get_timing()[1] == 0
    ll = h.last_launch()
    print(family, ll)
    assert ll["kernel"] and ll["grid"] > 0 and ll["block"] > 0, ll
    # timing on: one feed, one bracket
    h.set_timing(True)
    feed()
    ms, n = h.get_timing(reset=False)
    assert n == 1 and ms > 0, (ms, n)
    assert h.get_timing(reset=False) == (ms, n)
    assert h.get_timing(reset=True) == (ms, n)
    assert h.get_timing() == (0.0, 0)
    h.set_timing(False)
    # the caller's stream: the same result from a fresh state (for AmDemodBank this needs the front to follow the stream)
    has_get = hasattr(h, "get_stream")
    own = h.get_stream() if has_get else None
    if has_get:
        assert own != 0
    s = torch.cuda.Stream()
    h.set_stream(s.cuda_stream)
    if has_get:
        assert h.get_stream() == s.cuda_stream
    h.reset()
    got = feed()
    assert got.dtype == own_out.dtype and np.array_equal(got, own_out)
    h.sync()
    h.set_stream(None)
    if has_get:
        assert h.get_stream() == own
    h.close()
