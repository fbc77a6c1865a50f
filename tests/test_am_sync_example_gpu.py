"""The airband example with --sync (examples/filesource_to_am.py: .sdriq -> FIFO -> channelizer bank at 48000 -> feed_bank ->
synchronous AM -> WAV) runs on the GPU: every carrier sits on its channel's centre, so every loop ends locked, and the WAV files hold
the audio the handle gave for the same spans through host pointers."""
import importlib.util
import os
import wave

import numpy as np
import pytest

import sdrangel_amd as sa

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("op", ["usb", "dsb"])
def test_example_with_sync(tmp_path, op):
    spec = importlib.util.spec_from_file_location("filesource_to_am", os.path.join(ROOT, "examples", "filesource_to_am.py"))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    res = mod.main(str(tmp_path), sync=op)
    _hdr, payload = sa.sdriq_parse(open(res["recording"], "rb").read())
    assert len(res["wav"]) == len(mod.CARRIERS) == len(res["pll"])
    # the same spans through a channelizer bank and a sync handle of the test's own, by host pointers
    bank = sa.ChannelizerBank(mod.FS, [mod.REQ_RATE] * len(mod.CARRIERS), mod.CARRIERS)
    am = sa.AmDemodBank(mod.demod_cfgs(bank), sync=[sa.AmSyncCfg(pll=1, sync_op=mod.SYNC_OPS[op], ssb_design_rate=mod.AUDIO_RATE,
                                                                 ssb_design_bw=mod.RF_BW)] * len(mod.CARRIERS))
    want, pos = [[] for _ in mod.CARRIERS], 0
    for n in res["spans"]:
        bank.feed(payload[2 * pos: 2 * (pos + n)])
        am.feed([bank.read(c) for c in range(len(mod.CARRIERS))])
        for c in range(len(mod.CARRIERS)):
            want[c].append(am.read(c))
        pos += n
    for c in range(len(mod.CARRIERS)):
        with wave.open(res["wav"][c], "rb") as w:
            assert (w.getnchannels(), w.getsampwidth(), w.getframerate()) == (1, 2, mod.AUDIO_RATE)
            got = np.frombuffer(w.readframes(w.getnframes()), "<i2")
        w_c = np.concatenate(want[c])
        assert got.size == w_c.size > 2 * mod.AUDIO_RATE // 10 and np.array_equal(got, w_c), c
        assert got[mod.AUDIO_RATE // 10:].any(), c
        locked, freq = res["pll"][c]
        assert locked and (locked, freq) == am.pll(c), (c, res["pll"][c], am.pll(c))
