"""The SSB example (examples/filesource_to_ssb.py: .sdriq -> FIFO -> channelizer bank at 48000 -> feed_bank -> stereo WAV) runs on
the GPU, and every sample of every WAV file equals the oracle's audio (channelizer oracle, then tests/ssb_oracle.c)."""
import importlib.util
import os
import wave

import numpy as np
import pytest

import sdrangel_amd as sa
from tests import oracle_py as orc
from tests import ssb_cases as sc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_example_wav_equals_the_oracle(tmp_path):
    spec = importlib.util.spec_from_file_location("filesource_to_ssb", os.path.join(ROOT, "examples", "filesource_to_ssb.py"))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    res = mod.main(str(tmp_path))
    _hdr, payload = sa.sdriq_parse(open(res["recording"], "rb").read())
    L = sc.build_oracle()
    assert len(res["wav"]) == len(mod.CARRIERS)
    for c, fc in enumerate(mod.CARRIERS):
        modes, out_rate, ofs = orc.chan_plan(mod.FS, mod.REQ_RATE, fc)
        chain = orc.Chain(modes)
        o = sc.OracleSsb(L, mod.channel_settings(c, out_rate, ofs))
        want, pos = [], 0
        for n in res["spans"]:
            want.append(o.feed(chain.feed(payload[2 * pos: 2 * (pos + n)]))[0])
            pos += n
        want = np.concatenate(want)
        with wave.open(res["wav"][c], "rb") as w:
            assert (w.getnchannels(), w.getsampwidth(), w.getframerate()) == (2, 2, mod.AUDIO_RATE)
            got = np.frombuffer(w.readframes(w.getnframes()), "<i2").reshape(-1, 2)
        assert got.shape == want.shape and got.shape[0] > 2 * mod.AUDIO_RATE // 10, (c, got.shape, want.shape)
        assert np.array_equal(got, want), c
        assert o.audio_active() and o.probe()["resets"] > got.shape[0] // 2
        z = got[mod.AUDIO_RATE // 10:, 0].astype(np.float64)
        s = np.abs(np.fft.rfft(z - z.mean()))
        f_peak = np.argmax(s) * mod.AUDIO_RATE / (2 * (s.size - 1))
        assert abs(f_peak - abs(mod.TONES[c])) < 20.0, (c, f_peak)
        mono = not mod.KINDS[c].get("audio_binaural")
        assert np.array_equal(got[:, 0], got[:, 1]) == mono, c
