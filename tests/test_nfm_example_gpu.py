"""The NFM audio example (examples/filesource_to_nfm_audio.py: .sdriq -> FIFO -> channelizer bank at 48000 -> feed_bank -> WAV)
runs on the GPU, and every sample of every WAV file equals the oracle's audio (channelizer oracle, then tests/nfm_oracle.c)."""
import importlib.util
import os
import wave

import numpy as np
import pytest

import sdrangel_amd as sa
from tests import nfm_cases as nc
from tests import oracle_py as orc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_example_wav_equals_the_oracle(tmp_path):
    spec = importlib.util.spec_from_file_location("filesource_to_nfm_audio", os.path.join(ROOT, "examples", "filesource_to_nfm_audio.py"))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    res = mod.main(str(tmp_path))
    _hdr, payload = sa.sdriq_parse(open(res["recording"], "rb").read())
    L = nc.build_oracle()
    assert len(res["wav"]) == len(mod.CARRIERS)
    for c, fc in enumerate(mod.CARRIERS):
        modes, out_rate, ofs = orc.chan_plan(mod.FS, mod.REQ_RATE, fc)
        chain = orc.Chain(modes)
        o = nc.OracleNfm(L, (out_rate, -ofs, mod.AUDIO_RATE, mod.RF_BW, mod.AF_BW, mod.FM_DEV, mod.VOLUME, mod.SQUELCH, mod.GATE, 0))
        want, pos = [], 0
        for n in res["spans"]:
            want.append(o.feed(chain.feed(payload[2 * pos: 2 * (pos + n)])))
            pos += n
        want = np.concatenate(want)
        with wave.open(res["wav"][c], "rb") as w:
            assert (w.getnchannels(), w.getsampwidth(), w.getframerate()) == (1, 2, mod.AUDIO_RATE)
            got = np.frombuffer(w.readframes(w.getnframes()), "<i2")
        assert got.size == want.size and got.size > 2 * mod.AUDIO_RATE // 10, (c, got.size, want.size)
        assert np.array_equal(got, want), c
        assert o.squelch_open() and o.probe()["open"] > got.size // 2
        z = got.astype(np.float64)[mod.AUDIO_RATE // 10:]
        s = np.abs(np.fft.rfft(z - z.mean()))
        f_peak = np.argmax(s) * mod.AUDIO_RATE / (2 * (s.size - 1))
        assert abs(f_peak - (500 + 400 * c)) < 20.0, (c, f_peak)
