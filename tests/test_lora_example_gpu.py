"""The LoRa example (examples/filesource_to_lora.py: .sdriq -> FIFO -> channelizer bank -> feed_bank -> lines and .npy) runs on the
GPU.  Its recording is built from a case's generator (tests/lora_cases.py) at the recording's rate, one frame per carrier; every
Sample of every .npy file and every line equal what a LoRa bank gives when it is fed, span by span, the channelizer oracle's
output for that carrier through the host entry point, and each carrier prints a line."""
import importlib.util
import os

import numpy as np
import pytest

import sdrangel_amd as sa
from tests import lora_cases as lc
from tests import oracle_py as orc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_example_equals_the_bank_behind_the_channelizer_oracle(tmp_path):
    spec = importlib.util.spec_from_file_location("filesource_to_lora", os.path.join(ROOT, "examples", "filesource_to_lora.py"))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    fr = lc.frame(24, 70)
    units = 256 * (fr["pre"] + fr["data"] + fr["down"]) + 600
    n = int(units * mod.FS / min(mod.BANDWIDTHS))
    t = np.arange(n) / mod.FS
    x = np.zeros(n, np.complex128)
    for c, (fc, bw) in enumerate(zip(mod.CARRIERS, mod.BANDWIDTHS)):
        iq = lc.signal({"kind": "frames", "frames": [fr], "lead": 0}, n, (mod.FS, 0, bw), 900 + c).astype(np.float64)
        x += 0.4 * (iq[0::2] + 1j * iq[1::2]) * np.exp(2j * np.pi * fc * t)
    res = mod.main(str(tmp_path), signal=x)
    _hdr, payload = sa.sdriq_parse(open(res["recording"], "rb").read())
    assert len(res["npy"]) == len(mod.CARRIERS) and sum(res["spans"]) == n
    for c, fc in enumerate(mod.CARRIERS):
        modes, out_rate, ofs = orc.chan_plan(mod.FS, mod.REQ_RATES[c], fc)
        chain = orc.Chain(modes)
        bank = sa.LoraDemodBank([sa.LoraCfg(in_rate=out_rate, nco_freq=-ofs, bandwidth=mod.BANDWIDTHS[c])])
        want, text, pos = [], "", 0
        for m in res["spans"]:
            bank.feed([chain.feed(payload[2 * pos: 2 * (pos + m)])])
            want.append(bank.read(0)); text += bank.read_text(0)
            pos += m
        want = np.concatenate(want)
        got = np.load(res["npy"][c])
        assert got.shape == want.shape and got.shape[0] > units // 2, (c, got.shape, want.shape)
        assert np.array_equal(got, want), c
        assert res["lines"][c] == text.split("\n")[:-1] and len(res["lines"][c]) >= 1, (c, res["lines"][c], text)
        st = res["state"][c]
        assert (st.count, st.lines) == (got.shape[0], len(res["lines"][c]))
