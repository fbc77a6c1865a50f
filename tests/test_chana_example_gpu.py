"""The analyzer example (examples/filesource_to_chanalyzer.py: .sdriq -> FIFO -> channelizer bank at 48000 -> feed_bank -> .npy of
the Samples) runs on the GPU, and every Sample of every file equals the oracle's (channelizer oracle, then tests/chana_oracle.c)."""
import importlib.util
import os

import numpy as np
import pytest

import sdrangel_amd as sa
from tests import chana_cases as cc
from tests import oracle_py as orc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_example_samples_equal_the_oracle(tmp_path):
    spec = importlib.util.spec_from_file_location("filesource_to_chanalyzer", os.path.join(ROOT, "examples", "filesource_to_chanalyzer.py"))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    res = mod.main(str(tmp_path))
    _hdr, payload = sa.sdriq_parse(open(res["recording"], "rb").read())
    L = cc.build_oracle()
    assert len(res["npy"]) == len(mod.CENTRES)
    for c, fc in enumerate(mod.CENTRES):
        modes, out_rate, ofs = orc.chan_plan(mod.FS, mod.REQ_RATE, fc)
        chain = orc.Chain(modes)
        cfg = mod.channel_settings(c, out_rate, ofs)
        o = cc.OracleChana(L, {k: cfg[k] for k in cc.FIELDS})
        want, pos = [], 0
        for n in res["spans"]:
            want.append(o.feed(chain.feed(payload[2 * pos: 2 * (pos + n)])))
            pos += n
        want = np.concatenate(want)
        got = np.load(res["npy"][c])
        assert got.dtype == np.int16 and got.shape == want.shape and got.shape[0] >= 4096, (c, got.shape, want.shape)
        assert np.array_equal(got, want), c
        assert got.any(), c
        if mod.KINDS[c].get("input_type") == 2:
            assert not got[:4095].any() and o.state()[2] >= 1, c       # nothing before the first block of 4096 is complete
