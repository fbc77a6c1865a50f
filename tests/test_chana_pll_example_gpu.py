"""The analyzer example with --pll (examples/filesource_to_chanalyzer.py) runs on the GPU: every Sample of every file equals the
oracle's (channelizer oracle, then tests/chana_pll_oracle.c), the PLL slice locks on its tone and the FLL slice shows an oscillator."""
import importlib.util
import os

import numpy as np
import pytest

import sdrangel_amd as sa
from tests import chana_pll_cases as pc
from tests import oracle_py as orc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_example_with_pll_equals_the_oracle(tmp_path):
    spec = importlib.util.spec_from_file_location("filesource_to_chanalyzer", os.path.join(ROOT, "examples", "filesource_to_chanalyzer.py"))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    res = mod.main(str(tmp_path), pll=True)
    _hdr, payload = sa.sdriq_parse(open(res["recording"], "rb").read())
    L = pc.build_oracle()
    for c, fc in enumerate(mod.CENTRES):
        modes, out_rate, ofs = orc.chan_plan(mod.FS, mod.REQ_RATE, fc)
        chain = orc.Chain(modes)
        cfg = dict(mod.channel_settings(c, out_rate, ofs, pll=True), psk_order=1)
        o = pc.OraclePll(L, cfg)
        want, pos = [], 0
        for n in res["spans"]:
            want.append(o.feed(chain.feed(payload[2 * pos: 2 * (pos + n)])))
            pos += n
        want = np.concatenate(want)
        got = np.load(res["npy"][c])
        assert got.shape == want.shape and got.shape[0] >= 4096 and np.array_equal(got, want), (c, got.shape, want.shape)
        if c == 0:
            locked, freq, dphi, phi = res["pll_state"]
            st = o.state()
            assert (int(locked),) + tuple(int(np.float32(v).view(np.uint32)) for v in (freq, dphi, phi)) == st[:4]
            assert locked, st
        if c == 2:                                          # InputPLL behind the FLL: points on the circle of radius 32768
            r = np.hypot(got[:, 0].astype(np.float64), got[:, 1].astype(np.float64))
            assert np.all(np.abs(r - 32768) < 2 * 32768 * 1e-4 + 2) or np.all((r > 32000) | (np.abs(got).max(axis=1) == 32768)), r.min()
