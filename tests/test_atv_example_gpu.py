"""The ATV example (examples/filesource_to_atv.py: .sdriq -> FIFO -> channelizer bank -> feed_bank -> one .pgm per stored frame)
runs on the GPU.  Every frame file, the last screen, the render events and the state equal what the ATV oracle
(tests/atv_oracle.cpp) gives when it is fed, span by span, the channelizer oracle's output for that carrier; each carrier stores
frames and its picture is no blank."""
import importlib.util
import os

import numpy as np
import pytest

import sdrangel_amd as sa
from tests import atv_cases as ac
from tests import oracle_py as orc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def read_pgm(path):
    raw = open(path, "rb").read()
    magic, size, maxval, data = raw.split(b"\n", 3)
    w, h = (int(v) for v in size.split())
    assert magic == b"P5" and maxval == b"255" and len(data) == w * h
    return np.frombuffer(data, np.uint8).reshape(h, w)


def test_example_equals_the_oracle_behind_the_channelizer_oracle(tmp_path):
    spec = importlib.util.spec_from_file_location("filesource_to_atv", os.path.join(ROOT, "examples", "filesource_to_atv.py"))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    res = mod.main(str(tmp_path))
    _hdr, payload = sa.sdriq_parse(open(res["recording"], "rb").read())
    L = ac.build_oracle()
    assert sum(res["spans"]) == payload.size // 2 and len(res["spans"]) >= 2
    for c, fc in enumerate(mod.CARRIERS):
        modes, out_rate, ofs = orc.chan_plan(mod.FS, mod.REQ_RATES[c], fc)
        chain = orc.Chain(modes)
        k = {name: getattr(res["cfgs"][c], name) for name, _ in ac.CFG_FIELDS}
        assert (k["in_rate"], k["nco_freq"]) == (out_rate, -ofs)
        o = ac.OracleAtv(L, k)
        frames, pos = [], 0
        for i, m in enumerate(res["spans"]):
            f = o.feed(chain.feed(payload[2 * pos: 2 * (pos + m)]))
            assert np.array_equal(res["events"][c][i], f["events"]), (c, i)
            frames += f["frames"]
            pos += m
        assert len(res["frames"][c]) == len(frames) >= mod.FRAMES - 2, (c, len(res["frames"][c]), len(frames))
        for p, want in zip(res["frames"][c], frames):
            assert np.array_equal(read_pgm(p), want), p
        assert np.array_equal(read_pgm(res["screens"][c]), f["screen"])
        assert ac.state_words(res["state"][c]) == f["state"]
        assert len(np.unique(frames[-1])) > 4, c                      # a picture, not a blank
        o.close()
