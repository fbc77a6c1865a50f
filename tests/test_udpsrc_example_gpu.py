"""The UDP example (examples/filesource_to_udp.py: .sdriq -> FIFO -> channelizer bank at 48000 -> feed_bank -> datagram payloads
in files) runs on the GPU without opening a socket, and every datagram equals the oracle's stream (channelizer oracle, then
tests/udpsrc_oracle.c) cut at 512 bytes; the discriminator format under the rule of tests/test_udpsrc_gpu.py."""
import importlib.util
import os
import socket

import numpy as np
import pytest

import sdrangel_amd as sa
from tests import oracle_py as orc
from tests import udpsrc_cases as uc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_example_payloads_equal_the_oracle(tmp_path, monkeypatch):
    def no_socket(*a, **k):
        raise AssertionError("the example must not open a socket")
    monkeypatch.setattr(socket, "socket", no_socket)
    spec = importlib.util.spec_from_file_location("filesource_to_udp", os.path.join(ROOT, "examples", "filesource_to_udp.py"))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    res = mod.main(str(tmp_path))
    _hdr, payload = sa.sdriq_parse(open(res["recording"], "rb").read())
    L = uc.build_oracle()
    assert len(res["payloads"]) == len(mod.CARRIERS) and set(mod.FORMATS) == {0, 1, 3, 9}
    for c, fc in enumerate(mod.CARRIERS):
        fmt = mod.FORMATS[c]
        modes, out_rate, ofs = orc.chan_plan(mod.FS, mod.REQ_RATE, fc)
        chain = orc.Chain(modes)
        o = uc.OracleUdp(L, (out_rate, -ofs, mod.OUT_RATE, fmt, mod.RF_BW, mod.FM_DEV, mod.GAIN, mod.SQUELCH_DB, mod.GATE, 1, mod.AGC[c]))
        want, pos = [], 0
        for n in res["spans"]:
            want.append(o.feed(chain.feed(payload[2 * pos: 2 * (pos + n)]))[0])
            pos += n
        want = np.concatenate(want)
        per = 512 // uc.elem_bytes(fmt)
        raw = open(res["payloads"][c], "rb").read()
        assert res["totals"][c] == want.shape[0] == o.state()["total"] and want.shape[0] > 5000, (c, res["totals"][c], want.shape)
        assert len(raw) == 512 * res["datagrams"][c] and res["datagrams"][c] == want.shape[0] // per, (c, len(raw))
        got = uc.as_samples(fmt, raw)
        want = want[: got.shape[0]]
        assert o.state()["open"] and got.any(), c
        if fmt == uc.NFM_MONO:
            diff = (got.astype(np.int32) - want.astype(np.int32)).astype(np.int16)
            assert np.abs(diff.astype(np.int32)).max() <= 1 and 4 * np.count_nonzero(diff) <= got.size, c
        else:
            assert np.array_equal(got, want), c
