"""CPU: sdrx_udpsrc_* rejects bad configurations with SDRX_EINVAL and a message before any device is touched (the SSB formats
4 .. 7 among them), fails loudly without a device (no CPU fallback), its accessors refuse a null
handle, and the datagram framing of UdpPayloadCutter (what UdpSrcBank.payloads hands out) is UDPSink<T>::write's."""
import ctypes as C

import numpy as np
import pytest

import sdrangel_amd as sa

GOOD = dict(in_rate=48000, nco_freq=-1000, output_sample_rate=8000.0, sample_format=0, rf_bandwidth=5000.0, fm_deviation=2500, gain=1.0,
            squelch_db=-60, squelch_gate=5, squelch_enabled=1, agc=0)


def _create(n_ch=1, cfgs=None, **kw):
    d = dict(GOOD); d.update(kw)
    arr = (sa.UdpSrcCfg * max(n_ch, 1))(*(cfgs or [sa.UdpSrcCfg(**d)] * max(n_ch, 1)))
    h = C.c_void_p()
    # device 1 << 20 does not exist anywhere: a configuration that passes validation must then fail with SDRX_ENODEV
    rc = sa.lib().sdrx_udpsrc_create(C.byref(h), 1 << 20, n_ch, arr)
    assert not h.value
    return rc, sa.lib().sdrx_last_error().decode()


@pytest.mark.parametrize("fmt", [4, 5, 6, 7])
def test_the_ssb_formats_are_rejected(fmt):
    rc, msg = _create(sample_format=fmt)
    assert rc == -1 and "sdrx_udpsrc_create" in msg and "SSB" in msg, (rc, msg)


@pytest.mark.parametrize("kw", [dict(sample_format=11), dict(sample_format=-1), dict(sample_format=1 << 20),
                                dict(output_sample_rate=48000.5), dict(output_sample_rate=0.0), dict(output_sample_rate=999.0),
                                dict(output_sample_rate=-8000.0), dict(output_sample_rate=float("nan")), dict(output_sample_rate=float("inf")),
                                dict(in_rate=0), dict(in_rate=-5), dict(in_rate=4000),
                                dict(in_rate=1 << 30, output_sample_rate=1.5e7),
                                dict(rf_bandwidth=0.0), dict(rf_bandwidth=-5000.0), dict(rf_bandwidth=float("nan")), dict(rf_bandwidth=2.0e7),
                                dict(sample_format=10, rf_bandwidth=600.0),
                                dict(fm_deviation=0), dict(fm_deviation=-2500), dict(squelch_gate=-1), dict(squelch_gate=1001),
                                dict(squelch_db=-301), dict(squelch_db=301), dict(gain=float("nan")), dict(gain=float("inf")),
                                dict(sample_format=9, gain=float("-inf"))])
def test_bad_configurations_are_rejected_before_the_device(kw):
    rc, msg = _create(**kw)
    assert rc == -1 and "sdrx_udpsrc_create" in msg, (rc, msg)      # SDRX_EINVAL, not SDRX_ENODEV


def test_bad_arguments():
    assert _create(n_ch=0)[0] == -1
    assert sa.lib().sdrx_udpsrc_create(None, 0, 1, (sa.UdpSrcCfg * 1)(sa.UdpSrcCfg(**GOOD))) == -1
    h = C.c_void_p()
    assert sa.lib().sdrx_udpsrc_create(C.byref(h), 0, 1, None) == -1
    # a bad channel anywhere in the list
    cfgs = [sa.UdpSrcCfg(**GOOD), sa.UdpSrcCfg(**dict(GOOD, sample_format=5))]
    assert _create(n_ch=2, cfgs=cfgs)[0] == -1
    assert sa.lib().sdrx_udpsrc_destroy(None) == 0


def test_null_handle_accessors():
    L = sa.lib()
    ptrs, ns = (C.c_void_p * 1)(), (C.c_int64 * 1)(0)
    out, p, n = (C.c_int16 * 4)(), C.c_void_p(), C.c_int64()
    d, g, g2, nt, fs = C.c_double(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_float()
    name, a, b, c = C.create_string_buffer(64), C.c_int(), C.c_int(), C.c_int()
    calls = [(L.sdrx_udpsrc_reset, (None,)), (L.sdrx_udpsrc_sync, (None,)), (L.sdrx_udpsrc_feed, (None, ptrs, ns)),
             (L.sdrx_udpsrc_feed_dev, (None, ptrs, ns)), (L.sdrx_udpsrc_feed_bank, (None, None)), (L.sdrx_udpsrc_sample_bytes, (None, 0)),
             (L.sdrx_udpsrc_read, (None, 0, out, 1)), (L.sdrx_udpsrc_last_dev, (None, 0, C.byref(p), C.byref(n))),
             (L.sdrx_udpsrc_read_spectrum, (None, 0, out, 1)), (L.sdrx_udpsrc_spectrum_last_dev, (None, 0, C.byref(p), C.byref(n))),
             (L.sdrx_udpsrc_squelch_open, (None, 0)), (L.sdrx_udpsrc_squelch_counts, (None, 0, C.byref(g), C.byref(g2))),
             (L.sdrx_udpsrc_in_magsq, (None, 0, C.byref(d))), (L.sdrx_udpsrc_total, (None, 0)),
             (L.sdrx_udpsrc_get_design, (None, 0, C.byref(nt), None, 0, None, C.byref(g), None, C.byref(g), C.byref(g2), C.byref(d), C.byref(fs), C.byref(fs), None, C.byref(d))),
             (L.sdrx_udpsrc_set_stream, (None, None)), (L.sdrx_udpsrc_get_stream, (None, C.byref(p))), (L.sdrx_udpsrc_set_timing, (None, 1)),
             (L.sdrx_udpsrc_get_timing, (None, C.byref(d), C.byref(n), 0)),
             (L.sdrx_udpsrc_last_launch, (None, name, 64, C.byref(a), C.byref(b), C.byref(c)))]
    for fn, args in calls:
        assert fn(*args) == -1, fn.__name__


@pytest.mark.parametrize("kw", [dict(), dict(output_sample_rate=1000.0, in_rate=1000), dict(output_sample_rate=48000.0), dict(sample_format=1),
                                dict(sample_format=2, agc=1), dict(sample_format=3, squelch_gate=0), dict(sample_format=8, squelch_enabled=0),
                                dict(sample_format=9, squelch_gate=1000), dict(sample_format=10, rf_bandwidth=600.5), dict(output_sample_rate=11025.5),
                                dict(sample_format=0, agc=1), dict(sample_format=8, agc=1), dict(sample_format=9, agc=1),
                                dict(sample_format=10, agc=1), dict(sample_format=8, agc=1, in_rate=1 << 20, output_sample_rate=655365.0),
                                dict(sample_format=0, agc=1, in_rate=1 << 20, output_sample_rate=1000000.0)])
def test_a_good_configuration_reaches_the_device_check(kw):
    rc, msg = _create(**kw)
    assert rc == -2, (rc, msg)                                      # SDRX_ENODEV: validation passed, the device index did not


def test_no_cpu_fallback():
    if sa.lib().sdrx_device_count() > 0:
        return                                                      # the GPU suite creates handles there
    with pytest.raises(sa.SdrxError) as e:
        sa.UdpSrcBank([sa.UdpSrcCfg(**GOOD)])
    assert "rc=-2" in str(e.value)


def test_cfg_struct_matches_the_header():
    assert C.sizeof(sa.UdpSrcCfg) == 44 and sa.UdpSrcCfg.agc.offset == 40 and sa.UdpSrcCfg.output_sample_rate.offset == 8
    assert sa.UdpSrcCfg.sample_format.offset == 12 and sa.UdpSrcCfg.gain.offset == 24
    for name in ("create", "destroy", "reset", "feed", "feed_dev", "feed_bank", "sample_bytes", "read", "last_dev", "read_spectrum",
                 "spectrum_last_dev", "squelch_open", "squelch_counts", "in_magsq", "total", "get_design", "sync", "set_stream", "get_stream",
                 "set_timing", "get_timing", "last_launch"):
        assert f"sdrx_udpsrc_{name}" in sa.exported_symbols(), name


def test_payloads_takes_every_feed_once():
    """UdpSrcBank.payloads compares the running total with what its cutter has been given: a second call for the same feed adds
    nothing, and a feed that was never collected is an error, not a hole in the datagram stream"""
    class Fake(sa.UdpSrcBank):
        def __init__(self):
            self._cutters, self.n, self.last, self.reads = [sa.UdpPayloadCutter(2)], 0, 0, 0

        def feed_samples(self, k):
            self.n += k; self.last = k

        def total(self, ch):
            return self.n

        def last_dev(self, ch):
            return 0, self.last

        def read_raw(self, ch):
            self.reads += 1
            return bytes(2 * self.last)

        def close(self):
            pass

    b = Fake()
    assert b.payloads(0) == [] and b.reads == 0             # nothing fed yet
    b.feed_samples(300)
    assert len(b.payloads(0)) == 1 and b._cutters[0].pending == 44
    assert b.payloads(0) == [] and b.payloads(0) == [] and b.reads == 1
    b.feed_samples(300)
    assert len(b.payloads(0)) == 1 and b._cutters[0].pending == 88 and b.reads == 2
    b.feed_samples(0)                                       # an empty feed changes nothing
    assert b.payloads(0) == [] and b.reads == 2
    b.feed_samples(100)                                     # not collected ...
    b.feed_samples(50)
    with pytest.raises(sa.SdrxError):                       # ... so 150 are outstanding and the handle holds 50
        b.payloads(0)
    assert b.reads == 2 and b._cutters[0].pending == 88


@pytest.mark.parametrize("sample_bytes,per", [(4, 128), (2, 256), (8, 64)])
def test_payload_framing(sample_bytes, per):
    """UDPSink<T>::write sends exactly samples [k * M, (k + 1) * M), M = 512 / sizeof(T); the remainder waits across feeds"""
    rng = np.random.default_rng(sample_bytes)
    stream = rng.integers(0, 256, size=sample_bytes * (5 * per + 37), dtype=np.uint8).tobytes()
    cut = sa.UdpPayloadCutter(sample_bytes)
    assert cut.per_datagram == per
    feeds = [0, 1, per - 2, 1, 0, 1, 2 * per + 5, per - 5, 3, per + 28]          # in samples; sums to 5 * per + 37 - 5 ... checked below
    assert sum(feeds) == 5 * per + 32
    feeds.append(5)
    got, pos = [], 0
    pend = []
    for m in feeds:
        out = cut.push(stream[pos * sample_bytes: (pos + m) * sample_bytes])
        pos += m
        got += out
        pend.append(cut.pending)
        assert all(len(d) == 512 for d in out)
        assert cut.sent == len(got) * per and cut.pending == pos - cut.sent
    assert pos * sample_bytes == len(stream)
    assert len(got) == 5 and cut.pending == 37
    for k, d in enumerate(got):
        assert d == stream[k * 512: (k + 1) * 512]
    # the first datagram leaves with the feed that completes it, not earlier
    assert pend[:4] == [0, 1, per - 1, 0]
