"""sdrx_spectrum_* on the MI355X against the strict-IEEE restatement of SpectrumVis (tests/spectrum_oracle.c), case by case
(tests/spectrum_cases.py): window tables bit for bit, the frame count of every feed, linear output and averaged linear power
bit-identical.  dB output: the device evaluates log2f in double and rounds once.  It must lie within 1 ulp of the oracle
run with that same log2 (any further difference would come from the power or the averaging), and the bins that differ
from the glibc-log2f oracle at all are counted and printed, with the largest distance: a 1-ulp log2f difference becomes
several ulps of m_mult * log2f(v) + m_ofs where the sum cancels (dB values near 0)."""
import numpy as np
import pytest

import sdrangel_amd as sa
from tests import spectrum_cases as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def oracle():
    return sc.build_oracle()


def _compare(got, want, want_dbl, linear, what, stats):
    """stats: [bins differing from the glibc oracle, bins compared, largest ulp distance to it, bins differing from the
    double-log2 oracle]"""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if linear:
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), what
        return
    d = sc.ulp_diff(got, want)
    d2 = sc.ulp_diff(got, want_dbl)
    stats[0] += int(np.count_nonzero(d)); stats[1] += d.size
    stats[2] = max(stats[2], int(d.max(initial=0))); stats[3] += int(np.count_nonzero(d2))
    assert int(d2.max(initial=0)) <= 1, (what, int(d2.max()), np.argwhere(d2 > 1)[:5])
    # where the two log2 flavours agree the frame must too (up to that same 1-ulp allowance)
    same = want.view(np.int32) == want_dbl.view(np.int32)
    assert int(d[same].max(initial=0)) <= 1, what


def _report(name, stats):
    print(f"{name}: {stats[0]} of {stats[1]} dB bins differ from glibc log2f (max {stats[2]} ulp), {stats[3]} from the double-log2 oracle")


@pytest.mark.parametrize("case", sc.CASES, ids=[c["name"] for c in sc.CASES])
def test_spectrum_matches_oracle(oracle, case):
    want = sc.run_oracle(oracle, case)
    want_dbl = sc.run_oracle(oracle, case, log2_double=True)
    cfg = case["cfg"]
    g = sa.SpectrumVis(*cfg)
    assert np.array_equal(g.window().view(np.int32), want[0][1].view(np.int32)), "window"
    linear = cfg[5]
    stats = [0, 0, 0, 0]
    for i, (step, iq) in enumerate(zip(case["steps"], sc.inputs(case))):
        kind, ref = want[i + 1]
        if step[0] == "configure":
            g.configure(*step[1])
            linear = step[1][5]
            assert np.array_equal(g.window().view(np.int32), ref.view(np.int32)), f"window after step {i}"
            continue
        g.feed(iq, step[2])
        assert g.available() == ref.shape[0], f"step {i}: {g.available()} frames queued, oracle emitted {ref.shape[0]}"
        _compare(g.read(), ref, want_dbl[i + 1][1], linear, f"step {i}", stats)
        assert g.available() == 0
    _report(case["name"], stats)
    ll = g.last_launch()
    assert ll["kernel"] == "spectrum_fft_kernel" and ll["block"] == 256 and ll["grid"] > 0
    g.close()


@pytest.mark.parametrize("n_fft", [1024, 4096])
def test_one_second_at_61m44(oracle, n_fft):
    """one second of a 61.44 MS/s device stream, in 64 Ki-sample spans, dB and moving average"""
    rng = np.random.default_rng(n_fft)
    total, span = 61_440_000, 65536
    for cfg in [(n_fft, 0, 0, sc.NONE, sc.BH, 0), (n_fft, 10, 5, sc.MOVING, 3, 0)]:
        g, o, o2 = sa.SpectrumVis(*cfg), sc.OracleSpectrum(oracle, cfg), sc.OracleSpectrum(oracle, cfg, log2_double=True)
        stats, frames = [0, 0, 0, 0], 0
        for s in range(0, total, span):
            iq = sc.signal("noise" if (s // span) % 3 else "tone", min(span, total - s), rng)
            ref, ref2 = o.feed(iq, False), o2.feed(iq, False)
            g.feed(iq)
            assert g.available() == ref.shape[0]
            _compare(g.read(), ref, ref2, False, f"span at {s}", stats)
            frames += ref.shape[0]
        _report(f"N={n_fft} cfg={cfg}, {frames} frames", stats)
        g.close(); o.close(); o2.close()


def test_feed_dev_equals_feed():
    import torch
    rng = np.random.default_rng(3)
    cfg = (2048, 25, 3, sc.MOVING, sc.BH, 1)
    a, b = sa.SpectrumVis(*cfg), sa.SpectrumVis(*cfg)
    for n in (5000, 1, 2047, 30000, 700):
        iq = sc.signal("noise", n, rng)
        a.feed(iq)
        t = torch.from_numpy(iq).to("cuda:0")
        torch.cuda.synchronize()
        b.feed_dev(t)
        b.sync()
        assert a.available() == b.available()
        x, y = a.read(), b.read()
        assert np.array_equal(x.view(np.int32), y.view(np.int32))
    assert b.last_launch()["kernel"] == "spectrum_fft_kernel"


def test_queue_and_state_rules():
    g = sa.SpectrumVis(256, 0, 0, sc.NONE, sc.BH, 0)
    g.feed(np.zeros(2 * 256 * 5, np.int16))
    assert g.available() == 5
    with pytest.raises(sa.SdrxError):
        g.configure(512, 0, 0, sc.NONE, sc.BH, 0)      # queued frames of another size
    assert g.skip(2) == 2 and g.available() == 3
    fr = g.read()
    assert fr.shape == (3, 256) and np.all(np.isneginf(fr))
    g.configure(512, 0, 0, sc.NONE, sc.BH, 0)
    g.reset()
    assert g.available() == 0 and g.fft_size == 512
    g.set_timing(True)
    g.feed(np.ones(2 * 512 * 4, np.int16))
    ms, feeds = g.get_timing()
    assert feeds == 1 and ms > 0
    assert g.get_stream() != 0


def test_cxx_mirror_delivers_frames(tmp_path):
    """sdrx::SpectrumVis (include/sdrx/dsp.hpp) hands every frame to its newSpectrum callback, in the order of the C ABI"""
    import os
    import subprocess
    src = tmp_path / "spec_mirror.cpp"
    src.write_text(r'''
#include "sdrx/dsp.hpp"
#include <cstring>
int main() {
    int frames = 0; unsigned h = 2166136261u;
    sdrx::SpectrumVis v(32768.0f, [&](const std::vector<float>& s, int n) {
        frames++;
        for (int i = 0; i < n; i++) { unsigned b; std::memcpy(&b, &s[i], 4); h = (h ^ b) * 16777619u; }
    });
    if (!v.ok() || !v.configure(256, 25, 3, 1, 1, true)) return 1;
    sdrx::SampleVector x(5000);
    for (size_t i = 0; i < x.size(); i++) x[i] = sdrx::Sample((int16_t)(i * 7919 % 65536 - 32768), (int16_t)(i * 104729 % 65536 - 32768));
    v.feed(x.begin(), x.begin() + 100, false);
    v.feed(x.begin() + 100, x.end(), false);
    std::printf("%d %u\n", frames, h);
    return 0;
}
''')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "spec_mirror")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(root, "include"), str(src), "-o", exe,
                           "-L", os.path.join(root, "sdrangel_amd"), "-lsdrx", "-Wl,-rpath," + os.path.join(root, "sdrangel_amd")])
    frames, h = subprocess.run([exe], capture_output=True, text=True, timeout=120, check=True).stdout.split()
    i = np.arange(5000, dtype=np.int64)
    iq = np.empty(10000, np.int16)
    iq[0::2] = (i * 7919 % 65536 - 32768).astype(np.int16)
    iq[1::2] = (i * 104729 % 65536 - 32768).astype(np.int16)
    g = sa.SpectrumVis(256, 25, 3, sc.MOVING, sc.BH, 1)
    g.feed(iq[:200]); g.feed(iq[200:])
    want = g.read()
    hh = 2166136261
    for b in want.reshape(-1).view(np.uint32):
        hh = ((hh ^ int(b)) * 16777619) & 0xFFFFFFFF
    assert int(frames) == want.shape[0] and int(h) == hh
