"""Cases of the AM demodulator bank's synchronous-AM channels (sdrx_am_create_ex), shared by the golden recorder
tests/golden/make_golden_am_sync.py, tests/test_am_sync_gpu.py and tests/test_am_sync_host.py.

A case is a demodulator configuration, its sync options, a signal at the channel rate and the lengths of the feeds it is cut into:
    cfg  = (in_rate, nco_freq, audio_rate, rf_bandwidth, volume, squelch_db, audio_mute, bandpass_enable)     as tests/am_cases.py
    sync = (pll, sync_op, ssb_design_rate, ssb_design_bw)       sync_op 0 DSB, 1 USB, 2 LSB; the two design values as SSBFilter got them
    sig  = {"kind": ...}   see signal()

The `am2` signal is a carrier at f0 whose two sidebands carry different tones (fu above, fl below, different depths), so that a
swapped sideband changes the audio, and whose amplitude follows a list of runs.  Rates are low (4 to 8 kS/s audio) so that the
squelch opens after a few hundred samples, the AGC history (rate / 4) fills, and six to twelve filter blocks fit in under 10 000
audio samples.  The expectations (`locked`, `reopens`, `never_open`, `sat`) are asserted by the recorder's maker on the recording
itself."""
from __future__ import annotations

import hashlib

import numpy as np

from tests.am_cases import _amp_runs
from tests.wfm_cases import _clip16, _gauss, _uniform_i16, cut  # noqa: F401  (cut is re-exported)

DSB, USB, LSB = 0, 1, 2
OPS = ("dsb", "usb", "lsb")


def block(sync_op: int) -> int:
    return 1024 if sync_op == DSB else 512


def signal(sig: dict, n: int, rate: int, seed: int) -> np.ndarray:
    kind = sig["kind"]
    iq = np.empty(2 * n, np.int16)
    if kind == "noise_full":
        iq[0::2] = _uniform_i16(seed, n, 1)
        iq[1::2] = _uniform_i16(seed, n, 2)
    elif kind == "am2":
        t = np.arange(n, dtype=np.float64)
        inc = int(round(sig.get("f0", 0.0) / rate * 4294967296.0))
        ph = ((np.arange(1, n + 1, dtype=np.int64) * inc) & 0xFFFFFFFF).astype(np.float64) * (2 * np.pi / 4294967296.0)
        amp = _amp_runs(n, sig["runs"], sig["amps"]) if "runs" in sig else np.full(n, float(sig.get("amp", 6000.0)))
        up = float(sig.get("du", 0.45)) * np.exp(2j * np.pi * float(sig.get("fu", 400.0)) * t / rate)
        lo = float(sig.get("dl", 0.25)) * np.exp(-2j * np.pi * float(sig.get("fl", 650.0)) * t / rate)
        z = amp * np.exp(1j * ph) * (1.0 + up + lo)
        sg = float(sig.get("noise", 10.0))
        iq[0::2] = _clip16(z.real + _gauss(seed, n, 3, sg))
        iq[1::2] = _clip16(z.imag + _gauss(seed, n, 4, sg))
    else:
        raise ValueError(kind)
    return iq


def _cfg(in_rate, audio_rate, nco_freq=0, rf=3000.0, vol=1.0, sq=-40.0, mute=0, bp=0):
    return (in_rate, nco_freq, audio_rate, rf, vol, sq, mute, bp)


def _ragged(n: int, seed: int) -> list[int]:
    """feed lengths adding up to n: empty and one-sample feeds, spans shorter and longer than a block"""
    rng = np.random.default_rng(seed)
    out, left = [], n
    head = [1, 0, 2, 100, 101, 0, 333]
    k = 0
    while left > 0:
        m = head[k] if k < len(head) else int(rng.choice([0, 1, 7, int(rng.integers(1, 300)), int(rng.integers(1, 1500)), int(rng.integers(1, 4000))]))
        m = min(m, left)
        out.append(m); left -= m; k += 1
    return out


def make_cases() -> list[dict]:
    cases = []

    def add(name, cfg, sync, sig, n, splits=None, **expect):
        seed = 100 + len(cases)
        cases.append({"name": name, "cfg": cfg, "sync": sync, "sig": sig, "n": n, "seed": seed, "splits": splits or _ragged(n, seed), "expect": expect})

    am2 = lambda f0, **kw: dict({"kind": "am2", "f0": f0}, **kw)
    # the three operations at the three carrier offsets, Bandpass on and off, three audio rates, in_rate equal to it or twice it.  -170 Hz
    # (and +30 Hz, later) takes the loop's phase past two pi: the saturation branches
    add("dsb_0", _cfg(8000, 8000), (1, DSB, 0, 0.0), am2(0.0), 9000, locked=True)
    add("usb_0_bp", _cfg(8000, 8000, bp=1), (1, USB, 0, 0.0), am2(0.0), 7000, locked=True)
    add("lsb_0", _cfg(12000, 6000, nco_freq=-1500), (1, LSB, 0, 0.0), am2(1500.0), 14000, locked=True)
    add("dsb_p30_bp", _cfg(16000, 8000, nco_freq=-2000, bp=1), (1, DSB, 0, 0.0), am2(2030.0), 19000, sat=True)
    add("usb_p30", _cfg(6000, 6000), (1, USB, 0, 0.0), am2(30.0), 7000, sat=True)
    add("lsb_p30_bp", _cfg(6000, 6000, bp=1), (1, LSB, 0, 0.0), am2(30.0), 6000, sat=True)
    add("dsb_m170", _cfg(4000, 4000, rf=2000.0), (1, DSB, 0, 0.0), am2(-170.0, fu=250.0, fl=420.0), 7000, sat=True)
    add("usb_m170_bp", _cfg(12000, 6000, nco_freq=1000, bp=1), (1, USB, 0, 0.0), am2(-1170.0), 12000, sat=True)
    add("lsb_m170", _cfg(8000, 8000), (1, LSB, 0, 0.0), am2(-170.0), 7000, sat=True)
    # SSBFilter designed once from other values than the channel's: the same stream through a filter made from the channel's own
    add("usb_design_default", _cfg(8000, 8000, vol=2.0), (1, USB, 0, 0.0), am2(0.0, fu=900.0, fl=300.0), 6000)
    add("usb_design_own", _cfg(8000, 8000, vol=2.0), (1, USB, 8000, 3000.0), am2(0.0, fu=900.0, fl=300.0), 6000)
    # squelch gating: a closure in the middle of a block and a reopening; muted; never open
    gap = am2(0.0, runs=[3000, 1500, 4500], amps=[6000.0, 20.0])
    add("usb_reopen", _cfg(8000, 8000), (1, USB, 0, 0.0), gap, 9000, reopens=True)
    add("dsb_reopen_bp", _cfg(8000, 8000, bp=1), (1, DSB, 0, 0.0), am2(30.0, runs=[2500, 1200, 5300], amps=[6000.0, 20.0]), 9000, reopens=True)
    add("lsb_muted", _cfg(8000, 8000, mute=1), (1, LSB, 0, 0.0), am2(0.0), 3000, never_open=True)
    add("dsb_never_open", _cfg(8000, 8000, sq=-10.0), (1, DSB, 0, 0.0), am2(0.0, amp=300.0), 3000, never_open=True)
    add("usb_noise", _cfg(8000, 8000, sq=-100.0), (1, USB, 0, 0.0), {"kind": "noise_full"}, 5000, locked=False)
    # block edges: a constant-amplitude carrier from the first sample with the squelch at -100 dB opens at audio index rate / 20 - 1 (the
    # counter reaches rate / 20 on the 400th sample), so 399 inputs bring no open sample and the feeds behind them are all open: a feed
    # shorter than a block, one of exactly B, B - 1, B + 1
    for op in (USB, DSB):
        B = block(op)
        edges = [399, 100, B - 100, B, B - 1, B + 1, 1, B - 1, 3]
        add(f"{OPS[op]}_block_edges", _cfg(8000, 8000, sq=-100.0), (1, op, 0, 0.0), am2(0.0, noise=0.0), sum(edges) + B + 77, splits=edges + [B + 77],
            edges=True)
    # the host check's trace (tests/test_am_sync_host.py): short, so that the per-sample recording stays small
    add("trace_usb_m170", _cfg(4000, 4000, rf=2000.0), (1, USB, 0, 0.0), am2(-170.0, fu=250.0, fl=420.0), 2500, trace=True, sat=True)
    for c in cases:
        assert sum(c["splits"]) == c["n"], c["name"]
        assert c["n"] <= 20000
    return cases


CASES = make_cases()
BY = {c["name"]: c for c in CASES}


def inputs(case: dict) -> np.ndarray:
    return signal(case["sig"], case["n"], case["cfg"][0], case["seed"])


def sha(a: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
