"""Cases of the LoRa demodulator bank (sdrx_lora_*), shared by the golden recorder tests/golden/make_golden_lora.py,
tests/test_lora_gpu.py, tests/test_lora_golden.py and tests/test_lora_host.py.

A case is a demodulator configuration, a signal at the channel rate and the lengths of the feeds it is cut into:
    cfg = (in_rate, nco_freq, bandwidth)
    sig = {"kind": "zero" | "noise_full" | "frames", ...}   see signal()

The `frames` signal is built on the time axis of the decimator's output (one unit per output sample) and evaluated at the input
rate.  Symbol s is exp(j 2 pi (A(t) / 256 + s t / 256)) over 256 units with A(t) = (t + 1)(t + 2) / 2, which at whole t is the
cumulative sum of 1 .. 256 the demodulator's dechirp runs through; from the whole t at which the instantaneous frequency passes
half a cycle per unit on, one cycle per unit is taken off, which changes nothing at whole t and keeps the signal inside the
channel between them.  A frame is `pre` symbols of s = 0, data symbols s = 4 k with k in 0 .. 63, and `down` conjugated symbols
that close the squelch; the frame is rotated by `rot` units so that the preamble lands off bin 0 (the decimator's own delay, 36
input samples, counts against it).  Amplitude 0.2 of full scale,
Gaussian noise of sigma 0.01 of full scale.  What each case is for (`expect`) is asserted by the maker on the recording itself."""
from __future__ import annotations

import hashlib

import numpy as np

from tests.wfm_cases import _clip16, _gauss, _uniform_i16, cut  # noqa: F401  (cut is re-exported)

BANDWIDTHS = (7813, 15625, 20833, 31250, 62500)     # LoRaDemodSettings::bandwidths
AMP, SIGMA = 0.2 * 32768.0, 0.01 * 32768.0


def nco_actual(nco_freq: int, in_rate: int) -> float:
    """the frequency NCO::setFreq really turns by: the table increment is truncated"""
    return int(np.float32(np.float32(nco_freq) * np.float32(4096)) / np.float32(in_rate)) * in_rate / 4096.0


def symbols(frame: dict, seed: int) -> list[int]:
    """the data symbols k of a frame; one that equals the symbol three before it while that one is repeated next to it would pass
    the preamble test again (bin == history[t - 6] == history[t - 12]), so such draws are taken again"""
    rng = np.random.default_rng(seed)
    out: list[int] = []
    while len(out) < frame["data"]:
        k = int(rng.integers(0, 64))
        if len(out) >= 1 and k == out[-1]:
            continue
        if len(out) >= 2 and k == out[-2]:
            continue
        if len(out) >= 3 and k == out[-3]:
            continue
        out.append(k)
    return out


def _frame_phase(frame: dict, seed: int):
    """(symbol value s per symbol, +1 / -1 per symbol) of one frame"""
    s = [0] * frame["pre"] + [4 * k for k in symbols(frame, seed)] + [0] * frame["down"]
    sign = [1] * (frame["pre"] + frame["data"]) + [-1] * frame["down"]
    return np.array(s, np.float64), np.array(sign, np.float64)


def _chirp(t: np.ndarray, s: np.ndarray) -> np.ndarray:
    """cycles of symbol value s at time t in [0, 256) of the symbol"""
    ph = ((t + 1.0) * (t + 2.0) / 2.0 + s * t) / 256.0
    tw = np.ceil(126.5 - s)                          # (t + 1.5 + s) / 256 passes 1 / 2 at t = 126.5 - s; s up to 252: also at 382.5 - s
    tw2 = np.ceil(382.5 - s)
    ph = ph - np.where(t >= tw, t - tw, 0.0) - np.where(t >= tw2, t - tw2, 0.0)
    return ph


def signal(sig: dict, n: int, cfg, seed: int) -> np.ndarray:
    in_rate, nco_freq, bw = cfg
    kind = sig["kind"]
    iq = np.empty(2 * n, np.int16)
    if kind == "zero":
        iq[:] = 0
        return iq
    if kind == "noise_full":
        iq[0::2] = _uniform_i16(seed, n, 1)
        iq[1::2] = _uniform_i16(seed, n, 2)
        return iq
    assert kind == "frames"
    m = np.arange(n, dtype=np.float64)
    tau = m * (float(bw) / float(in_rate))           # decimator-output units
    z = np.zeros(n, np.complex128)
    start = float(sig.get("lead", 0))
    for i, fr in enumerate(sig["frames"]):
        s, sign = _frame_phase(fr, seed * 31 + i)
        length = 256.0 * s.size
        inside = (tau >= start) & (tau < start + length)
        u = np.mod(tau[inside] - start + float(fr["rot"]), length)          # the frame rotated by `rot` units
        k = np.minimum((u // 256.0).astype(np.int64), s.size - 1)
        ph = _chirp(u - 256.0 * k, s[k])
        z[inside] = np.exp(2j * np.pi * ph * sign[k])
        start += length + float(fr.get("gap", 0))
    if nco_freq:
        z *= np.exp(-2j * np.pi * nco_actual(nco_freq, in_rate) * m / in_rate)      # the NCO turns it back
    iq[0::2] = _clip16(AMP * z.real + _gauss(seed, n, 3, SIGMA))
    iq[1::2] = _clip16(AMP * z.imag + _gauss(seed, n, 4, SIGMA))
    return iq


def _ragged(n: int, seed: int) -> list[int]:
    """feed lengths adding up to n: empty and one-sample feeds, spans shorter and longer than a fetch and than the delay"""
    rng = np.random.default_rng(seed)
    out, left = [], n
    head = [1, 0, 2, 61, 64, 0, 333]
    k = 0
    while left > 0:
        m = head[k] if k < len(head) else int(rng.choice([0, 1, 63, int(rng.integers(1, 300)), int(rng.integers(1, 3000)), int(rng.integers(1, 9000))]))
        m = min(m, left)
        out.append(m); left -= m; k += 1
    return out


def frame(data: int, rot: int, pre: int = 8, down: int = 3, gap: int = 0) -> dict:
    return {"pre": pre, "data": data, "down": down, "rot": rot, "gap": gap}


def samples_for(cfg, units: int) -> int:
    """input samples that cover `units` decimator outputs"""
    return int(np.ceil(units * cfg[0] / cfg[2])) + 8


def make_cases() -> list[dict]:
    cases = []

    def add(name, cfg, sig, n, splits=None, **expect):
        seed = 300 + len(cases)
        cases.append({"name": name, "cfg": cfg, "sig": sig, "n": n, "seed": seed, "splits": splits or _ragged(n, seed), "expect": expect})

    def frames(*fr, lead=0):
        return {"kind": "frames", "frames": list(fr), "lead": lead}

    def units(*fr, lead=0, tail=300):
        return lead + sum(256 * (f["pre"] + f["data"] + f["down"]) + f["gap"] for f in fr) + tail

    # front variants: step 1, step 2, a non-integer step, an NCO; every bandwidth once.  7813 is the bandwidth whose cutoff
    # float(7813) / 1.9 moves the taps when it passes through a float (tests/test_lora_gpu.py)
    f30 = frame(30, 74)
    add("bw7813_step1", (7813, 0, 7813), frames(f30), samples_for((7813, 0, 7813), units(f30)), locks=1, lines=1)
    add("bw15625_step2", (31250, 0, 15625), frames(frame(30, 21)), samples_for((31250, 0, 15625), units(f30)), locks=1, lines=1)
    add("bw31250_frac", (48000, 0, 31250), frames(frame(30, 50)), samples_for((48000, 0, 31250), units(f30)), locks=1, lines=1)
    add("bw20833_nco", (41666, -3000, 20833), frames(frame(30, 77)), samples_for((41666, -3000, 20833), units(f30)), locks=1, lines=1)
    add("bw62500_step1", (62500, 0, 62500), frames(frame(30, 101)), samples_for((62500, 0, 62500), units(f30)), locks=1, lines=1)
    # silence: every tie resolves to index 0 and the preamble test fires on bin 0; noise: no lock, no line
    add("silence", (15625, 0, 15625), {"kind": "zero"}, 3000, silence=True)
    add("noise", (15625, 0, 15625), {"kind": "noise_full"}, 6000, lines=0)
    # a squelch closure that leaves m_time at or below 70: no dump
    f10 = frame(10, 74)
    add("short_close", (7813, 0, 7813), frames(f10), samples_for((7813, 0, 7813), units(f10)), locks=1, lines=0, short_close=True)
    # a dump clipped at 140 symbols; m_time past 1023
    f150 = frame(150, 60)
    add("clip140", (7813, 0, 7813), frames(f150), samples_for((7813, 0, 7813), units(f150)), locks=1, lines=1, clip=True)
    f270 = frame(270, 21)
    add("time_wrap", (15625, 0, 15625), frames(f270), samples_for((15625, 0, 15625), units(f270)), locks=1, wrap=True)
    # two frames in one stream: two lines and a re-tune in between
    fa, fb = frame(25, 37, gap=700), frame(28, 90)
    add("two_frames", (20833, 0, 20833), frames(fa, fb, lead=200), samples_for((20833, 0, 20833), units(fa, fb, lead=200)), locks=2, lines=2)
    # feeds that end inside, on and just past a fetch (64 outputs) and the delay length (128 outputs) of the stream position
    edges = [0, 1, 62, 1, 1, 62, 1, 1, 0, 63, 64, 65, 1]
    n_e = samples_for((7813, 0, 7813), units(f30))
    add("feed_edges", (7813, 0, 7813), frames(frame(30, 64)), n_e, splits=edges + [n_e - sum(edges)], locks=1, lines=1, edges=True)
    # the host check's trace (tests/test_lora_host.py): as short as a frame with a line can be
    f20 = frame(20, 74)
    add("trace", (7813, 0, 7813), frames(f20), samples_for((7813, 0, 7813), units(f20, tail=100)), locks=1, lines=1, trace=True)
    for c in cases:
        assert sum(c["splits"]) == c["n"], c["name"]
        assert c["n"] < 80000, (c["name"], c["n"])
    return cases


CASES = make_cases()
BY = {c["name"]: c for c in CASES}


def inputs(case: dict) -> np.ndarray:
    return signal(case["sig"], case["n"], case["cfg"], case["seed"])


def sha(a: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
