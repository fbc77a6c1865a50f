"""Cases of the LoRa demodulator bank (sdrx_lora_*) and the ctypes face of tests/lora_oracle.cpp, shared by the golden recorder
tests/golden/make_golden_lora.py, tests/test_lora_gpu.py, tests/test_lora_golden.py, tests/test_lora_host.py,
tests/test_lora_oracle.py (CPU) and tests/test_lora_random_gpu.py.

A case is a demodulator configuration, a signal at the channel rate and the lengths of the feeds it is cut into:
    cfg = (in_rate, nco_freq, bandwidth)
    sig = {"kind": "zero" | "noise_full" | "frames" | "frames_x" | "const" | "pm1" | "noise", ...}   see signal()

The oracle (OracleLora, build_oracle(), run_oracle()) is LoRaDemod::feed in plain scalar code, built on the fly with strict-IEEE
flags and linked to oracle/libsdro.so for the front; it needs neither the reference tree nor Qt, so it gives the expected output
of any input where the GPU is.  It is tied to the reference by tests/test_lora_oracle.py: equal to the recording lora_golden.npz
on CASES; equal to the recorder, feed by feed, on random_cases() and NAMED where the reference is present; and equal to the
recorder's digests of those cases in tests/golden/lora_random_golden.npz anywhere.

CASES are the thirteen recorded ones.  random_cases() are 100 seeded draws of rates (listed and unlisted bandwidths, bandwidth 1,
ratios 1, 2 .. 4, non-integer, and 17 .. 66), NCO offsets (zero, small, next to +- in_rate / 2), signals (frames of random shape
at 3 units to clipped full scale in noise up to the amplitude, with a down-chirped copy, real-only; a constant, -1 / 0 / 1 noise,
noise, silence) and cuts (_ragged or one feed); what they reach is asserted by assert_coverage().  NAMED are the cases with two
and three lines in one feed (LINE_CASES) and a tie above zero (TIE_CASE).

The `frames` signal is built on the time axis of the decimator's output (one unit per output sample) and evaluated at the input
rate.  Symbol s is exp(j 2 pi (A(t) / 256 + s t / 256)) over 256 units with A(t) = (t + 1)(t + 2) / 2, which at whole t is the
cumulative sum of 1 .. 256 the demodulator's dechirp runs through; from the whole t at which the instantaneous frequency passes
half a cycle per unit on, one cycle per unit is taken off, which changes nothing at whole t and keeps the signal inside the
channel between them.  A frame is `pre` symbols of s = 0, data symbols s = 4 k with k in 0 .. 63, and `down` conjugated symbols
that close the squelch; the frame is rotated by `rot` units so that the preamble lands off bin 0 (the decimator's own delay, 36
input samples, counts against it).  Amplitude 0.2 of full scale,
Gaussian noise of sigma 0.01 of full scale.  What each case is for (`expect`) is asserted by the maker on the recording itself."""
from __future__ import annotations

import ctypes as C
import hashlib
import os
import subprocess
import tempfile

import numpy as np

from tests.wfm_cases import _clip16, _gauss, _splitmix, _uniform_i16, cut  # noqa: F401  (cut is re-exported)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_SRC = os.path.join(ROOT, "tests", "lora_oracle.cpp")
ORACLE_DIR = os.path.join(ROOT, "oracle")
CSRC = os.path.join(ROOT, "sdrangel_amd", "csrc")
RANDOM_GOLDEN = os.path.join(ROOT, "tests", "golden", "lora_random_golden.npz")

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


def _frames_z(sig: dict, n: int, cfg, seed: int) -> np.ndarray:
    """the frames of `sig` as unit-amplitude complex samples at the input rate, before the NCO's offset"""
    in_rate, _, bw = cfg
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
    return z


def signal(sig: dict, n: int, cfg, seed: int) -> np.ndarray:
    """kinds: zero; noise_full (uniform over the int16 range); frames (amplitude AMP, noise SIGMA); and for the random cases
    frames_x: frames at amplitude `amp` (int16 units, clipped past full scale) in Gaussian noise of `sigma`, with `down` times
        the conjugate -- a down-chirped copy of the same frames -- added, and the imaginary part dropped when `real` is set;
    const: the sample (i, q) throughout;  pm1: I and Q uniform over -1, 0, 1;  noise: Gaussian of `sigma`"""
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
    if kind == "const":
        iq[0::2] = sig["i"]
        iq[1::2] = sig["q"]
        return iq
    if kind == "pm1":
        iq[0::2] = (_splitmix(seed, n, 1) % np.uint64(3)).astype(np.int16) - 1
        iq[1::2] = (_splitmix(seed, n, 2) % np.uint64(3)).astype(np.int16) - 1
        return iq
    if kind == "noise":
        iq[0::2] = _clip16(_gauss(seed, n, 3, float(sig["sigma"])))
        iq[1::2] = _clip16(_gauss(seed, n, 4, float(sig["sigma"])))
        return iq
    assert kind in ("frames", "frames_x"), kind
    z = _frames_z(sig, n, cfg, seed)
    amp, sigma = AMP, SIGMA
    if kind == "frames_x":
        amp, sigma = float(sig["amp"]), float(sig["sigma"])
        if sig.get("down"):
            z = z + float(sig["down"]) * np.conj(z)
    if nco_freq:
        m = np.arange(n, dtype=np.float64)
        z *= np.exp(-2j * np.pi * nco_actual(nco_freq, in_rate) * m / in_rate)      # the NCO turns it back
    iq[0::2] = _clip16(amp * z.real + _gauss(seed, n, 3, sigma))
    iq[1::2] = _clip16(amp * z.imag + _gauss(seed, n, 4, sigma)) if not sig.get("real") else 0
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


# ---------------------------------------------------------------- oracle
STATE = ("tune", "time", "result", "bin", "count", "lines")
EVENTS = ("tuned_up", "tuned_plain", "short_closes", "locks", "wraps")
PROBES = ("max_lines_in_feed", "squelch_near", "ties")


def build_oracle() -> C.CDLL:
    so = os.path.join(tempfile.mkdtemp(), "liblro.so")
    if not os.path.exists(os.path.join(ORACLE_DIR, "libsdro.so")):
        subprocess.check_call(["make", "-C", ORACLE_DIR, "libsdro.so"])
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-I" + CSRC, ORACLE_SRC, "-o", so,
                           "-L" + ORACLE_DIR, "-lsdro", "-Wl,-rpath," + ORACLE_DIR, "-lm"])
    L = C.CDLL(so)
    L.lro_create.restype = C.c_void_p
    L.lro_create.argtypes = [C.c_int, C.c_int, C.c_int]
    L.lro_destroy.argtypes = [C.c_void_p]
    L.lro_feed.restype = C.c_long
    L.lro_feed.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_void_p, C.c_long]
    L.lro_text.restype = C.c_long
    L.lro_text.argtypes = [C.c_void_p, C.c_void_p, C.c_long]
    L.lro_state.argtypes = [C.c_void_p, C.c_void_p]
    L.lro_design.restype = C.c_int
    L.lro_design.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_void_p, C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    return L


class OracleLora:
    def __init__(self, L: C.CDLL, cfg):
        self.L = L
        self.h = L.lro_create(int(cfg[0]), int(cfg[1]), int(cfg[2]))
        assert self.h

    def feed(self, iq: np.ndarray):
        """(Samples [n, 2] of re, im; the text dumpRaw printed during this feed)"""
        iq = np.ascontiguousarray(iq, np.int16)
        n = iq.size // 2
        out = np.empty((n + 1, 2), np.int16)                    # the step is at least 1: at most one Sample per input
        k = self.L.lro_feed(self.h, iq.ctypes.data, n, out.ctypes.data, n + 1)
        assert k <= n
        buf = C.create_string_buffer(256 * (k // 4544 + 2))
        nb = self.L.lro_text(self.h, buf, len(buf))
        assert nb <= len(buf)
        return out[:k].copy(), buf.raw[:nb].decode("latin-1")

    def counters(self) -> dict:
        """the six state values, the five event counters and the three probes"""
        v = np.zeros(14, np.int64)
        self.L.lro_state(self.h, v.ctypes.data)
        return dict(zip(STATE + EVENTS + PROBES, (int(x) for x in v)))

    def design(self):
        """in the layout of sdrx_lora_get_design: (taps per phase, taps [16 * ntaps], NCO increment, vrot as 256 floats, k2, the
        dechirp table as 512 floats, the Sample table as [128, 2] int16)"""
        taps, vrot, chirp = np.zeros(16 * 128, np.float32), np.zeros(256, np.float32), np.zeros(512, np.float32)
        sample = np.zeros((128, 2), np.int16)
        inc, k2 = C.c_int32(), C.c_float()
        nt = self.L.lro_design(self.h, taps.ctypes.data, C.byref(inc), vrot.ctypes.data, C.byref(k2), chirp.ctypes.data, sample.ctypes.data)
        return nt, taps[: 16 * nt].copy(), inc.value, vrot, k2.value, chirp, sample

    def close(self):
        if self.h:
            self.L.lro_destroy(self.h)
            self.h = None

    __del__ = close


def run_spans(L: C.CDLL, cfg, spans) -> dict:
    """the oracle over a list of feeds: per feed the Samples, the text and the counters (state, events and probes so far)"""
    o = OracleLora(L, cfg)
    feeds, texts, counters = [], [], []
    for x in spans:
        s, t = o.feed(x)
        feeds.append(s); texts.append(t); counters.append(o.counters())
    o.close()
    return {"feeds": feeds, "texts": texts, "counters": counters}


def run_oracle(L: C.CDLL, case: dict, splits=None) -> dict:
    return run_spans(L, case["cfg"], cut(inputs(case), splits or case["splits"]))


def state_list(counters: dict) -> list[int]:
    return [counters[k] for k in STATE]


# ---------------------------------------------------------------- random cases
#: bandwidths LoRaDemodSettings does not list: primes, odd and even ones
OTHER_BANDWIDTHS = (9973, 12345, 25000, 33333, 41667, 50021, 4999, 10000)
N_CAP = 79999


def _units(frames, lead=0, tail=300) -> int:
    return lead + sum(256 * (f["pre"] + f["data"] + f["down"]) + f["gap"] for f in frames) + tail


def _rates(rng, i):
    """(in_rate, bandwidth) of random case i.  Every tenth case has a ratio above 16 (500000 / 7813 first, up to 70); case 41 is
    bandwidth 1 in in_rate 3, which the recorder and sdrx_lora_create both accept (1 is the smallest either takes); the others
    are bandwidth == in_rate, an integer ratio or a non-integer one up to 4"""
    bw = int(rng.choice(BANDWIDTHS + OTHER_BANDWIDTHS))
    how = int(rng.integers(0, 5))
    frac = float(rng.random())
    if i == 41:
        return 3, 1
    if i % 10 == 3:
        if i == 3:
            return 500000, 7813
        bw = int(rng.choice((4999, 7813, 9973, 10000)))
        return int(bw * (17.0 + 53.0 * frac)), bw
    if how <= 1:
        return bw, bw
    if how == 2:
        return bw * int(rng.choice((2, 3, 4))), bw
    return int(bw * (1.0 + 3.0 * frac)) + 1, bw


def _nco(rng, in_rate: int) -> int:
    """zero, small, or within 50 of +- in_rate / 2"""
    how, small, near, sign = int(rng.integers(0, 4)), int(rng.integers(1, 2000)), int(rng.integers(0, 50)), int(rng.choice((-1, 1)))
    if how == 0 or in_rate < 8:
        return 0
    if how == 3:
        return sign * max(in_rate // 2 - near, 0)
    return sign * min(small, in_rate // 2 - 1)


def random_case(rng, i) -> dict:
    """one random configuration, signal and split list; the order of the rng calls is part of the case set"""
    in_rate, bw = _rates(rng, i)
    cfg = (in_rate, _nco(rng, in_rate), bw)
    ratio = in_rate / bw
    # frames: pre 4 .. 12, down 0 .. 4, any rotation, lead and gap; data sized so that two frames fit the cap at this ratio.
    # Case 7 runs m_time past 1023 and case 23 into the dump's clip at 140 symbols, both at ratio 1.
    room = int(min(N_CAP, 26000 if ratio <= 4.5 else N_CAP) / ratio)              # decimator outputs the case may span
    nfr = int(rng.integers(1, 3))
    frames = []
    for _ in range(nfr):
        pre, down, rot, gap = int(rng.integers(4, 13)), int(rng.integers(0, 5)), int(rng.integers(0, 256)), int(rng.integers(0, 1500))
        most = max(2, min(60, (room // nfr - 700) // 256 - pre - down))
        frames.append(frame(int(rng.integers(2, most + 1)), rot, pre=pre, down=down, gap=gap))
    lead = int(rng.integers(0, 2000))
    amp = float(np.round(3.0 * (15000.0 ** float(rng.random()))))                  # 3 .. 45000 units: clipped past 32767
    sigma = float(np.round(amp * float(rng.choice((0.0, 0.01, 0.1, 0.3, 1.0)))))
    down_level = float(np.round(0.2 + float(rng.random()), 2))                     # 0.2 .. 1.2
    misc = (i // 10) % 7                                                             # every other kind in turn
    whole = float(rng.random()) < 0.2
    if i in (7, 23):
        cfg = (bw, 0, bw)
        frames, lead = [frame(270 if i == 7 else 150, frames[0]["rot"], pre=frames[0]["pre"], down=max(frames[0]["down"], 1))], 0
        sig = {"kind": "frames_x", "frames": frames, "lead": lead, "amp": max(amp, 50.0), "sigma": min(sigma, 0.1 * max(amp, 50.0))}
    elif i % 10 == 5:
        sig = {"kind": "frames_x", "frames": frames, "lead": lead, "amp": amp, "sigma": sigma, "down": down_level}
    elif i % 10 == 8:
        sig = [{"kind": "const", "i": int(amp) % 30000, "q": -(int(sigma) % 30000)}, {"kind": "pm1"}, {"kind": "noise_full"}, {"kind": "zero"},
               {"kind": "noise", "sigma": max(amp, 1.0)}, {"kind": "frames_x", "frames": frames, "lead": lead, "amp": amp, "sigma": sigma, "real": 1},
               {"kind": "frames_x", "frames": frames, "lead": lead, "amp": amp, "sigma": sigma, "real": 1}][misc]
    else:
        sig = {"kind": "frames_x", "frames": frames, "lead": lead, "amp": amp, "sigma": sigma}
    if "frames" in sig:
        n = min(samples_for(cfg, _units(sig["frames"], lead=sig["lead"])), N_CAP if ratio > 4.5 or i in (7, 23) else 26000)      # cut short if need be
    else:
        n = min(int(3000 * max(1.0, ratio)), N_CAP)
    seed = 5000 + i
    return {"name": f"random{i}", "cfg": cfg, "sig": sig, "n": n, "seed": seed, "splits": [n] if whole else _ragged(n, seed)}


#: the seed of random_cases(): the cases the `ref` test of tests/test_lora_oracle.py proves against the recorder and
#: tests/golden/lora_random_golden.npz keeps the recorder's digests of
RANDOM_SEED = 20261021


def random_cases(count: int = 100) -> list[dict]:
    """the first `count` random cases, drawn in order from one generator"""
    rng = np.random.default_rng(RANDOM_SEED)
    return [random_case(rng, i) for i in range(count)]


def assert_coverage(cases, counters, texts, probes: bool):
    """what the random cases have to reach, on the counters after each case's last feed (the oracle's, or the recorder's five
    events with state: then probes is False and squelch_near, which the recorder does not count, is left out) and each case's
    whole text"""
    count = lambda f: sum(1 for k in counters if f(k))
    assert count(lambda k: k["locks"] > 0) >= 20 and count(lambda k: k["lines"] > 0) >= 10
    assert count(lambda k: k["locks"] == 0) >= 1
    for key in ("tuned_up", "tuned_plain", "short_closes", "wraps"):
        assert sum(k[key] for k in counters) >= 1, key
    assert any(len(line) == 140 // 2 - 1 for t in texts for line in t.split("\n")), "no dump clipped at 140 symbols"
    if probes:
        assert count(lambda k: k["squelch_near"] >= 1) >= 5
    assert len({c["cfg"][2] for c in cases}) >= 10
    assert sum(1 for c in cases if c["cfg"][0] / c["cfg"][2] > 16) >= 5 and max(c["cfg"][0] / c["cfg"][2] for c in cases) >= 64
    assert sum(c["n"] for c in cases) < 2500000 and all(c["n"] < 80000 for c in cases)


# ---------------------------------------------------------------- more than one line in a feed
def make_line_cases() -> list[dict]:
    """Named cases for the text slots (lora_synch's slot *n_lines, read_text's join, lora_lines_bound): all at step 1 from a
    fresh start, so that input sample k is decimator output k and the fetches fall on inputs 63, 127, ...

    A line needs m_time > 70 at the closure, 71 fetches after the lock, so a feed of n outputs from a fresh start ends at most
    n / 4544 lines and stays two under lora_lines_bound(n) = n / 4544 + 2.  The bound's last slot is for a line whose m_time
    was run up before the feed began: `three_lines_late` feeds the first frame up to its last data symbol first, and the
    closure of all three lines then falls in one feed, one under its bound."""
    cfg = (15625, 0, 15625)
    cases = []

    def add(name, frames, splits=None, lead=100, tail=300, seed=0):
        n = samples_for(cfg, _units(frames, lead=lead, tail=tail))
        sig = {"kind": "frames", "frames": frames, "lead": lead}
        cases.append({"name": name, "cfg": cfg, "sig": sig, "n": n, "seed": 700 + seed, "splits": splits(n) if splits else [n]})

    two = [frame(25, 37, gap=700), frame(28, 90)]
    add("two_lines_one_feed", two, seed=1)
    three = short_frames(SHORT_DATA)
    add("three_lines_one_feed", three, tail=100, seed=2)
    add("three_lines_late", three, splits=lambda n: [LATE_CUT, n - LATE_CUT], tail=100, seed=2)
    add("three_lines_short_feed", three, splits=lambda n: [SECOND_LINE_AT - 40, 50, n - SECOND_LINE_AT - 10], tail=100, seed=2)
    for c in cases:
        assert sum(c["splits"]) == c["n"] < 80000, c["name"]
    return cases


#: the short frame of the three-line cases: the fewest data symbols after a preamble of SHORT_PRE with which all three frames
#: run m_time past 70 before the single down-chirp closes the squelch (one fewer and only the first dumps:
#: tests/test_lora_oracle.py::test_short_frames_are_just_long_enough)
SHORT_PRE, SHORT_DATA = 6, 16
#: the input sample (= decimator output) whose fetch ends the second line of the three-line stream, and a cut between the
#: fetch that takes the first frame's m_time past 70 and the one that ends its line (both asserted on the oracle's counters in
#: tests/test_lora_oracle.py)
SECOND_LINE_AT, LATE_CUT = 11711, 5800


def short_frames(data: int) -> list[dict]:
    return [frame(data, rot, pre=SHORT_PRE, down=1, gap=0) for rot in (37, 90, 201)]


LINE_CASES = make_line_cases()

#: a tie above zero, found among the random draws and kept by name: four units of amplitude and no noise, so that the magnitudes
#: are sums of few small integers' products; one fetch has its largest value at two indices, and the first has to win
TIE_CASE = {"name": "tie_above_zero", "cfg": (128063, 64018, 50021),
            "sig": {"kind": "frames_x", "frames": [frame(48, 105, pre=10, down=4, gap=873)], "lead": 1983, "amp": 4.0, "sigma": 0.0},
            "n": 48724, "seed": 5054, "splits": _ragged(48724, 5054)}
NAMED = LINE_CASES + [TIE_CASE]
