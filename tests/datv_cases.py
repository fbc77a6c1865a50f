"""Cases of the DATV receiver bank (sdrx_datv_*), their synthetic signals and the portable oracle.

tests/datv_oracle.cpp is a scalar restatement of DATVDemod::feed down to p_symbols, built here with strict IEEE flags and linked to
oracle/libsdro.so for the NCO, g_fft and runFilt; it needs neither the reference tree nor Qt, so it gives the expected output of
any input where the GPU is.

The signal is a symbol train on the sample grid of the channel rate: random points of a unit constellation (the PSKs, rings for
the APSKs, a grid for the QAMs), shaped by a raised-cosine pulse of +-4 symbols, at `sps` samples per symbol with a fractional
start and a rate error (`timing`: the generator's symbol period is sps * (1 + timing)), on a carrier at `f0` Hz that moves by `slope` Hz per sample, with
Gaussian noise.  `lead` samples of silence come first."""
from __future__ import annotations

import ctypes as C
import hashlib
import os
import subprocess
import tempfile

import numpy as np

from tests.wfm_cases import _clip16, _gauss, _uniform_i16, cut  # noqa: F401  (cut is re-exported)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_SRC = os.path.join(ROOT, "tests", "datv_oracle.cpp")
ORACLE_DIR = os.path.join(ROOT, "oracle")
CSRC = os.path.join(ROOT, "sdrangel_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "datv_golden.npz")
RANDOM_GOLDEN = os.path.join(ROOT, "tests", "golden", "datv_random_golden.npz")

BPSK, QPSK, PSK8, APSK16, APSK32, APSK64E, QAM16, QAM64, QAM256 = range(9)
FEC12, FEC23, FEC46, FEC34, FEC56, FEC78, FEC45, FEC89, FEC910 = range(9)
NEAREST, LINEAR, RRC = range(3)

CFG_FIELDS = (("msps", "i"), ("sample_rate", "i"), ("centre_frequency", "i"), ("rf_bandwidth", "i"), ("symbol_rate", "i"), ("modulation", "i"),
              ("fec", "i"), ("standard", "i"), ("sampler", "i"), ("rolloff", "f"), ("excursion", "i"), ("hard_metric", "i"), ("viterbi", "i"),
              ("allow_drift", "i"), ("notch_filters", "i"), ("finfo", "f"))
STATE_WORDS = ("mu", "phase", "freqw", "agc_gain", "est_insp", "est_sp", "est_ep", "meas_count", "update_freq_phase")
DESIGN_FLOATS = ("omega", "min_omega", "max_omega", "min_freqw", "max_freqw", "freq_beta")
DESIGN_INTS = ("meas_decimation", "rrc_steps", "ncoeffs", "readahead", "nsymbols", "nco_inc")
#: the oracle's branch counters, in the order of tests/datv_oracle.cpp's HIT_ enum
HITS = ("clamp_low", "clamp_high", "drift_reset", "two_meas", "no_symbol", "mu_negative", "halved", "max_halvings", "coeffs_rebuilt",
        "fewer_taps", "symbols", "max_taps")


class Cfg(C.Structure):
    """sdrx_datv_cfg"""
    _fields_ = [(k, C.c_int32 if t == "i" else C.c_float) for k, t in CFG_FIELDS]


class State(C.Structure):
    """sdrx_datv_state_t"""
    _fields_ = [(k, C.c_uint32) for k in STATE_WORDS[:8]] + [("update_freq_phase", C.c_int32), ("hist_p", C.c_uint32 * 6), ("hist_c", C.c_uint32 * 6),
                                                             ("held", C.c_int32), ("chunks", C.c_int64), ("n_in", C.c_int64), ("n_symbols", C.c_int64)]


class Design(C.Structure):
    """sdrx_datv_design_t"""
    _fields_ = [(k, C.c_float) for k in DESIGN_FLOATS] + [(k, C.c_int32) for k in DESIGN_INTS]


class Meas(C.Structure):
    """sdrx_datv_meas_t"""
    _fields_ = [(k, C.c_float) for k in ("freq", "ss", "mer", "est_insp", "est_sp", "est_ep")]


MEAS_DTYPE = np.dtype([(k, np.uint32) for k in ("freq", "ss", "mer", "est_insp", "est_sp", "est_ep")])


def state_words(st) -> list[int]:
    """every field of a state struct (the oracle's or the bank's), in order; update_freq_phase as its 32 bits"""
    return ([int(getattr(st, k)) & 0xffffffff for k in STATE_WORDS] + [int(v) for v in st.hist_p] + [int(v) for v in st.hist_c]
            + [int(st.held), int(st.chunks), int(st.n_in), int(st.n_symbols)])


def design_words(d) -> list[int]:
    """the design as integers: the floats as their bits"""
    return [int(np.float32(getattr(d, k)).view(np.uint32)) for k in DESIGN_FLOATS] + [int(getattr(d, k)) for k in DESIGN_INTS]


def cfg(**kw) -> dict:
    """1 MS/s, QPSK 1/2 at 250 kS/s, the RRC sampler at the reference's defaults, a measurement every 300 samples"""
    d = dict(msps=1000000, sample_rate=1000000, centre_frequency=0, rf_bandwidth=512000, symbol_rate=250000, modulation=QPSK, fec=FEC12,
             standard=0, sampler=RRC, rolloff=0.35, excursion=10, hard_metric=0, viterbi=0, allow_drift=0, notch_filters=0, finfo=1000000 / 300.0)
    d.update(kw)
    return d


def as_struct(k: dict, cls=Cfg):
    return cls(**{name: (int(k[name]) if t == "i" else float(k[name])) for name, t in CFG_FIELDS})


# ---------------------------------------------------------------- the signal
def unit_points(mod: int) -> np.ndarray:
    if mod == BPSK:
        return np.exp(1j * np.pi * (np.array([1, 5]) / 4))
    if mod in (QPSK, PSK8):
        m = 4 if mod == QPSK else 8
        return np.exp(1j * 2 * np.pi * (np.arange(m) + 0.5) / m)
    if mod in (APSK16, APSK32, APSK64E):
        rings = {APSK16: [(4, 0.4), (12, 1.1)], APSK32: [(4, 0.3), (12, 0.75), (16, 1.3)], APSK64E: [(4, 0.2), (12, 0.5), (20, 0.85), (28, 1.3)]}[mod]
        return np.concatenate([r * np.exp(1j * 2 * np.pi * (np.arange(m) + 0.5) / m) for m, r in rings])
    m = {QAM16: 4, QAM64: 8, QAM256: 16}[mod]
    g = np.arange(m) - (m - 1) / 2
    pts = (g[:, None] + 1j * g[None, :]).ravel()
    return pts / np.sqrt(np.mean(np.abs(pts) ** 2))


def signal(sig: dict, k: dict, n: int, seed: int) -> np.ndarray:
    kind = sig["kind"]
    iq = np.zeros(2 * n, np.int16)
    if kind == "zero":
        return iq
    if kind == "noise":
        iq[0::2], iq[1::2] = _uniform_i16(seed, n, 1), _uniform_i16(seed, n, 2)
        return iq
    assert kind == "psk", kind
    lead = int(sig.get("lead", 0))
    m = n - lead
    sps = k["sample_rate"] / k["symbol_rate"] * (1.0 + sig.get("timing", 0.0))
    pts = unit_points(k["modulation"])
    nsym = int(m / sps) + 12
    pick = (_uniform_i16(seed, nsym, 5).astype(np.int64) + 32768) % len(pts)
    train = pts[pick]
    t = (np.arange(m) + sig.get("start", 0.3)) / sps            # in symbols
    base = np.floor(t).astype(np.int64)
    beta = 0.35
    acc = np.zeros(m, np.complex128)
    for d in range(-4, 5):
        idx = base + d
        x = t - idx
        den = 1.0 - (2 * beta * x) ** 2
        den = np.where(np.abs(den) < 1e-9, 1e-9, den)
        h = np.sinc(x) * np.cos(np.pi * beta * x) / den
        ok = (idx >= 0) & (idx < nsym)
        acc += np.where(ok, train[np.clip(idx, 0, nsym - 1)] * h, 0.0)
    amp = float(sig.get("amp", 6000.0))
    tt = np.arange(m, dtype=np.float64)
    ph = 2 * np.pi * (sig.get("f0", 0.0) * tt + 0.5 * sig.get("slope", 0.0) * tt * tt) / k["msps"]      # slope: Hz per sample
    z = amp * acc * np.exp(1j * ph)
    sigma = float(sig.get("sigma", 0.0))
    re = z.real + (_gauss(seed, m, 1, sigma) if sigma else 0.0)
    im = z.imag + (_gauss(seed, m, 2, sigma) if sigma else 0.0)
    iq[2 * lead::2], iq[2 * lead + 1::2] = _clip16(re), _clip16(im)
    return iq


def inputs(case: dict) -> np.ndarray:
    return signal(case["sig"], case["cfg"], case["n"], case["seed"])


def sha(a: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _ragged(n: int, seed: int, pieces: int) -> list[int]:
    """a cut of n into `pieces` feeds of seeded lengths, a zero-length one among them"""
    r = (_uniform_i16(seed, pieces - 1, 9).astype(np.int64) + 32768) * n // 65536
    edges = sorted(set([0, n] + [int(v) for v in r]))
    out = [b - a for a, b in zip(edges[:-1], edges[1:])]
    return out[:1] + [0] + out[1:]


def _case(name: str, seed: int, n: int, sig: dict, splits=None, **kw) -> dict:
    return {"name": name, "seed": seed, "n": n, "sig": sig, "cfg": cfg(**kw), "splits": splits or _ragged(n, seed, 5)}


PSK = {"kind": "psk", "sigma": 150.0}
#: a supported code rate per constellation (16APSK and 32APSK have radii for some only)
FEC_OF = {BPSK: FEC12, QPSK: FEC34, PSK8: FEC23, APSK16: FEC34, APSK32: FEC45, APSK64E: FEC56, QAM16: FEC78, QAM64: FEC12, QAM256: FEC910}
MOD_NAMES = ("bpsk", "qpsk", "psk8", "apsk16", "apsk32", "apsk64e", "qam16", "qam64", "qam256")


def _rate(ratio: float, fs: int = 1000000) -> int:
    return int(round(fs / ratio))


CASES = (
    # each sampler
    [_case("nearest", 1, 8000, PSK, sampler=NEAREST), _case("linear", 2, 8000, PSK, sampler=LINEAR), _case("rrc", 3, 8000, PSK, sampler=RRC)]
    # each constellation at a supported rate, the samplers in turn
    + [_case(f"mod_{MOD_NAMES[m]}", 10 + m, 7000, PSK, modulation=m, fec=FEC_OF[m], sampler=(RRC, LINEAR, NEAREST)[m % 3]) for m in range(9)]
    # the radii of the other rates
    + [_case("apsk16_fec910", 20, 6000, PSK, modulation=APSK16, fec=FEC910), _case("apsk32_fec34", 21, 6000, PSK, modulation=APSK32, fec=FEC34, sampler=LINEAR)]
    # the switches, each on (off in the cases above)
    + [_case("hard_metric", 22, 7000, PSK, hard_metric=1), _case("hard_metric_8psk", 23, 7000, PSK, hard_metric=1, modulation=PSK8, fec=FEC23, sampler=LINEAR),
       _case("viterbi", 24, 7000, PSK, viterbi=1), _case("viterbi_off_offset", 25, 9000, dict(PSK, f0=9000.0)),
       _case("viterbi_offset", 26, 9000, dict(PSK, f0=9000.0), viterbi=1),
       _case("allow_drift", 27, 12000, dict(PSK, f0=45000.0), allow_drift=1), _case("allow_drift_nearest", 28, 9000, dict(PSK, f0=-45000.0), allow_drift=1, sampler=NEAREST)]
    # Fs / Fm from 1.2 to 8: rrc_steps from 53 down to 8, taps per symbol from 3 to 63
    + [_case("ratio_1p2_taps3", 30, 7000, PSK, symbol_rate=_rate(1.2), excursion=9, rf_bandwidth=900000),
       _case("ratio_1p2", 31, 7000, PSK, symbol_rate=_rate(1.2), rf_bandwidth=900000),
       _case("ratio_1p5", 32, 7000, PSK, symbol_rate=_rate(1.5), rolloff=0.25, rf_bandwidth=800000),
       _case("ratio_2", 33, 7000, PSK, symbol_rate=500000, rf_bandwidth=700000),
       _case("ratio_2_taps55", 34, 9000, PSK, symbol_rate=500000, rolloff=0.1, excursion=30, rf_bandwidth=700000),
       _case("ratio_3", 35, 8000, PSK, symbol_rate=_rate(3.0), rolloff=0.2, excursion=20),
       _case("ratio_8", 36, 12000, PSK, symbol_rate=125000, rf_bandwidth=300000),
       _case("ratio_8_taps63", 37, 14000, PSK, symbol_rate=125000, excursion=30, rf_bandwidth=300000),
       # the limit itself: 507 coefficients at 8 steps are 64 taps, lane 63 carries one and the window is read at pin + 63
       _case("ratio_8_taps64", 63, 14000, PSK, symbol_rate=125000, excursion=30, rolloff=0.345, rf_bandwidth=300000),
       _case("ratio_8_linear", 38, 12000, PSK, symbol_rate=125000, sampler=LINEAR, rf_bandwidth=300000),
       _case("ratio_1p2_nearest", 39, 6000, PSK, symbol_rate=_rate(1.2), sampler=NEAREST, rf_bandwidth=900000),
       # omega under 1.1: a mucorr of -0.1 takes mu below 0, the FIR starts past `subsampling` and sums fewer taps
       _case("ratio_1p05_mu_negative", 60, 7000, dict(PSK, timing=-0.02), symbol_rate=_rate(1.05), rf_bandwidth=980000),
       _case("ratio_1p05_linear", 61, 7000, dict(PSK, timing=-0.02), symbol_rate=_rate(1.05), rf_bandwidth=980000, sampler=LINEAR)]
    # meas_decimation 100, 128, 300 (the default here) and more than the stream
    + [_case("meas_100", 40, 7000, PSK, finfo=10000.0), _case("meas_128", 41, 7000, PSK, finfo=1000000 / 128.0),
       _case("meas_never", 42, 7000, PSK, finfo=0.0), _case("meas_100_linear", 43, 7000, PSK, finfo=10000.0, sampler=LINEAR)]
    # a carrier offset past the limit: freqw is put back; both signs
    # (a fixed offset past the limit is past the detector's ambiguity too and never pulls freqw there; a carrier that moves does)
    + [_case("drift_reset_down", 44, 20000, dict(PSK, slope=-2.5, sigma=50.0)), _case("drift_reset_up", 45, 20000, dict(PSK, slope=2.5, sigma=50.0), sampler=LINEAR),
       _case("offset_past_limit", 62, 9000, dict(PSK, f0=45000.0)),
       _case("nco_offset", 46, 9000, dict(PSK, f0=100000.0), centre_frequency=100000),
       _case("nco_offset_neg", 47, 9000, dict(PSK, f0=-123456.0), centre_frequency=-123456, sampler=NEAREST)]
    # a timing offset that drives mucorr into both clamps
    + [_case("timing_fast", 48, 12000, dict(PSK, timing=0.03, amp=9000.0)), _case("timing_slow", 49, 12000, dict(PSK, timing=-0.03, amp=9000.0), sampler=LINEAR),
       _case("timing_bpsk", 50, 12000, dict(PSK, timing=0.05), modulation=BPSK, sampler=NEAREST)]
    # inputs that are no signal
    # omega of 300: most chunks have no symbol -- no constellation point, no AGC or estimate update, measurements still counted
    + [_case("omega_300_no_symbol", 64, 9000, PSK, symbol_rate=3333, rf_bandwidth=20000, sampler=NEAREST, finfo=10000.0),
       _case("omega_300_linear", 65, 9000, PSK, symbol_rate=3333, rf_bandwidth=20000, sampler=LINEAR),
       _case("silence", 51, 6000, {"kind": "zero"}), _case("silence_linear", 52, 6000, {"kind": "zero"}, sampler=LINEAR, modulation=BPSK),
       _case("noise", 53, 8000, {"kind": "noise"}), _case("noise_qam256", 54, 8000, {"kind": "noise"}, modulation=QAM256, fec=FEC12, sampler=NEAREST),
       _case("clipped", 55, 8000, dict(PSK, amp=60000.0)),
       # 256 000 samples of silence, then full scale: agc_gain near 10^4, lookup halves about twenty times
       # (64 more, so that the filter's delay of 256 does not put the first full-scale sample at the head of a chunk, behind one that
       # has seen the pulse's precursors only and has let the AGC down already)
       _case("silence_then_full", 56, 256064 + 6000, dict(PSK, lead=256064, amp=30000.0), splits=[100000, 156064, 6000]),
       _case("silence_then_full_nearest", 57, 256064 + 6000, dict(PSK, lead=256064, amp=30000.0), splits=[256064 + 6000], sampler=NEAREST, finfo=0.0)]
    # one feed of everything, and feeds of one sample
    + [_case("one_feed", 58, 9000, PSK, splits=[9000]), _case("tiny_feeds", 59, 1500, PSK, splits=[1] * 40 + [0, 1460], sampler=LINEAR)]
)
BY_NAME = {c["name"]: c for c in CASES}
FULL = 12000            # cases up to this many samples keep their outputs as they are in the fixture


# ---------------------------------------------------------------- oracle
def build_oracle() -> C.CDLL:
    so = os.path.join(tempfile.mkdtemp(), "libdto.so")
    if not os.path.exists(os.path.join(ORACLE_DIR, "libsdro.so")):
        subprocess.check_call(["make", "-C", ORACLE_DIR, "libsdro.so"])
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-I" + CSRC, ORACLE_SRC, "-o", so,
                           "-L" + ORACLE_DIR, "-lsdro", "-Wl,-rpath," + ORACLE_DIR, "-lm"])
    L = C.CDLL(so)
    L.dto_create.restype = C.c_void_p
    L.dto_create.argtypes = [C.c_void_p] * 5
    L.dto_destroy.argtypes = [C.c_void_p]
    L.dto_feed.restype = C.c_long
    L.dto_feed.argtypes = [C.c_void_p, C.c_void_p, C.c_long]
    L.dto_symbols.restype = None
    L.dto_symbols.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    for name in ("dto_points", "dto_meas", "dto_written"):
        getattr(L, name).restype = C.c_long
        getattr(L, name).argtypes = [C.c_void_p, C.c_void_p]
    L.dto_tables.restype = C.c_int
    L.dto_tables.argtypes = [C.c_void_p] * 5
    for name in ("dto_state", "dto_design", "dto_hits"):
        getattr(L, name).restype = None
        getattr(L, name).argtypes = [C.c_void_p, C.c_void_p]
    return L


def empty_tables():
    """(coeffs, trig, lut, symbols) buffers of the sizes the table getters fill"""
    return np.zeros(4096, np.float32), np.zeros(2 * 65536, np.float32), np.zeros(65536 * 8, np.uint8), np.zeros(512, np.int8)


class OracleDatv:
    def __init__(self, L: C.CDLL, k: dict, tables=None):
        """tables: (coeffs, trig, lut, symbols) to run on instead of the oracle's own"""
        self.L, self.k = L, k
        s = as_struct(k)
        if tables is None:
            self.h = L.dto_create(C.byref(s), None, None, None, None)
        else:
            co, tr, lut, sy = tables
            self.h = L.dto_create(C.byref(s), tr.ctypes.data, lut.ctypes.data, sy.ctypes.data, co.ctypes.data if co.size else None)
        assert self.h, k
        self.design = Design()
        L.dto_design(self.h, C.byref(self.design))

    def feed(self, iq: np.ndarray) -> dict:
        """one feed's outputs: cost, symbol, the points, the measurements (as bits) and the state's words"""
        iq = np.ascontiguousarray(iq, np.int16)
        ns = self.L.dto_feed(self.h, iq.ctypes.data, iq.size // 2)
        cost, symbol = np.empty(max(ns, 1), np.int16), np.empty(max(ns, 1), np.uint8)
        self.L.dto_symbols(self.h, cost.ctypes.data, symbol.ctypes.data)
        np_ = self.L.dto_points(self.h, None)
        pts = np.empty(2 * max(np_, 1), np.float32)
        self.L.dto_points(self.h, pts.ctypes.data)
        nm = self.L.dto_meas(self.h, None)
        meas = np.zeros(max(nm, 1), MEAS_DTYPE)
        self.L.dto_meas(self.h, meas.ctypes.data)
        st = State()
        self.L.dto_state(self.h, C.byref(st))
        return {"cost": cost[:ns].copy(), "symbol": symbol[:ns].copy(), "points": pts[:2 * np_].view(np.uint32).copy(), "meas": meas[:nm].copy(),
                "state": state_words(st)}

    def written(self) -> np.ndarray:
        """the filtered samples the last feed handed to the receiver, as float32 (re, im) pairs"""
        n = self.L.dto_written(self.h, None)
        out = np.empty(2 * max(n, 1), np.float32)
        self.L.dto_written(self.h, out.ctypes.data)
        return out[:2 * n].copy()

    def tables(self):
        co, tr, lut, sy = empty_tables()
        nc = self.L.dto_tables(self.h, co.ctypes.data, tr.ctypes.data, lut.ctypes.data, sy.ctypes.data)
        return co[:nc].copy(), tr, lut, sy

    def hits(self) -> dict:
        out = (C.c_int64 * len(HITS))()
        self.L.dto_hits(self.h, out)
        return dict(zip(HITS, (int(v) for v in out)))

    def close(self):
        self.L.dto_destroy(self.h)
        self.h = None


def run_spans(L: C.CDLL, k: dict, spans, tables=None) -> dict:
    o = OracleDatv(L, k, tables)
    feeds = [o.feed(x) for x in spans]
    res = {"feeds": feeds, "hits": o.hits(), "design": design_words(o.design)}
    o.close()
    return res


def run_oracle(L: C.CDLL, case: dict, splits=None, tables=None) -> dict:
    return run_spans(L, case["cfg"], cut(inputs(case), splits or case["splits"]), tables)


def merged(feeds) -> dict:
    """feeds of one stream as one: the concatenated outputs and the last state"""
    return {"cost": np.concatenate([f["cost"] for f in feeds]), "symbol": np.concatenate([f["symbol"] for f in feeds]),
            "points": np.concatenate([f["points"] for f in feeds]), "meas": np.concatenate([f["meas"] for f in feeds]), "state": feeds[-1]["state"]}


def assert_same_feed(got: dict, want: dict, what: str = ""):
    for key in ("cost", "symbol", "points", "meas"):
        assert got[key].shape == want[key].shape and np.array_equal(got[key], want[key]), f"{what}: {key} differs ({got[key].shape} against {want[key].shape})"
    assert got["state"] == want["state"], f"{what}: state {got['state']} against {want['state']}"


def table_digests(tables) -> list[str]:
    return [sha(t) for t in tables]


#: what CASES have to reach, summed over them: counter -> least count
COVERAGE = {"no_symbol": 1, "clamp_low": 1, "clamp_high": 1, "drift_reset": 1, "two_meas": 1, "mu_negative": 1, "halved": 1, "max_halvings": 12,
            "coeffs_rebuilt": 2, "fewer_taps": 1, "symbols": 1, "max_taps": 64}


def assert_coverage(hits_per_case: list[dict]):
    total = {k: (max if k in ("max_halvings", "max_taps") else sum)(h[k] for h in hits_per_case) for k in HITS}
    short = {k: (total[k], v) for k, v in COVERAGE.items() if total[k] < v}
    assert not short, f"branches the cases do not reach (have, need): {short}"
    return total


# ---------------------------------------------------------------- every cut of one stream
CUT_STREAM = _case("cut_stream", 70, 1300, dict(PSK, f0=3000.0), splits=[1300], finfo=10000.0)
CUT_CHANNELS = 130                      # channel i gets i + 1 samples per feed until the stream is through


def cut_lengths(readahead: int) -> list[int]:
    return [1, 127, 128, 129, 511, 512, 513, 640 + readahead - 1, 640 + readahead, 640 + readahead + 1]


def even_cut(n: int, m: int) -> list[int]:
    return [m] * (n // m) + ([n % m] if n % m else [])


# ---------------------------------------------------------------- random configurations
RANDOM_SEED = 20261021


def random_case(rng, i: int) -> dict:
    kind = str(rng.choice(["psk", "psk", "psk", "sweep", "sweep", "timing", "timing", "noise", "clipped"]))
    sampler = int(rng.choice([NEAREST, LINEAR, RRC], p=[0.3, 0.3, 0.4]))
    mod = int(rng.choice(np.arange(9), p=[0.1, 0.3, 0.1, 0.08, 0.08, 0.08, 0.1, 0.08, 0.08]))
    fec = FEC_OF[mod] if mod in (APSK16, APSK32) else int(rng.integers(0, 9))
    msps = int(rng.choice([250000, 1000000, 2000000, 4000000]))
    ratio = float(rng.choice([1.2, 1.5, 2.0, 2.0, 3.0, 4.0, 4.0, 6.0, 8.0]))
    rolloff = float(np.float32(rng.choice([0.2, 0.25, 0.35, 0.35, 0.5])))
    exc = int(rng.choice([9, 10, 10, 15, 20]))
    dec = int(rng.choice([100, 128, 300, 1000, 10 ** 7]))
    half = msps // 2
    centre = int(rng.choice([0, 0, int(rng.integers(-half // 2, half // 2))]))
    drift, viterbi = int(rng.random() < 0.2), int(rng.random() < 0.25)
    n = int(rng.integers(6000, 14001))
    nlim = {BPSK: 2, QPSK: 4, PSK8: 8, APSK16: 12, APSK32: 16}.get(mod, 4)          # update_freq_limits' n
    if kind == "sweep":
        # a carrier that starts at the channel's centre and moves past the drift limit while the loop follows it: the loop needs a
        # phase error of slope * omega^2 * 65536 / (msps * freq_beta * omega) to follow, 2200 of 65536 here, and reaches the limit
        # after omega * 12412 / nlim samples; so no viterbi (a sixth of the loop gain), omega of 4 at most (2 for BPSK), 20000 samples
        drift, viterbi, n = 0, 0, 20000
        ratio = float(rng.choice([1.5, 2.0] if mod == BPSK else [1.5, 2.0, 3.0, 4.0]))
    fm = int(round(msps / ratio))
    k = cfg(msps=msps, sample_rate=msps, centre_frequency=centre, rf_bandwidth=int(min(0.95 * msps, 1.6 * fm)), symbol_rate=fm, modulation=mod, fec=fec,
            standard=int(rng.integers(0, 2)), sampler=sampler, rolloff=rolloff, excursion=exc, hard_metric=int(rng.random() < 0.25),
            viterbi=viterbi, allow_drift=drift, finfo=float(np.float32(msps / (dec + 0.5))))
    sig = dict(PSK, start=float(rng.uniform(0, 1)), sigma=float(rng.choice([0.0, 150.0, 900.0])), f0=float(centre))
    if kind == "sweep":
        omega = msps / fm
        sig["slope"] = -2200.0 * msps * 0.0012 / (omega * omega * 65536.0)
        sig["sigma"] = 50.0
    elif kind == "timing":
        sig["timing"] = float(rng.choice([-1, 1])) * float(rng.uniform(0.02, 0.06))
        sig["amp"] = 9000.0
    elif kind == "clipped":
        sig["amp"] = 60000.0
    elif kind == "noise":
        sig = {"kind": "noise"}
    seed = 2000 + i
    return {"name": f"random_{i:03d}", "seed": seed, "n": n, "sig": sig, "cfg": k, "splits": _ragged(n, seed, int(rng.integers(2, 6)))}


def random_cases(count: int = 100) -> list[dict]:
    """the first `count` random cases, drawn in order from one generator"""
    rng = np.random.default_rng(RANDOM_SEED)
    return [random_case(rng, i) for i in range(count)]


def assert_random_shares(cases, hits_per_case):
    """the issue's conditions on the draw, on the configurations and on the oracle's counters"""
    assert len(cases) == len(hits_per_case) == 100
    for s in (NEAREST, LINEAR, RRC):
        assert sum(1 for c in cases if c["cfg"]["sampler"] == s) >= 25, s
    for m in range(9):
        assert sum(1 for c in cases if c["cfg"]["modulation"] == m) >= 5, m
    assert all(h["symbols"] > 0 for h in hits_per_case)
    clamp = sum(1 for h in hits_per_case if h["clamp_low"] + h["clamp_high"] > 0)
    reset = sum(1 for h in hits_per_case if h["drift_reset"] > 0)
    two = sum(1 for h in hits_per_case if h["two_meas"] > 0)
    assert clamp >= 10 and reset >= 5 and two >= 5, (clamp, reset, two)
    return clamp, reset, two
