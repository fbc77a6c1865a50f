"""Builds tests/golden/nfm_tone_rec.cpp against the reference's own NCO, Interpolator, PhaseDiscriminators, MovingAverageUtil,
DoubleBufferFIFO, Bandpass, Lowpass and CTCSSDetector (sdrbase/dsp/nco.cpp, interpolator.cpp and ctcssdetector.cpp compiled
where they lie, the rest are headers; Qt headers of the build image for qint16 & co.) and records
tests/golden/nfm_tone_golden.npz for the cases of tests/nfm_tone_cases.py.

    python tests/golden/make_golden_nfm_tone.py [--ref /root/reference]

Per case the fixture keeps the audio count of every feed, the audio in full when the case's output is small (<= 24 KiB),
else its sha256, the moving average, m_magsqSum, m_magsqPeak, m_magsqCount and the final squelch state, every change of
m_ctcssIndex (audio sample position in the stream, new index), and the detector's final state: m_ctcssIndex, changes,
completed blocks, toneDetected, maxPowerIndex, power[32], and its design: coef[32], N, rate; and the AFSquelch as NFMDemod's
constructor configures it (N, tones[2], coef[2], threshold, 1000 * isOpen + squelchCount, m_afSquelchOpen, the two moving-average sums)."""
from __future__ import annotations

import argparse
import hashlib
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

QTINC = os.environ.get("QTINC", "/opt/conda/include/qt")
FULL_LIMIT = 24 << 10


def available(ref: str) -> bool:
    return os.path.isfile(os.path.join(ref, "sdrbase", "dsp", "bandpass.h")) and os.path.isfile(os.path.join(QTINC, "QtCore", "QtGlobal"))


def build_recorder(ref: str, out_dir: str | None = None) -> str:
    d = out_dir or tempfile.mkdtemp()
    exe = os.path.join(d, "nfm_tone_rec")
    # strict IEEE, scalar Interpolator (USE_SSE2 undefined)
    flags = ["-O2", "-std=c++11", "-fPIC", "-fno-fast-math", "-ffp-contract=off", "-w", "-DQT_NO_VERSION_TAGGING", "-DQT_NO_DEBUG_OUTPUT",
             "-Dsdrangel_STATIC", "-I" + QTINC, "-I" + os.path.join(QTINC, "QtCore"), "-I" + os.path.join(ref, "sdrbase"), "-I" + os.path.join(ref, "exports")]
    srcs = [os.path.join(ref, "sdrbase", "dsp", s) for s in ("nco.cpp", "interpolator.cpp", "ctcssdetector.cpp", "afsquelch.cpp")]
    subprocess.check_call(["g++"] + flags + [os.path.join(HERE, "nfm_tone_rec.cpp")] + srcs + ["-o", exe])
    return exe


def record(exe: str, cfg, iq: np.ndarray, splits) -> dict:
    """runs the recorder on one demodulator: the stream iq cut into feeds of the given lengths"""
    d = tempfile.mkdtemp()
    fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
    with open(fin, "wb") as f:
        f.write(np.ascontiguousarray(iq, np.int16).tobytes())
    f32 = lambda v: "%.9g" % float(np.float32(v))
    cmds = ["new %d %d %d %s %s %d %s %s %d %d %d %d %d" % (cfg[0], cfg[1], cfg[2], f32(cfg[3]), f32(cfg[4]), int(cfg[5]), f32(cfg[6]), f32(cfg[7]),
                                                        int(cfg[8]), int(cfg[9]), int(cfg[10]), int(cfg[11]), int(cfg[12]) if len(cfg) > 12 else 0)]
    cmds += [f"feed {int(m)}" for m in splits] + ["end"]
    subprocess.run([exe, fin, fout], input="\n".join(cmds) + "\n", text=True, check=True, timeout=600)
    raw = open(fout, "rb").read()
    feeds, events, pos, base = [], [], 0, 0
    for _ in splits:
        k = int(np.frombuffer(raw, np.int64, 1, pos)[0]); pos += 8
        feeds.append(np.frombuffer(raw, np.int16, k, pos).copy()); pos += 2 * k
        ne = int(np.frombuffer(raw, np.int64, 1, pos)[0]); pos += 8
        ev = np.frombuffer(raw, np.int64, 2 * ne, pos).reshape(ne, 2); pos += 16 * ne
        events += [(base + int(a), int(i)) for a, i in ev]
        base += k
    m, s, p = np.frombuffer(raw, np.float64, 3, pos); pos += 24
    cnt, op, st = np.frombuffer(raw, np.int64, 3, pos); pos += 24
    index, changes, blocks, det, mi = (int(v) for v in np.frombuffer(raw, np.int64, 5, pos)); pos += 40
    power = np.frombuffer(raw, np.float32, 32, pos).copy(); pos += 128
    coef = np.frombuffer(raw, np.float32, 32, pos).copy(); pos += 128
    N, rate = (int(v) for v in np.frombuffer(raw, np.int32, 2, pos)); pos += 8
    af = np.frombuffer(raw, np.float64, 10, pos).copy(); pos += 80
    assert pos == len(raw)
    return {"feeds": feeds, "events": events, "magsq": float(m), "sum": float(s), "peak": float(p), "count": int(cnt), "open": bool(op), "state": int(st),
            "index": index, "changes": changes, "blocks": blocks, "detected": bool(det), "max_index": mi, "power": power, "coef": coef, "N": N,
            "rate": rate, "af": af}


def audio_hash(a: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(a, np.int16).tobytes()).hexdigest()


def main():
    from tests import nfm_tone_cases as ac
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(HERE, "nfm_tone_golden.npz"))
    args = ap.parse_args()
    if not available(args.ref):
        sys.exit("reference tree or Qt headers not found")
    exe = build_recorder(args.ref)
    arrays = {}
    for c in ac.CASES:
        r = record(exe, c["cfg"], ac.inputs(c), c["splits"])
        name = c["name"]
        audio = np.concatenate(r["feeds"]) if r["feeds"] else np.zeros(0, np.int16)
        arrays[f"{name}/counts"] = np.array([f.size for f in r["feeds"]], np.int64)
        if audio.nbytes <= FULL_LIMIT:
            arrays[f"{name}/audio"] = audio
        else:
            arrays[f"{name}/sha256"] = np.array(audio_hash(audio))
        arrays[f"{name}/levels"] = np.array([r["magsq"], r["sum"], r["peak"]], np.float64)
        arrays[f"{name}/state"] = np.array([r["count"], int(r["open"]), r["state"]], np.int64)
        arrays[f"{name}/events"] = np.array(r["events"], np.int64).reshape(-1, 2)
        arrays[f"{name}/tone"] = np.array([r["index"], r["changes"], r["blocks"], int(r["detected"]), r["max_index"], r["N"], r["rate"]], np.int64)
        arrays[f"{name}/power"] = r["power"]
        arrays[f"{name}/coef"] = r["coef"]
        arrays[f"{name}/af"] = r["af"]
    np.savez_compressed(args.out, **arrays)
    print(f"wrote {args.out}: {len(ac.CASES)} cases, {os.path.getsize(args.out)} bytes")


if __name__ == "__main__":
    main()
