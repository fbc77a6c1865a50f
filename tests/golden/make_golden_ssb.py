"""Builds tests/golden/ssb_rec.cpp against the reference's own NCO, Interpolator, fftfilt, MagAGC, DoubleBufferFIFO and
StepFunctions (sdrbase/dsp/nco.cpp, interpolator.cpp, fftfilt.cpp, agc.cpp and util/db.cpp compiled where they lie, the rest are
headers; Qt headers of the build image for qint16 & co.) and records tests/golden/ssb_golden.npz for the cases of
tests/ssb_cases.py.

    python tests/golden/make_golden_ssb.py [--ref /root/reference]

Per case the fixture keeps the audio and spectrum counts of every feed, the audio and the spectrum stream in full when small
(<= 24 KiB each), else their sha256, plus m_magsq, m_magsqSum, m_magsqPeak, m_magsqCount, m_audioActive, m_undersampleCount and
the AGC's getValue(), getStepValue() and getStepDownValue() after the last feed."""
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
    return os.path.isfile(os.path.join(ref, "sdrbase", "dsp", "agc.cpp")) and os.path.isfile(os.path.join(QTINC, "QtCore", "QtGlobal"))


def build_recorder(ref: str, out_dir: str | None = None) -> str:
    d = out_dir or tempfile.mkdtemp()
    exe = os.path.join(d, "ssb_rec")
    # strict IEEE, scalar Interpolator (USE_SSE2 undefined)
    flags = ["-O2", "-std=c++11", "-fPIC", "-fno-fast-math", "-ffp-contract=off", "-w", "-DQT_NO_VERSION_TAGGING", "-DQT_NO_DEBUG_OUTPUT",
             "-Dsdrangel_STATIC", "-I" + QTINC, "-I" + os.path.join(QTINC, "QtCore"), "-I" + os.path.join(ref, "sdrbase"), "-I" + os.path.join(ref, "exports")]
    srcs = [os.path.join(ref, "sdrbase", *s) for s in (("dsp", "nco.cpp"), ("dsp", "interpolator.cpp"), ("dsp", "fftfilt.cpp"), ("dsp", "agc.cpp"),
                                                      ("util", "db.cpp"))]
    subprocess.check_call(["g++"] + flags + [os.path.join(HERE, "ssb_rec.cpp")] + srcs + ["-o", exe])
    return exe


def record(exe: str, cfg: dict, iq: np.ndarray, splits) -> dict:
    """runs the recorder on one demodulator: the stream iq cut into feeds of the given lengths"""
    from tests.ssb_cases import FIELDS
    d = tempfile.mkdtemp()
    fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
    with open(fin, "wb") as f:
        f.write(np.ascontiguousarray(iq, np.int16).tobytes())
    f32 = lambda v: "%.9g" % float(np.float32(v))
    k = [cfg[f] for f in FIELDS]
    cmds = ["new %d %d %d %s %s %s " % (k[0], k[1], k[2], f32(k[3]), f32(k[4]), f32(k[5])) + " ".join(str(int(v)) for v in k[6:])]
    cmds += [f"feed {int(m)}" for m in splits] + ["end"]
    subprocess.run([exe, fin, fout], input="\n".join(cmds) + "\n", text=True, check=True, timeout=600)
    raw = open(fout, "rb").read()
    audio, spec, pos = [], [], 0
    for _ in splits:
        n = int(np.frombuffer(raw, np.int64, 1, pos)[0]); pos += 8
        audio.append(np.frombuffer(raw, np.int16, 2 * n, pos).reshape(n, 2).copy()); pos += 4 * n
        n = int(np.frombuffer(raw, np.int64, 1, pos)[0]); pos += 8
        spec.append(np.frombuffer(raw, np.int16, 2 * n, pos).reshape(n, 2).copy()); pos += 4 * n
    m, s, p = np.frombuffer(raw, np.float64, 3, pos); pos += 24
    cnt, act, usc = np.frombuffer(raw, np.int64, 3, pos); pos += 24
    u0, sv, sdv = np.frombuffer(raw, np.float64, 3, pos); pos += 24
    assert pos == len(raw)
    return {"audio": audio, "spec": spec, "magsq": float(m), "sum": float(s), "peak": float(p), "count": int(cnt), "active": bool(act),
            "usc": int(usc), "agc": (float(u0), float(sv), float(sdv))}


def stream_hash(a: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(a, np.int16).tobytes()).hexdigest()


def cat(parts) -> np.ndarray:
    return np.concatenate(parts) if parts else np.zeros((0, 2), np.int16)


def main():
    from tests import ssb_cases as sc
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(HERE, "ssb_golden.npz"))
    args = ap.parse_args()
    if not available(args.ref):
        sys.exit("reference tree or Qt headers not found")
    exe = build_recorder(args.ref)
    arrays = {}
    for c in sc.CASES:
        r = record(exe, c["cfg"], sc.inputs(c), c["splits"])
        name = c["name"]
        arrays[f"{name}/counts"] = np.array([[a.shape[0], s.shape[0]] for a, s in zip(r["audio"], r["spec"])], np.int64).reshape(-1, 2)
        for key in ("audio", "spec"):
            full = cat(r[key])
            if full.nbytes <= FULL_LIMIT:
                arrays[f"{name}/{key}"] = full
            else:
                arrays[f"{name}/{key}_sha256"] = np.array(stream_hash(full))
        arrays[f"{name}/levels"] = np.array([r["magsq"], r["sum"], r["peak"]], np.float64)
        arrays[f"{name}/state"] = np.array([r["count"], int(r["active"]), r["usc"]], np.int64)
        arrays[f"{name}/agc"] = np.array(r["agc"], np.float64)
    np.savez_compressed(args.out, **arrays)
    print(f"wrote {args.out}: {len(sc.CASES)} cases, {os.path.getsize(args.out)} bytes")


if __name__ == "__main__":
    main()
