"""Builds tests/golden/chana_rec.cpp against the reference's own NCOF, Interpolator, fftfilt and fftcorr (sdrbase/dsp/ncof.cpp,
interpolator.cpp, fftfilt.cpp and fftcorr.cpp compiled where they lie, the rest are headers; Qt headers of the build image for
qint16 & co.) and records tests/golden/chana_golden.npz for the cases of tests/chana_cases.py.

    python tests/golden/make_golden_chana.py [--ref /root/reference]

Per case the fixture keeps the Sample count of every feed, the Sample stream in full when small (<= 24 KiB), else its sha256,
plus m_magsq and m_undersampleCount after the last feed."""
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
    return os.path.isfile(os.path.join(ref, "sdrbase", "dsp", "fftcorr.cpp")) and os.path.isfile(os.path.join(QTINC, "QtCore", "QtGlobal"))


def build_recorder(ref: str, out_dir: str | None = None) -> str:
    d = out_dir or tempfile.mkdtemp()
    exe = os.path.join(d, "chana_rec")
    # strict IEEE, scalar Interpolator (USE_SSE2 undefined)
    flags = ["-O2", "-std=c++11", "-fPIC", "-fno-fast-math", "-ffp-contract=off", "-w", "-DQT_NO_VERSION_TAGGING", "-DQT_NO_DEBUG_OUTPUT",
             "-Dsdrangel_STATIC", "-I" + QTINC, "-I" + os.path.join(QTINC, "QtCore"), "-I" + os.path.join(ref, "sdrbase"), "-I" + os.path.join(ref, "exports")]
    srcs = [os.path.join(ref, "sdrbase", "dsp", s) for s in ("ncof.cpp", "interpolator.cpp", "fftfilt.cpp", "fftcorr.cpp")]
    subprocess.check_call(["g++"] + flags + [os.path.join(HERE, "chana_rec.cpp")] + srcs + ["-o", exe])
    return exe


def record(exe: str, cfg: dict, iq: np.ndarray, splits) -> dict:
    """runs the recorder on one analyzer: the stream iq cut into feeds of the given lengths"""
    from tests.chana_cases import FIELDS
    d = tempfile.mkdtemp()
    fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
    with open(fin, "wb") as f:
        f.write(np.ascontiguousarray(iq, np.int16).tobytes())
    cmds = ["new " + " ".join(str(int(cfg[f])) for f in FIELDS)] + [f"feed {int(m)}" for m in splits] + ["end"]
    subprocess.run([exe, fin, fout], input="\n".join(cmds) + "\n", text=True, check=True, timeout=600)
    raw = open(fout, "rb").read()
    out, pos = [], 0
    for _ in splits:
        n = int(np.frombuffer(raw, np.int64, 1, pos)[0]); pos += 8
        out.append(np.frombuffer(raw, np.int16, 2 * n, pos).reshape(n, 2).copy()); pos += 4 * n
    m = float(np.frombuffer(raw, np.float64, 1, pos)[0]); pos += 8
    usc = int(np.frombuffer(raw, np.int64, 1, pos)[0]); pos += 8
    assert pos == len(raw)
    return {"out": out, "magsq": m, "usc": usc}


def stream_hash(a: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(a, np.int16).tobytes()).hexdigest()


def cat(parts) -> np.ndarray:
    return np.concatenate(parts) if parts else np.zeros((0, 2), np.int16)


def main():
    from tests import chana_cases as cc
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(HERE, "chana_golden.npz"))
    args = ap.parse_args()
    if not available(args.ref):
        sys.exit("reference tree or Qt headers not found")
    exe = build_recorder(args.ref)
    arrays = {}
    for c in cc.CASES:
        r = record(exe, c["cfg"], cc.inputs(c), c["splits"])
        name = c["name"]
        arrays[f"{name}/counts"] = np.array([a.shape[0] for a in r["out"]], np.int64)
        full = cat(r["out"])
        if full.nbytes <= FULL_LIMIT:
            arrays[f"{name}/out"] = full
        else:
            arrays[f"{name}/out_sha256"] = np.array(stream_hash(full))
        arrays[f"{name}/magsq"] = np.array([r["magsq"]], np.float64)
        arrays[f"{name}/usc"] = np.array([r["usc"]], np.int64)
    np.savez_compressed(args.out, **arrays)
    print(f"wrote {args.out}: {len(cc.CASES)} cases, {os.path.getsize(args.out)} bytes")


if __name__ == "__main__":
    main()
