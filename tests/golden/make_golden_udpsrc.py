"""Builds tests/golden/udpsrc_rec.cpp against the reference's own NCO, Interpolator, MagAGC, MovingAverage, PhaseDiscriminators
and Bandpass (sdrbase/dsp/nco.cpp, interpolator.cpp and agc.cpp compiled where they lie, the rest are headers; Qt headers of the build image
for qint16 & co.) and records tests/golden/udpsrc_golden.npz for the cases of tests/udpsrc_cases.py.

    python tests/golden/make_golden_udpsrc.py [--ref /root/reference]

Per case the fixture keeps the sample count of every feed, the payload bytes and the spectrum Samples in full when they are
small (<= 24 KiB each), else their sha256, plus m_inMagsq and the final squelch state."""
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
    exe = os.path.join(d, "udpsrc_rec")
    # strict IEEE, scalar Interpolator (USE_SSE2 undefined)
    flags = ["-O2", "-std=c++11", "-fPIC", "-fno-fast-math", "-ffp-contract=off", "-w", "-DQT_NO_VERSION_TAGGING", "-DQT_NO_DEBUG_OUTPUT",
             "-Dsdrangel_STATIC", "-I" + QTINC, "-I" + os.path.join(QTINC, "QtCore"), "-I" + os.path.join(ref, "sdrbase"), "-I" + os.path.join(ref, "exports")]
    srcs = [os.path.join(ref, "sdrbase", "dsp", s) for s in ("nco.cpp", "interpolator.cpp", "agc.cpp")]
    subprocess.check_call(["g++"] + flags + [os.path.join(HERE, "udpsrc_rec.cpp")] + srcs + ["-o", exe])
    return exe


def record(exe: str, cfg, iq: np.ndarray, splits) -> dict:
    """runs the recorder on one channel: the stream iq cut into feeds of the given lengths"""
    from tests import udpsrc_cases as uc
    d = tempfile.mkdtemp()
    fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
    with open(fin, "wb") as f:
        f.write(np.ascontiguousarray(iq, np.int16).tobytes())
    f32 = lambda v: "%.9g" % float(np.float32(v))
    fmt = int(cfg[3])
    cmds = ["new %d %d %s %d %s %d %s %d %d %d %d" % (cfg[0], cfg[1], f32(cfg[2]), fmt, f32(cfg[4]), int(cfg[5]), f32(cfg[6]), int(cfg[7]),
                                                  int(cfg[8]), int(cfg[9]), int(cfg[10]) if len(cfg) > 10 else 0)]
    cmds += [f"feed {int(m)}" for m in splits] + ["end"]
    subprocess.run([exe, fin, fout], input="\n".join(cmds) + "\n", text=True, check=True, timeout=600)
    raw = open(fout, "rb").read()
    feeds, specs, pos = [], [], 0
    es = uc.elem_bytes(fmt)
    for _ in splits:
        k = int(np.frombuffer(raw, np.int64, 1, pos)[0]); pos += 8
        feeds.append(uc.as_samples(fmt, raw[pos: pos + es * k])); pos += es * k
        specs.append(np.frombuffer(raw, np.int16, 2 * k, pos).reshape(-1, 2).copy()); pos += 4 * k
    m = float(np.frombuffer(raw, np.float64, 1, pos)[0]); pos += 8
    op, oc, cc = np.frombuffer(raw, np.int64, 3, pos); pos += 24
    assert pos == len(raw)
    return {"feeds": feeds, "specs": specs, "in_magsq": m, "open": bool(op), "open_count": int(oc), "close_count": int(cc)}


def digest(a: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def joined(parts, fmt=None):
    from tests import udpsrc_cases as uc
    if parts:
        return np.concatenate(parts)
    return uc.as_samples(fmt, b"") if fmt is not None else np.zeros((0, 2), np.int16)


def main():
    from tests import udpsrc_cases as uc
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(HERE, "udpsrc_golden.npz"))
    args = ap.parse_args()
    if not available(args.ref):
        sys.exit("reference tree or Qt headers not found")
    exe = build_recorder(args.ref)
    arrays = {}
    for c in uc.CASES:
        r = record(exe, c["cfg"], uc.inputs(c), c["splits"])
        name = c["name"]
        arrays[f"{name}/counts"] = np.array([f.shape[0] for f in r["feeds"]], np.int64)
        for key, a in (("payload", joined(r["feeds"], c["cfg"][3])), ("spectrum", joined(r["specs"]))):
            if a.nbytes <= FULL_LIMIT:
                arrays[f"{name}/{key}"] = a
            else:
                arrays[f"{name}/{key}_sha256"] = np.array(digest(a))
        arrays[f"{name}/in_magsq"] = np.array([r["in_magsq"]], np.float64)
        arrays[f"{name}/state"] = np.array([int(r["open"]), r["open_count"], r["close_count"]], np.int64)
    np.savez_compressed(args.out, **arrays)
    print(f"wrote {args.out}: {len(uc.CASES)} cases, {os.path.getsize(args.out)} bytes")


if __name__ == "__main__":
    main()
