"""Builds tests/golden/udpsrc_ssb_rec.cpp against the reference's own fftfilt, g_fft, MagAGC, MovingAverage, NCO and Interpolator
(sdrbase/dsp/fftfilt.cpp, nco.cpp, interpolator.cpp and agc.cpp compiled where they lie, the rest are headers; Qt headers of the
build image for qint16 & co.) and records tests/golden/udpsrc_ssb_golden.npz for the cases of tests/udpsrc_ssb_cases.py.

    python tests/golden/make_golden_udpsrc_ssb.py [--ref /root/reference]

Per case the fixture keeps the resampled and the payload count of every feed, the payload bytes and the spectrum Samples in
full when they are small (<= 4 KiB each), else their sha256, plus m_inMagsq, the final squelch state with gate and release, and
fftfilt's inptr.  The filter design, the same for every case, is kept once."""
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
FULL_LIMIT = 4 << 10


def available(ref: str) -> bool:
    return os.path.isfile(os.path.join(ref, "sdrbase", "dsp", "fftfilt.cpp")) and os.path.isfile(os.path.join(QTINC, "QtCore", "QtGlobal"))


def build_recorder(ref: str, out_dir: str | None = None) -> str:
    d = out_dir or tempfile.mkdtemp()
    exe = os.path.join(d, "udpsrc_ssb_rec")
    flags = ["-O2", "-std=c++11", "-fPIC", "-fno-fast-math", "-ffp-contract=off", "-w", "-DQT_NO_VERSION_TAGGING", "-DQT_NO_DEBUG_OUTPUT",
             "-Dsdrangel_STATIC", "-I" + QTINC, "-I" + os.path.join(QTINC, "QtCore"), "-I" + os.path.join(ref, "sdrbase"), "-I" + os.path.join(ref, "exports")]
    srcs = [os.path.join(ref, "sdrbase", "dsp", s) for s in ("nco.cpp", "interpolator.cpp", "agc.cpp", "fftfilt.cpp")]
    subprocess.check_call(["g++"] + flags + [os.path.join(HERE, "udpsrc_ssb_rec.cpp")] + srcs + ["-o", exe])
    return exe


def record(exe: str, cfg, iq: np.ndarray, splits) -> dict:
    """runs the recorder on one channel: the stream iq cut into feeds of the given lengths"""
    from tests import udpsrc_ssb_cases as sc
    d = tempfile.mkdtemp()
    fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
    with open(fin, "wb") as f:
        f.write(np.ascontiguousarray(iq, np.int16).tobytes())
    f32 = lambda v: "%.9g" % float(np.float32(v))
    fmt = int(cfg[3])
    cmds = ["new %d %d %s %d %s %d %s %d %d %d %d" % (cfg[0], cfg[1], f32(cfg[2]), fmt, f32(cfg[4]), int(cfg[5]), f32(cfg[6]), int(cfg[7]),
                                                  int(cfg[8]), int(cfg[9]), int(cfg[10]))]
    cmds += [f"feed {int(m)}" for m in splits] + ["end"]
    subprocess.run([exe, fin, fout], input="\n".join(cmds) + "\n", text=True, check=True, timeout=600)
    raw = open(fout, "rb").read()
    feeds, specs, pos = [], [], 0
    es = sc.elem_bytes(fmt)
    for _ in splits:
        k, m = (int(v) for v in np.frombuffer(raw, np.int64, 2, pos)); pos += 16
        feeds.append(sc.as_elements(fmt, raw[pos: pos + es * m])); pos += es * m
        specs.append(np.frombuffer(raw, np.int16, 2 * k, pos).reshape(-1, 2).copy()); pos += 4 * k
    mag = float(np.frombuffer(raw, np.float64, 1, pos)[0]); pos += 8
    op, oc, cc, gate, rel, inptr = (int(v) for v in np.frombuffer(raw, np.int64, 6, pos)); pos += 48
    filt = np.frombuffer(raw, np.float32, 1024, pos).copy(); pos += 4096
    assert pos == len(raw)
    return {"feeds": feeds, "specs": specs, "in_magsq": mag, "open": bool(op), "open_count": oc, "close_count": cc, "gate": gate, "release": rel,
            "pending": inptr, "filter": filt}


def digest(a: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def main():
    from tests import udpsrc_ssb_cases as sc
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(HERE, "udpsrc_ssb_golden.npz"))
    args = ap.parse_args()
    if not available(args.ref):
        sys.exit("reference tree or Qt headers not found")
    exe = build_recorder(args.ref)
    arrays = {}
    for c in sc.CASES:
        r = record(exe, c["cfg"], sc.inputs(c), c["splits"])
        name, fmt = c["name"], c["cfg"][3]
        arrays[f"{name}/counts"] = np.array([[s.shape[0], f.shape[0]] for s, f in zip(r["specs"], r["feeds"])], np.int64)
        for key, a in (("payload", np.concatenate(r["feeds"]) if r["feeds"] else sc.as_elements(fmt, b"")), ("spectrum", np.concatenate(r["specs"]))):
            if a.nbytes <= FULL_LIMIT:
                arrays[f"{name}/{key}"] = a
            else:
                arrays[f"{name}/{key}_sha256"] = np.array(digest(a))
        arrays[f"{name}/in_magsq"] = np.array([r["in_magsq"]], np.float64)
        arrays[f"{name}/state"] = np.array([int(r["open"]), r["open_count"], r["close_count"], r["gate"], r["release"], r["pending"]], np.int64)
        if "filter" in arrays:
            assert np.array_equal(arrays["filter"].view(np.uint32), r["filter"].view(np.uint32)), name       # item 1: one design for every configuration
        arrays["filter"] = r["filter"]
    np.savez_compressed(args.out, **arrays)
    print(f"wrote {args.out}: {len(sc.CASES)} cases, {os.path.getsize(args.out)} bytes")


if __name__ == "__main__":
    main()
