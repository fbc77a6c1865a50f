"""Builds tests/golden/spectrum_rec.cpp against the reference's own SpectrumVis (sdrgui/dsp/spectrumvis.cpp with
fftengine / kissengine / fftwindow, basebandsamplesink, dspcommands, message, messagequeue and their moc output; Qt 5 of
the build image) and records tests/golden/spectrum_golden.npz for the cases of tests/spectrum_cases.py.

    python tests/golden/make_golden_spectrum.py [--ref /root/reference]

Per case the fixture keeps the frame count of every feed; the frames themselves in full when the case's output is small
(<= 24 KiB), else the sha256 of each feed's frames (float32 bits)."""
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
QTLIB = os.environ.get("QTLIB", "/opt/conda/lib")
MOC = os.environ.get("MOC", "/opt/conda/bin/moc")
FULL_LIMIT = 24 << 10

GLSPECTRUM_STUB = """#pragma once
#include <vector>
#include "dsp/dsptypes.h"
class GLSpectrum {
public:
    void newSpectrum(const std::vector<Real>& spectrum, int fftSize);
};
"""


def available(ref: str) -> bool:
    return (os.path.isfile(os.path.join(ref, "sdrgui", "dsp", "spectrumvis.cpp")) and os.access(MOC, os.X_OK)
            and os.path.isfile(os.path.join(QTLIB, "libQt5Core.so.5")) and os.path.isdir(os.path.join(QTINC, "QtCore")))


def build_recorder(ref: str, out_dir: str | None = None) -> str:
    d = out_dir or tempfile.mkdtemp()
    os.makedirs(os.path.join(d, "gui"), exist_ok=True)
    with open(os.path.join(d, "gui", "glspectrum.h"), "w") as f:
        f.write(GLSPECTRUM_STUB)
    inc = ["-I" + d, "-I" + os.path.join(ref, "sdrgui"), "-I" + os.path.join(ref, "sdrbase"), "-I" + os.path.join(ref, "exports")]
    mocs = []
    for h in ("sdrbase/dsp/basebandsamplesink.h", "sdrbase/util/messagequeue.h"):
        m = os.path.join(d, "moc_" + os.path.basename(h)[:-2] + ".cpp")
        subprocess.check_call([MOC] + inc + [os.path.join(ref, h), "-o", m])
        mocs.append(m)
    srcs = [os.path.join(ref, s) for s in ("sdrgui/dsp/spectrumvis.cpp", "sdrbase/dsp/fftengine.cpp", "sdrbase/dsp/kissengine.cpp",
                                           "sdrbase/dsp/fftwindow.cpp", "sdrbase/dsp/basebandsamplesink.cpp",
                                           "sdrbase/dsp/dspcommands.cpp", "sdrbase/util/message.cpp", "sdrbase/util/messagequeue.cpp")]
    exe = os.path.join(d, "spectrum_rec")
    # strict IEEE, kissfft engine (the reference picks it when FFTW is absent: sdrbase/CMakeLists.txt)
    flags = ["-O2", "-std=c++11", "-fPIC", "-fno-fast-math", "-ffp-contract=off", "-w", "-DUSE_KISSFFT", "-DLINUX",
             "-DQT_NO_VERSION_TAGGING", "-DQT_NO_DEBUG_OUTPUT", "-Dsdrangel_STATIC", "-I" + QTINC, "-I" + os.path.join(QTINC, "QtCore")]
    subprocess.check_call(["g++"] + flags + inc + [os.path.join(HERE, "spectrum_rec.cpp")] + srcs + mocs +
                          [os.path.join(QTLIB, "libQt5Core.so.5"), "-Wl,-rpath," + QTLIB, "-Wl,-rpath-link," + QTLIB, "-o", exe])
    return exe


def record(exe: str, cfg, steps, inputs):
    """runs the recorder on one start configuration and its steps; returns per feed step the frames (k, N) float32"""
    d = tempfile.mkdtemp()
    fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
    with open(fin, "wb") as f:
        for s, iq in zip(steps, inputs):
            if s[0] == "feed":
                f.write(np.ascontiguousarray(iq, np.int16).tobytes())
    cmds = ["cfg " + " ".join(str(int(v)) for v in cfg)]
    for s in steps:
        cmds.append(f"feed {int(s[1])} {int(bool(s[2]))}" if s[0] == "feed" else "cfg " + " ".join(str(int(v)) for v in s[1]))
    # the system libstdc++ ahead of the (older) one next to Qt5Core, which the rpath would pick first
    env = dict(os.environ, LD_LIBRARY_PATH=":".join(p for p in ("/usr/lib/x86_64-linux-gnu", os.environ.get("LD_LIBRARY_PATH", "")) if p))
    subprocess.run([exe, fin, fout], input="\n".join(cmds) + "\n", text=True, check=True, timeout=600, env=env)
    raw = open(fout, "rb").read()
    res, pos = [], 0
    for s in steps:
        if s[0] != "feed":
            continue
        k, n = np.frombuffer(raw, np.int64, 2, pos)
        pos += 16
        fr = np.frombuffer(raw, np.float32, int(k * n), pos).reshape(int(k), int(n)) if k else np.zeros((0, 0), np.float32)
        pos += int(k * n) * 4
        res.append(fr.copy())
    assert pos == len(raw)
    return res


def frames_hash(fr: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(fr, np.float32).tobytes()).hexdigest()


def main():
    from tests import spectrum_cases as sc
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(HERE, "spectrum_golden.npz"))
    args = ap.parse_args()
    if not available(args.ref):
        sys.exit("reference tree, moc or Qt5Core not found")
    exe = build_recorder(args.ref)
    arrays = {}
    for c in sc.CASES:
        feeds = record(exe, c["cfg"], c["steps"], sc.inputs(c))
        name = c["name"]
        arrays[f"{name}/counts"] = np.array([f.shape[0] for f in feeds], np.int64)
        if sum(f.nbytes for f in feeds) <= FULL_LIMIT:
            arrays[f"{name}/frames"] = np.concatenate([f.reshape(-1) for f in feeds]).astype(np.float32) if feeds else np.zeros(0, np.float32)
        else:
            arrays[f"{name}/sha256"] = np.array([frames_hash(f) for f in feeds])
    np.savez_compressed(args.out, **arrays)
    print(f"wrote {args.out}: {len(sc.CASES)} cases, {os.path.getsize(args.out)} bytes")


if __name__ == "__main__":
    main()
