"""Builds tests/golden/chana_pll_rec.cpp against the reference's own PhaseLockComplex, FreqLockComplex, NCOF, Interpolator, fftfilt
and fftcorr (sdrbase/dsp/*.cpp compiled where they lie; Qt headers of the build image for qint16 & co.) and records
tests/golden/chana_pll_golden.npz for the cases of tests/chana_pll_cases.py, and tests/golden/chana_random_golden.npz for its 100
random cases.

    python tests/golden/make_golden_chana_pll.py [--ref /root/reference]

Per case the fixture keeps the inputs, the Sample count of every feed, the Sample stream, and after every feed m_magsq,
isPllLocked and the bits of getPllFrequency, getPllDeltaPhase and getPllPhase.  `host` notes the libm the recorder ran on: the
loops call its cosf, sinf and atan2f, and feed back what they return.

The random cases' fixture holds digests only, every feed of every case in one row of flat arrays (`feeds` has the feeds per case):
the Sample count, a SHA-256 of the feed's Samples, m_magsq, isPllLocked and the three floats' bits."""
from __future__ import annotations

import argparse
import hashlib
import os
import platform
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

QTINC = os.environ.get("QTINC", "/opt/conda/include/qt")
SOURCES = ("ncof.cpp", "interpolator.cpp", "fftfilt.cpp", "fftcorr.cpp", "phaselockcomplex.cpp", "freqlockcomplex.cpp")


def available(ref: str) -> bool:
    return all(os.path.isfile(os.path.join(ref, "sdrbase", "dsp", s)) for s in SOURCES) and os.path.isfile(os.path.join(QTINC, "QtCore", "QtGlobal"))


def build_recorder(ref: str, out_dir: str | None = None) -> str:
    d = out_dir or tempfile.mkdtemp()
    exe = os.path.join(d, "chana_pll_rec")
    # strict IEEE, scalar Interpolator (USE_SSE2 undefined)
    flags = ["-O2", "-std=c++11", "-fPIC", "-fno-fast-math", "-ffp-contract=off", "-w", "-DQT_NO_VERSION_TAGGING", "-DQT_NO_DEBUG_OUTPUT",
             "-Dsdrangel_STATIC", "-I" + QTINC, "-I" + os.path.join(QTINC, "QtCore"), "-I" + os.path.join(ref, "sdrbase"), "-I" + os.path.join(ref, "exports")]
    srcs = [os.path.join(ref, "sdrbase", "dsp", s) for s in SOURCES]
    subprocess.check_call(["g++"] + flags + [os.path.join(HERE, "chana_pll_rec.cpp")] + srcs + ["-o", exe])
    return exe


def host_note() -> str:
    try:
        flags = next(l for l in open("/proc/cpuinfo") if l.startswith("flags")).split()
    except (OSError, StopIteration):
        flags = []
    return f"{' '.join(platform.libc_ver())} {platform.machine()} fma={int('fma' in flags)}"


def record(exe: str, cfg: dict, iq: np.ndarray, splits, timed: bool = False) -> dict:
    """runs the recorder on one analyzer: the stream iq cut into feeds of the given lengths"""
    from tests.chana_pll_cases import FIELDS
    d = tempfile.mkdtemp()
    fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
    with open(fin, "wb") as f:
        f.write(np.ascontiguousarray(iq, np.int16).tobytes())
    cmds = ["new " + " ".join(str(int(cfg[f])) for f in FIELDS)] + [f"feed {int(m)}" for m in splits] + (["time"] if timed else [])
    p = subprocess.run([exe, fin, fout], input="\n".join(cmds) + "\n", text=True, check=True, timeout=600, capture_output=True)
    raw = open(fout, "rb").read()
    out, states, pos = [], [], 0
    for _ in splits:
        n = int(np.frombuffer(raw, np.int64, 1, pos)[0]); pos += 8
        out.append(np.frombuffer(raw, np.int16, 2 * n, pos).reshape(n, 2).copy()); pos += 4 * n
        m = float(np.frombuffer(raw, np.float64, 1, pos)[0]); pos += 8
        locked = int(np.frombuffer(raw, np.int32, 1, pos)[0]); pos += 4
        bits = np.frombuffer(raw, np.uint32, 3, pos); pos += 12
        states.append((locked, int(bits[0]), int(bits[1]), int(bits[2]), m))
    assert pos == len(raw)
    res = {"out": out, "states": states}
    if timed:
        res["seconds"] = float(p.stdout.split()[-1])
    return res


def sha(a: np.ndarray) -> np.ndarray:
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a, np.int16).tobytes()).digest(), np.uint8)


def digest(cases, results) -> dict:
    """the arrays of chana_random_golden.npz from one result per case (the recorder's, or the oracle's to compare with)"""
    flat = [(o, s) for r in results for o, s in zip(r["out"], r["states"])]
    return {"names": np.array([c["name"] for c in cases]), "feeds": np.array([len(r["out"]) for r in results], np.int32),
            "counts": np.array([o.shape[0] for o, _ in flat], np.int64), "sha": np.stack([sha(o) for o, _ in flat]),
            "locked": np.array([s[0] for _, s in flat], np.int32), "state_bits": np.array([s[1:4] for _, s in flat], np.uint32).reshape(-1, 3),
            "magsq": np.array([s[4] for _, s in flat], np.float64)}


def cat(parts) -> np.ndarray:
    return np.concatenate(parts) if parts else np.zeros((0, 2), np.int16)


def main():
    from tests import chana_pll_cases as pc
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(HERE, "chana_pll_golden.npz"))
    ap.add_argument("--random-out", default=os.path.join(HERE, "chana_random_golden.npz"))
    args = ap.parse_args()
    if not available(args.ref):
        sys.exit("reference tree or Qt headers not found")
    exe = build_recorder(args.ref)
    arrays = {"host": np.array(host_note())}
    for c in pc.CASES:
        x = pc.inputs(c)
        r = record(exe, c["cfg"], x, c["splits"])
        name = c["name"]
        arrays[f"{name}/in"] = x
        arrays[f"{name}/counts"] = np.array([a.shape[0] for a in r["out"]], np.int64)
        arrays[f"{name}/out"] = cat(r["out"])
        arrays[f"{name}/locked"] = np.array([s[0] for s in r["states"]], np.int32)
        arrays[f"{name}/state_bits"] = np.array([s[1:4] for s in r["states"]], np.uint32).reshape(-1, 3)
        arrays[f"{name}/magsq"] = np.array([s[4] for s in r["states"]], np.float64)
    np.savez_compressed(args.out, **arrays)
    print(f"wrote {args.out}: {len(pc.CASES)} cases on {host_note()}, {os.path.getsize(args.out)} bytes")
    cases = pc.random_cases()
    arrays = digest(cases, [record(exe, c["cfg"], pc.inputs(c), c["splits"]) for c in cases])
    np.savez_compressed(args.random_out, host=np.array(host_note()), **arrays)
    print(f"wrote {args.random_out}: {len(cases)} random cases, {os.path.getsize(args.random_out)} bytes")


if __name__ == "__main__":
    main()
