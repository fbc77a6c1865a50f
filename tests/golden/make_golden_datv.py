"""Builds tests/golden/datv_rec.cpp against the reference's own NCO, fftfilt and leansdr headers, compiled where they lie with
strict-IEEE flags (the Qt headers are needed for QtGlobal's types only; nothing of Qt is linked), and records
tests/golden/datv_golden.npz for the cases of tests/datv_cases.py.  The recorder restates DATVDemod's wiring down to p_symbols
and calls the reference's classes; it copies none of their text (see its header).

    python tests/golden/make_golden_datv.py [--ref /root/reference] [--random]

--random records tests/golden/datv_random_golden.npz instead: the cut stream fed whole and the 100 random cases of
tests/datv_cases.py, digests only.

Per case the fixture keeps the sha256 of the input (the generator is tests/datv_cases.py's, seeded), the design words, the sha256 of
the coefficients, of the trig table, of the constellation table and of symbols[], and per feed the counts, the state's words and
the symbols, points and measurements -- as they are for cases up to FULL samples, as sha256 beyond.  A measurement is recorded as
(freq, ss, mer); the estimates behind it are in the state at the end of each feed."""
from __future__ import annotations

import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

QTINC = os.environ.get("QTINC", "/opt/conda/include/qt")
DATV_DIR = ("plugins", "channelrx", "demoddatv")
SOURCES = ("dsp/nco.cpp", "dsp/fftfilt.cpp")
MEAS3 = np.dtype([(k, np.uint32) for k in ("freq", "ss", "mer")])


def available(ref: str) -> bool:
    return os.path.isfile(os.path.join(ref, *DATV_DIR, "leansdr", "sdr.h")) and os.path.isfile(os.path.join(QTINC, "QtCore", "QtGlobal"))


def build_recorder(ref: str) -> str:
    exe = os.path.join(tempfile.mkdtemp(), "datv_rec")
    inc = ["-I" + QTINC, "-I" + os.path.join(QTINC, "QtCore"), "-I" + os.path.join(ref, "sdrbase"), "-I" + os.path.join(ref, "exports"),
           "-I" + os.path.join(ref, *DATV_DIR)]
    flags = ["-O2", "-std=c++11", "-fPIC", "-fno-fast-math", "-ffp-contract=off", "-w", "-DQT_NO_VERSION_TAGGING", "-DQT_NO_DEBUG_OUTPUT", "-Dsdrangel_STATIC"]
    subprocess.check_call(["g++"] + flags + inc + [os.path.join(HERE, "datv_rec.cpp")] + [os.path.join(ref, "sdrbase", s) for s in SOURCES] + ["-o", exe])
    return exe


def record(exe: str, case: dict, iq: np.ndarray, splits=None, step_every: int = 0) -> dict:
    """runs the recorder on one receiver: the stream iq cut into the case's feeds; step_every: a scheduler step every so many
    samples in place of feed()'s own rule"""
    from tests import datv_cases as dc
    k, splits = case["cfg"], splits or case["splits"]
    d = tempfile.mkdtemp()
    fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
    with open(fin, "wb") as f:
        f.write(np.ascontiguousarray(iq, np.int16).tobytes())
    word = lambda name, t: str(int(k[name])) if t == "i" else "%.9g" % float(np.float32(k[name]))
    cmds = [f"step {int(step_every)}", "new " + " ".join(word(name, t) for name, t in dc.CFG_FIELDS), "design"] + [f"feed {int(m)}" for m in splits]
    subprocess.run([exe, fin, fout], input="\n".join(cmds) + "\n", text=True, check=True, timeout=600, stderr=subprocess.DEVNULL)
    raw = open(fout, "rb").read()
    os.remove(fin); os.remove(fout)
    pos = 0

    def take(dtype, n):
        nonlocal pos
        a = np.frombuffer(raw, dtype, n, pos).copy()
        pos += a.nbytes
        return a

    fl, it = take(np.uint32, 6).tolist(), take(np.int32, 5).tolist()
    coeffs, trig, lut, sy = take(np.float32, it[2]), take(np.float32, 2 * 65536), take(np.uint8, 65536 * 8), take(np.int8, 512)
    feeds = []
    for _ in splits:
        ns = int(take(np.int64, 1)[0]); cost = take(np.int16, ns); symbol = take(np.uint8, ns)
        npts = int(take(np.int64, 1)[0]); pts = take(np.uint32, 2 * npts)
        nm = int(take(np.int64, 1)[0]); meas = take(np.uint32, 3 * nm).view(MEAS3)
        w = take(np.uint32, 21).tolist()
        held = int(take(np.int32, 1)[0])
        tail = take(np.int64, 3).tolist()
        feeds.append({"cost": cost, "symbol": symbol, "points": pts, "meas": meas, "state": w + [held] + tail})
    assert pos == len(raw)
    return {"design": fl + it, "tables": (coeffs, trig, lut, sy), "feeds": feeds}


def meas3(meas: np.ndarray) -> np.ndarray:
    """(freq, ss, mer) of the oracle's or the bank's measurement records, as the recorder has them"""
    out = np.zeros(meas.size, MEAS3)
    for k in ("freq", "ss", "mer"):
        out[k] = meas[k]
    return out


def pack(case: dict, r: dict, x: np.ndarray, full: bool) -> dict:
    """what the fixture keeps of one recording"""
    from tests import datv_cases as dc
    name, feeds = case["name"], r["feeds"]
    a = {f"{name}/in_sha256": np.array(dc.sha(x)), f"{name}/design": np.array(r["design"], np.int64),
         f"{name}/tables_sha256": np.array(dc.table_digests(r["tables"])),
         f"{name}/counts": np.array([[f["cost"].size, f["points"].size // 2, f["meas"].size] for f in feeds], np.int64),
         f"{name}/state": np.array([f["state"] for f in feeds], np.int64)}
    if full:
        a[f"{name}/cost"] = np.concatenate([f["cost"] for f in feeds]).astype(np.int16)
        a[f"{name}/symbol"] = np.concatenate([f["symbol"] for f in feeds]).astype(np.uint8)
        a[f"{name}/points"] = np.concatenate([f["points"] for f in feeds]).astype(np.uint32)
        a[f"{name}/meas"] = np.concatenate([f["meas"] for f in feeds]).view(np.uint32)
    else:
        a[f"{name}/feeds_sha256"] = np.array([[dc.sha(f["cost"]), dc.sha(f["symbol"]), dc.sha(f["points"]), dc.sha(f["meas"])] for f in feeds])
    return a


def main():
    from tests import datv_cases as dc
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--random", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not available(args.ref):
        sys.exit("reference tree or Qt headers not found")
    exe = build_recorder(args.ref)
    cases = ([dc.CUT_STREAM] + dc.random_cases()) if args.random else dc.CASES
    out = args.out or (dc.RANDOM_GOLDEN if args.random else dc.GOLDEN)
    arrays, symbols = {}, 0
    for c in cases:
        x = dc.inputs(c)
        r = record(exe, c, x)
        arrays.update(pack(c, r, x, full=not args.random and c["n"] <= dc.FULL))
        ns = [f["cost"].size for f in r["feeds"]]
        symbols += sum(ns)
        print(f"{c['name']}: symbols per feed {ns}, measurements {sum(f['meas'].size for f in r['feeds'])}")
    assert symbols >= len(cases)
    np.savez_compressed(out, **arrays)
    print(f"wrote {out}: {len(cases)} cases, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
