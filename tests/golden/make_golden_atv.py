"""Builds tests/golden/atv_rec.cpp against the reference's own ATVDemod (plugins/channelrx/demodatv/atvdemod.cpp and its moc output,
with NCO, Interpolator, fftfilt, phaselock, recursivefilters, BasebandSampleSink and the message classes, all
compiled where they lie, linked against QtCore) and records tests/golden/atv_golden.npz for the cases of tests/atv_cases.py.  The
stand-ins of tests/golden/atv_stubs/ come first on the include path and take the place of TVScreen, DeviceSourceAPI,
ThreadedBasebandSampleSink, DownChannelizer and of headers ATVDemod includes without using them.

    python tests/golden/make_golden_atv.py [--ref /root/reference] [--random]

--random records tests/golden/atv_random_golden.npz instead: the shape cases, the cut streams fed whole and the 100 random cases of
tests/atv_cases.py (golden_random_cases()), digests only -- per case the sha256 of the input and the design integers, per feed the
render events, the state's words and the sha256 of each stored frame, of the screen and of the scope stream, in arrays shared by all cases.

Per case the fixture keeps the sha256 of the input (the generator is tests/atv_cases.py's, seeded), the design integers, and per
feed the render events, the stored frames, the screen, the scope stream and the state's 28 words; frames, screens and scope as
they are for cases up to FULL samples, as sha256 beyond.  The maker asserts on the recorder's screen counters what can be seen
from outside the class: a negative and a too-large row, a negative and a too-large column, pixels on a null row, renders, more
renders in a feed than a frames_cap of 1 -- and that no scope Sample has an imaginary part."""
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
QTLIB = os.environ.get("QTLIB", "/opt/conda/lib")
MOC = os.environ.get("MOC", "/opt/conda/bin/moc")
ATV_DIR = ("plugins", "channelrx", "demodatv")
SOURCES = ("dsp/nco.cpp", "dsp/interpolator.cpp", "dsp/fftfilt.cpp", "dsp/phaselock.cpp", "dsp/recursivefilters.cpp", "dsp/basebandsamplesink.cpp",
           "util/message.cpp", "util/messagequeue.cpp")
MOCS = ("sdrbase/dsp/basebandsamplesink.h", "sdrbase/util/messagequeue.h")
FULL = 12000            # cases up to this many samples keep frames, screens and scope as they are


def available(ref: str) -> bool:
    return (os.path.isfile(os.path.join(ref, *ATV_DIR, "atvdemod.cpp")) and os.path.isfile(os.path.join(QTINC, "QtCore", "QtGlobal"))
            and os.path.isfile(os.path.join(QTLIB, "libQt5Core.so.5")) and os.access(MOC, os.X_OK))


def build_recorder(ref: str) -> str:
    d = tempfile.mkdtemp()
    exe = os.path.join(d, "atv_rec")
    atv = os.path.join(ref, *ATV_DIR)
    inc = ["-I" + os.path.join(HERE, "atv_stubs"), "-I" + QTINC, "-I" + os.path.join(QTINC, "QtCore"), "-I" + os.path.join(ref, "sdrbase"),
           "-I" + os.path.join(ref, "exports"), "-I" + atv]
    mocs = []
    for h in MOCS + (os.path.join(*ATV_DIR, "atvdemod.h"),):
        m = os.path.join(d, "moc_" + os.path.basename(h)[:-2] + ".cpp")
        subprocess.check_call([MOC] + inc + [os.path.join(ref, h), "-o", m])
        mocs.append(m)
    # strict IEEE, scalar Interpolator (USE_SSE2 undefined), 16-bit samples
    flags = ["-O2", "-std=c++11", "-fPIC", "-fno-fast-math", "-ffp-contract=off", "-w", "-DQT_NO_VERSION_TAGGING", "-DQT_NO_DEBUG_OUTPUT", "-Dsdrangel_STATIC"]
    srcs = [os.path.join(ref, "sdrbase", s) for s in SOURCES] + [os.path.join(atv, "atvdemod.cpp")] + mocs
    subprocess.check_call(["g++"] + flags + inc + [os.path.join(HERE, "atv_rec.cpp")] + srcs +
                          [os.path.join(QTLIB, "libQt5Core.so.5"), "-Wl,-rpath," + QTLIB, "-Wl,-rpath-link," + QTLIB, "-o", exe])
    return exe


def record(exe: str, case: dict, iq: np.ndarray, splits=None) -> dict:
    """runs the recorder on one demodulator: the stream iq cut into the case's feeds"""
    from tests import atv_cases as ac
    k, splits = case["cfg"], splits or case["splits"]
    d = tempfile.mkdtemp()
    fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
    with open(fin, "wb") as f:
        f.write(np.ascontiguousarray(iq, np.int16).tobytes())
    word = lambda name, t: str(int(k[name])) if t == "i" else "%.9g" % float(np.float32(k[name]))
    cmds = ["new " + " ".join(word(name, t) for name, t in ac.CFG_FIELDS), "design"] + [f"feed {int(m)}" for m in splits]
    subprocess.run([exe, fin, fout], input="\n".join(cmds) + "\n", text=True, check=True, timeout=600, stderr=subprocess.DEVNULL)
    raw = open(fout, "rb").read()
    os.remove(fin); os.remove(fout)
    pos = 0

    def take(dtype, n):
        nonlocal pos
        a = np.frombuffer(raw, dtype, n, pos).copy()
        pos += a.nbytes
        return a

    design = take(np.int32, 12).tolist()
    rows, cols = design[10], design[9]
    feeds, counters = [], None
    for _ in splits:
        ne = int(take(np.int64, 1)[0]); events = take(np.int32, ne)
        ns = int(take(np.int64, 1)[0]); frames = [take(np.uint8, rows * cols).reshape(rows, cols) for _ in range(ns)]
        screen = take(np.uint8, rows * cols).reshape(rows, cols)
        nsc = int(take(np.int64, 1)[0]); scope = take(np.int16, nsc)
        st = take(np.uint32, 28)
        counters = take(np.int64, 6)
        feeds.append({"events": events, "frames": frames, "screen": screen, "scope": scope, "state": st[:10].view(np.int32).tolist() + st[10:].tolist()})
    assert pos == len(raw)
    return {"design": design, "feeds": feeds, "counters": counters}


def pack(case: dict, r: dict, x: np.ndarray) -> dict:
    """what the fixture keeps of one recording"""
    from tests import atv_cases as ac
    name, feeds = case["name"], r["feeds"]
    a = {f"{name}/in_sha256": np.array(ac.sha(x)), f"{name}/design": np.array(r["design"], np.int32),
         f"{name}/event_counts": np.array([f["events"].size for f in feeds], np.int64),
         f"{name}/events": np.concatenate([f["events"] for f in feeds]).astype(np.int32),
         f"{name}/state": np.array([f["state"] for f in feeds], np.int64),
         f"{name}/scope_counts": np.array([f["scope"].size for f in feeds], np.int64)}
    frames = [fr for f in feeds for fr in f["frames"]]
    a[f"{name}/frame_counts"] = np.array([len(f["frames"]) for f in feeds], np.int64)
    if case["n"] <= FULL:
        a[f"{name}/frames"] = np.array(frames, np.uint8).reshape(len(frames), *feeds[0]["screen"].shape)
        a[f"{name}/screens"] = np.array([f["screen"] for f in feeds], np.uint8)
        a[f"{name}/scope"] = np.concatenate([f["scope"] for f in feeds]).astype(np.int16)
    else:
        a[f"{name}/frames_sha256"] = np.array([ac.sha(fr) for fr in frames] or [""])
        a[f"{name}/screens_sha256"] = np.array([ac.sha(f["screen"]) for f in feeds])
        a[f"{name}/scope_sha256"] = np.array([ac.sha(f["scope"]) for f in feeds])
        a[f"{name}/last_screen"] = feeds[-1]["screen"]
    return a


def digest(a: np.ndarray) -> np.ndarray:
    """sha256 as 32 bytes"""
    import hashlib
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)


def pack_digests(runs: list) -> dict:
    """what the random fixture keeps of (case, feeds, design, input) tuples, every case's feeds end to end in arrays shared by all:
    no image, no stream.  tests/atv_cases.py's load_random_golden() takes it apart again; the oracle's results pack the same way"""
    feeds = [f for _, fs, _, _ in runs for f in fs]
    frames = [fr for f in feeds for fr in f["frames"]]
    return {"names": np.array([c["name"] for c, _, _, _ in runs]), "in_sha256": np.array([digest(x) for _, _, _, x in runs], np.uint8),
            "design": np.array([d for _, _, d, _ in runs], np.int32), "feeds": np.array([len(fs) for _, fs, _, _ in runs], np.int32),
            "event_counts": np.array([f["events"].size for f in feeds], np.int32),
            "events": np.concatenate([f["events"] for f in feeds]).astype(np.int32),
            "state": np.array([f["state"] for f in feeds], np.int64).astype(np.uint32),
            "frame_counts": np.array([len(f["frames"]) for f in feeds], np.int32),
            "frames_sha256": np.array([digest(fr) for fr in frames], np.uint8).reshape(len(frames), 32),
            "screens_sha256": np.array([digest(f["screen"]) for f in feeds], np.uint8),
            "scope_sha256": np.array([digest(f["scope"]) for f in feeds], np.uint8)}


def record_random(exe: str, out: str):
    from tests import atv_cases as ac
    cases = ac.golden_random_cases()
    ac.assert_random_shares(ac.random_cases())
    runs, renders = [], 0
    for c in cases:
        x = ac.inputs(c)
        r = record(exe, c, x)
        runs.append((c, r["feeds"], r["design"], x))
        renders += sum(f["events"].size for f in r["feeds"])
        print(f"{c['name']}: design {r['design']}, renders per feed {[f['events'].size for f in r['feeds']]}")
    assert renders >= len(cases)
    np.savez_compressed(out, **pack_digests(runs))
    print(f"wrote {out}: {len(cases)} cases, {os.path.getsize(out)} bytes")


def main():
    from tests import atv_cases as ac
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--random", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not available(args.ref):
        sys.exit("reference tree, moc, Qt headers or QtCore not found")
    exe = build_recorder(args.ref)
    if args.random:
        return record_random(exe, args.out or ac.RANDOM_GOLDEN)
    args.out = args.out or ac.GOLDEN
    arrays, total = {}, np.zeros(6, np.int64)
    renders, over_cap = 0, False
    for c in ac.CASES:
        x = ac.inputs(c)
        r = record(exe, c, x)
        arrays.update(pack(c, r, x))
        total += r["counters"]
        ne = [f["events"].size for f in r["feeds"]]
        renders += sum(ne)
        over_cap = over_cap or (c["cfg"]["frames_cap"] == 1 and max(ne) > 1)
        print(f"{c['name']}: design {r['design']}, renders per feed {ne}, screen counters {r['counters'].tolist()}")
    assert all(total[:5] >= 1) and total[5] == 0, total
    assert renders >= 1 and over_cap
    np.savez_compressed(args.out, **arrays)
    print(f"wrote {args.out}: {len(ac.CASES)} cases, {os.path.getsize(args.out)} bytes")


if __name__ == "__main__":
    main()
