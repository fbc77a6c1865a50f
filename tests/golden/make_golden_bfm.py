"""Builds tests/golden/bfm_rec.cpp against the reference's own NCO, fftfilt (g_fft), PhaseDiscriminators, RDSPhaseLock, Interpolator
and LowPassFilterRC (sdrbase/dsp/*.cpp compiled where they lie; Qt headers of the build image for qint16 & co.) and records
tests/golden/bfm_golden.npz for the cases of tests/bfm_cases.py.

    python tests/golden/make_golden_bfm.py [--ref /root/reference]
    python tests/golden/make_golden_bfm.py --random      records tests/golden/bfm_random_golden.npz for bfm_cases.random_cases()

Per case the fixture keeps the inputs (their sha256 beyond bfm_cases.IN_FULL samples), the l, r pairs of every feed, the real
parts of the sink stream's Samples (per feed their sha256 beyond bfm_cases.SINK_FULL samples), and after every feed m_magsqSum,
m_magsqPeak, m_magsqCount, m_squelchState, locked(), m_lock_cnt and the bits of m_pilot_level, m_freq, m_phase and both m_y1.
`host` notes the libm the recorder ran on: the pilot loop calls its sinf and cosf and feeds back what they return.

The random draw's fixture keeps digests only (bfm_cases.pack_digests): per feed the lengths and sha256 of audio and sink stream and
the same state words, m_magsqSum and m_magsqPeak as double bits; inputs as their sha256.  It is written with fixed zip timestamps:
the same recording gives the same bytes."""
from __future__ import annotations

import argparse
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
SOURCES = ("nco.cpp", "interpolator.cpp", "fftfilt.cpp", "phaselock.cpp", "filterrc.cpp")


def available(ref: str) -> bool:
    return all(os.path.isfile(os.path.join(ref, "sdrbase", "dsp", s)) for s in SOURCES) and os.path.isfile(os.path.join(QTINC, "QtCore", "QtGlobal"))


def build_recorder(ref: str, out_dir: str | None = None) -> str:
    d = out_dir or tempfile.mkdtemp()
    exe = os.path.join(d, "bfm_rec")
    # strict IEEE, scalar Interpolator (USE_SSE2 undefined)
    flags = ["-O2", "-std=c++11", "-fPIC", "-fno-fast-math", "-ffp-contract=off", "-w", "-DQT_NO_VERSION_TAGGING", "-DQT_NO_DEBUG_OUTPUT",
             "-Dsdrangel_STATIC", "-I" + QTINC, "-I" + os.path.join(QTINC, "QtCore"), "-I" + os.path.join(ref, "sdrbase"), "-I" + os.path.join(ref, "exports")]
    srcs = [os.path.join(ref, "sdrbase", "dsp", s) for s in SOURCES]
    subprocess.check_call(["g++"] + flags + [os.path.join(HERE, "bfm_rec.cpp")] + srcs + ["-o", exe])
    return exe


def host_note() -> str:
    try:
        flags = next(l for l in open("/proc/cpuinfo") if l.startswith("flags")).split()
    except (OSError, StopIteration):
        flags = []
    return f"{' '.join(platform.libc_ver())} {platform.machine()} fma={int('fma' in flags)}"


def record(exe: str, cfg: dict, iq: np.ndarray, splits) -> dict:
    """runs the recorder on one demodulator: the stream iq cut into feeds of the given lengths"""
    from tests.bfm_cases import FIELDS
    d = tempfile.mkdtemp()
    fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
    with open(fin, "wb") as f:
        f.write(np.ascontiguousarray(iq, np.int16).tobytes())
    word = lambda k: "%.9g" % float(np.float32(cfg[k])) if k in ("rf", "af", "vol", "sq") else str(int(cfg[k]))
    cmds = ["new " + " ".join(word(k) for k in FIELDS)] + [f"feed {int(m)}" for m in splits]
    subprocess.run([exe, fin, fout], input="\n".join(cmds) + "\n", text=True, check=True, timeout=600)
    raw = open(fout, "rb").read()
    audio, sink, states, pos = [], [], [], 0
    for _ in splits:
        k = int(np.frombuffer(raw, np.int64, 1, pos)[0]); pos += 8
        audio.append(np.frombuffer(raw, np.int16, 2 * k, pos).reshape(k, 2).copy()); pos += 4 * k
        m = int(np.frombuffer(raw, np.int64, 1, pos)[0]); pos += 8
        sink.append(np.frombuffer(raw, np.int16, m, pos).copy()); pos += 2 * m
        lv = np.frombuffer(raw, np.float64, 2, pos).copy(); pos += 16
        st = np.frombuffer(raw, np.int64, 4, pos).copy(); pos += 32
        bits = np.frombuffer(raw, np.uint32, 5, pos).copy(); pos += 20
        states.append((lv, st, bits))
    assert pos == len(raw)
    return {"audio": audio, "sink": sink, "states": states}


def save_npz(path: str, arrays: dict):
    """np.savez_compressed with the members' timestamps fixed: the bytes depend on the arrays alone"""
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name, a in arrays.items():
            with z.open(zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), "w") as f:
                f.compress_type = zipfile.ZIP_DEFLATED
                np.lib.format.write_array(f, np.asanyarray(a), allow_pickle=False)


def record_case(exe: str, case: dict, iq: np.ndarray) -> dict:
    """record() in bfm_cases.run_oracle's layout"""
    from tests import bfm_cases as bc
    r = record(exe, case["cfg"], iq, case["splits"])
    return {"audio": r["audio"], "sink": r["sink"], "states": bc.recorded_states(r["states"])}


def record_random(exe: str, out: str):
    from tests import bfm_cases as bc
    cases = bc.random_cases()
    arrays = bc.pack_digests(cases, [record_case(exe, c, bc.inputs(c)) for c in cases])
    arrays["host"] = np.array(host_note())
    save_npz(out, arrays)
    print(f"wrote {out}: {len(cases)} cases, {int(arrays['feeds'].sum())} feeds on {host_note()}, {os.path.getsize(out)} bytes")


def main():
    from tests import bfm_cases as bc
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=None)
    ap.add_argument("--random", action="store_true")
    args = ap.parse_args()
    if not available(args.ref):
        sys.exit("reference tree or Qt headers not found")
    exe = build_recorder(args.ref)
    if args.random:
        return record_random(exe, args.out or bc.RANDOM_GOLDEN)
    args.out = args.out or os.path.join(HERE, "bfm_golden.npz")
    arrays = {"host": np.array(host_note())}
    for c in bc.CASES:
        x = bc.inputs(c)
        r = record(exe, c["cfg"], x, c["splits"])
        name = c["name"]
        if c["n"] <= bc.IN_FULL:
            arrays[f"{name}/in"] = x
        arrays[f"{name}/in_sha256"] = np.array(bc.sha(x))
        arrays[f"{name}/audio_counts"] = np.array([a.shape[0] for a in r["audio"]], np.int64)
        arrays[f"{name}/audio"] = np.concatenate(r["audio"])
        arrays[f"{name}/sink_counts"] = np.array([s.size for s in r["sink"]], np.int64)
        if c["n"] <= bc.SINK_FULL:
            arrays[f"{name}/sink"] = np.concatenate(r["sink"])
        else:
            arrays[f"{name}/sink_sha256"] = np.array([bc.sha(s) for s in r["sink"]])
        arrays[f"{name}/levels"] = np.array([s[0] for s in r["states"]], np.float64).reshape(-1, 2)
        arrays[f"{name}/state"] = np.array([s[1] for s in r["states"]], np.int64).reshape(-1, 4)
        arrays[f"{name}/bits"] = np.array([s[2] for s in r["states"]], np.uint32).reshape(-1, 5)
    np.savez_compressed(args.out, **arrays)
    print(f"wrote {args.out}: {len(bc.CASES)} cases on {host_note()}, {os.path.getsize(args.out)} bytes")


if __name__ == "__main__":
    main()
