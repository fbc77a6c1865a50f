"""Builds tests/golden/am_sync_rec.cpp against the reference's own NCO, Interpolator, Lowpass, PhaseLockComplex, fftfilt, MagAGC,
Bandpass, MovingAverageUtil, DoubleBufferFIFO and StepFunctions (the .cpp files compiled where they lie, the rest are headers; Qt
headers of the build image for qint16 & co.) and records tests/golden/am_sync_golden.npz for the cases of tests/am_sync_cases.py.

    python tests/golden/make_golden_am_sync.py [--ref /root/reference] [--random]

Per case the fixture keeps the sha256 of the input (the generator is tests/am_sync_cases.py's, seeded), the audio count and the
audio of every feed, and after every feed m_magsq, m_magsqSum, m_magsqPeak, m_magsqCount, the squelch state, getPllLocked() and
the bits of getPllFrequency(); once per case the design products, the open-sample count after every feed and what the host build of
pll_phase_step (tests/am_sync_check.cpp probe) went through over the recorded loop input.  The case marked `trace` also keeps the
recorder's per-sample trace, for tests/test_am_sync_host.py.

The maker asserts on the recording itself that the cases do what they are for: at least one ends locked and one unlocked; every
sample before the conversion is finite and strictly inside the int16 range; a case that claims a reopening, a saturation branch, a
never-open squelch or feeds on block edges has it; the host step reproduces every recorded oscillator value; the two SSBFilter
designs give different audio.

--random records tests/am_sync_cases.random_cases(), envelope channels included (the recorder's pll argument), into
tests/golden/am_sync_random_golden.npz: per case the input digest, per feed the audio count and the sha256 of the audio, the
levels and the state after every feed, the final `opens`, and once a `host` string as tests/golden/bfm_random_golden.npz has one.
It stores digests, not audio; tests/test_am_sync_oracle.py compares the oracle with it case by case, and with the rebuilt recorder
in full where the reference tree is present."""
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
SOURCES = (("dsp", "nco.cpp"), ("dsp", "interpolator.cpp"), ("dsp", "fftfilt.cpp"), ("dsp", "agc.cpp"), ("dsp", "phaselockcomplex.cpp"))


def available(ref: str) -> bool:
    return os.path.isfile(os.path.join(ref, "sdrbase", "dsp", "phaselockcomplex.cpp")) and os.path.isfile(os.path.join(QTINC, "QtCore", "QtGlobal"))


def build_recorder(ref: str, out_dir: str | None = None) -> str:
    d = out_dir or tempfile.mkdtemp()
    exe = os.path.join(d, "am_sync_rec")
    # strict IEEE, scalar Interpolator (USE_SSE2 undefined)
    flags = ["-O2", "-std=c++11", "-fPIC", "-fno-fast-math", "-ffp-contract=off", "-w", "-DQT_NO_VERSION_TAGGING", "-DQT_NO_DEBUG_OUTPUT",
             "-Dsdrangel_STATIC", "-I" + QTINC, "-I" + os.path.join(QTINC, "QtCore"), "-I" + os.path.join(ref, "sdrbase"), "-I" + os.path.join(ref, "exports")]
    srcs = [os.path.join(ref, "sdrbase", *s) for s in SOURCES]
    subprocess.check_call(["g++"] + flags + [os.path.join(HERE, "am_sync_rec.cpp")] + srcs + ["-o", exe])
    return exe


def build_check(out_dir: str | None = None) -> str:
    exe = os.path.join(out_dir or tempfile.mkdtemp(), "am_sync_check")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "sdrangel_amd", "csrc"),
                           os.path.join(ROOT, "tests", "am_sync_check.cpp"), "-o", exe])
    return exe


def record(exe: str, case: dict, iq: np.ndarray) -> dict:
    """runs the recorder on one demodulator: the stream iq cut into the case's feeds, `end` after every one"""
    cfg, sync, splits = case["cfg"], case["sync"], case["splits"]
    d = tempfile.mkdtemp()
    fin, fout, ftr = os.path.join(d, "in.bin"), os.path.join(d, "out.bin"), os.path.join(d, "trace.bin")
    with open(fin, "wb") as f:
        f.write(np.ascontiguousarray(iq, np.int16).tobytes())
    f32 = lambda v: "%.9g" % float(np.float32(v))
    ssb_rate, ssb_bw = sync[2] or 48000, sync[3] or 5000.0
    cmds = ["new %d %d %d %s %s %s %d %d %d %d %s" % (cfg[0], cfg[1], cfg[2], f32(cfg[3]), f32(cfg[4]), f32(cfg[5]), int(cfg[6]), int(cfg[7]),
                                                      int(sync[1]), int(ssb_rate), f32(ssb_bw)) + " %d" % int(sync[0]),
            "design"]
    for m in splits:
        cmds += [f"feed {int(m)}", "end"]
    subprocess.run([exe, fin, fout, ftr], input="\n".join(cmds) + "\n", text=True, check=True, timeout=600)
    raw = open(fout, "rb").read()
    pos = 0
    taps = np.frombuffer(raw, np.float32, 51, pos).copy(); pos += 204
    flen = int(np.frombuffer(raw, np.int64, 1, pos)[0]); pos += 8
    filt = np.frombuffer(raw, np.float32, 2 * flen, pos).copy(); pos += 8 * flen
    coef = np.frombuffer(raw, np.float32, 5, pos).copy(); pos += 20
    feeds, opens, levels, state, largest = [], [], [], [], 0.0
    for _ in splits:
        k = int(np.frombuffer(raw, np.int64, 1, pos)[0]); pos += 8
        feeds.append(np.frombuffer(raw, np.int16, k, pos).copy()); pos += 2 * k
        opens.append(int(np.frombuffer(raw, np.int64, 1, pos)[0])); pos += 8
        levels.append(np.frombuffer(raw, np.float64, 3, pos).copy()); pos += 24
        state.append(np.frombuffer(raw, np.int64, 9, pos).copy()); pos += 72
        largest = float(np.frombuffer(raw, np.float64, 1, pos)[0]); pos += 8
    assert pos == len(raw)
    return {"feeds": feeds, "opens": np.array(opens, np.int64), "levels": np.array(levels), "state": np.array(state, np.int64), "largest": largest,
            "taps": taps, "filt": filt, "coef": coef, "trace": ftr}


def host_note() -> str:
    import platform
    try:
        flags = next(l for l in open("/proc/cpuinfo") if l.startswith("flags")).split()
    except (OSError, StopIteration):
        flags = []
    return f"{' '.join(platform.libc_ver())} {platform.machine()} fma={int('fma' in flags)}"


def random_arrays(exe: str, cases: list) -> dict:
    """what --random keeps of every case"""
    from tests import am_sync_cases as sc
    arrays = {"host": np.array(host_note())}
    for c in cases:
        x = sc.inputs(c)
        r = record(exe, c, x)
        name = c["name"]
        arrays[f"{name}/in_sha256"] = np.array(sc.sha(x))
        arrays[f"{name}/counts"] = np.array([f.size for f in r["feeds"]], np.int64)
        arrays[f"{name}/audio_sha256"] = np.array([sc.sha(f) for f in r["feeds"]])
        arrays[f"{name}/levels"] = r["levels"]
        arrays[f"{name}/state"] = r["state"][:, :5]
        arrays[f"{name}/opens"] = r["opens"][-1:]
    return arrays


def main():
    from tests import am_sync_cases as sc
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=None)
    ap.add_argument("--random", action="store_true")
    args = ap.parse_args()
    if not available(args.ref):
        sys.exit("reference tree or Qt headers not found")
    if args.random:
        out = args.out or os.path.join(HERE, "am_sync_random_golden.npz")
        cases = sc.random_cases()
        np.savez_compressed(out, **random_arrays(build_recorder(args.ref), cases))
        print(f"wrote {out}: {len(cases)} cases on {host_note()}, {os.path.getsize(out)} bytes")
        return
    args.out = args.out or os.path.join(HERE, "am_sync_golden.npz")
    exe, chk = build_recorder(args.ref), build_check()
    arrays, ends_locked, ends_unlocked, sat_cases = {}, 0, 0, 0
    audio_of = {}
    for c in sc.CASES:
        name, ex = c["name"], c["expect"]
        x = sc.inputs(c)
        r = record(exe, c, x)
        audio = np.concatenate(r["feeds"]) if r["feeds"] else np.zeros(0, np.int16)
        audio_of[name] = audio
        st = r["state"]            # per feed: count, open, squelch count, locked, freq bits, opens, reopenings, bad, opens before the first reopening
        locked = bool(st[-1, 3]) and bool(c["sync"][0])
        ends_locked += locked; ends_unlocked += not locked
        out = subprocess.run([chk, "probe", str(c["cfg"][2]), r["trace"]], capture_output=True, text=True, check=True).stdout.split()
        assert out[0] == "probe", out
        n_open, sat_hi, sat_lo, lock_up, lock_down, osc_bad, p_locked, p_freq = (int(v) for v in out[1:])
        print(f"{name}: {audio.size} audio, {n_open} open, largest |sample| {r['largest']:.1f}, locked {locked}, reopenings {int(st[-1, 6])}, "
              f"sat_hi {sat_hi} sat_lo {sat_lo}, lock_up {lock_up} lock_down {lock_down}")
        # every sample before the conversion finite and strictly inside the int16 range
        assert int(st[-1, 7]) == 0, (name, "out-of-range or non-finite samples", int(st[-1, 7]))
        # the host build of the step the device walk runs reproduces the recording
        assert n_open == int(st[-1, 5]) and osc_bad == 0 and p_locked == int(st[-1, 3]) and p_freq == int(st[-1, 4]), (name, out)
        if "locked" in ex:
            assert locked == ex["locked"], name
        if ex.get("sat"):
            assert sat_hi + sat_lo > 0, name
        sat_cases += sat_hi + sat_lo > 0
        if ex.get("reopens"):
            assert int(st[-1, 6]) >= 1, name
            B = sc.block(c["sync"][1])
            before = int(st[-1, 8])            # the squelch closed inside a block, with whole blocks on either side of the closure
            assert before > B and before % B not in (0, 1, B - 1) and n_open - before > B, (name, before, n_open)
        if ex.get("never_open"):
            assert n_open == 0 and not audio.any() and not locked and int(st[-1, 4]) == 0, name
        if ex.get("edges"):
            assert list(np.diff(np.concatenate(([0], r["opens"])))) == [0] + c["splits"][1:], (name, r["opens"])
        arrays[f"{name}/in_sha256"] = np.array(sc.sha(x))
        arrays[f"{name}/counts"] = np.array([f.size for f in r["feeds"]], np.int64)
        arrays[f"{name}/audio"] = audio
        arrays[f"{name}/levels"] = r["levels"]
        arrays[f"{name}/state"] = st[:, :5]
        arrays[f"{name}/opens"] = r["opens"]
        arrays[f"{name}/probe"] = np.array([sat_hi, sat_lo, lock_up, lock_down], np.int64)
        arrays[f"{name}/taps"], arrays[f"{name}/filter"], arrays[f"{name}/coef"] = r["taps"], r["filt"], r["coef"]
        if ex.get("trace"):
            arrays[f"{name}/trace"] = np.fromfile(r["trace"], np.float32).reshape(-1, 7)
            arrays[f"{name}/trace_sb"] = np.fromfile(r["trace"] + ".sb", np.float32).reshape(-1, 2)
    assert ends_locked >= 1 and ends_unlocked >= 1 and sat_cases >= 1, (ends_locked, ends_unlocked, sat_cases)
    # the once-designed SSBFilter: another design, another audio
    assert audio_of["usb_design_default"].size == audio_of["usb_design_own"].size
    assert not np.array_equal(audio_of["usb_design_default"], audio_of["usb_design_own"])
    np.savez_compressed(args.out, **arrays)
    print(f"wrote {args.out}: {len(sc.CASES)} cases, {os.path.getsize(args.out)} bytes")


if __name__ == "__main__":
    main()
