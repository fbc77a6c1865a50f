"""Builds tests/golden/lora_rec.cpp against the reference's own NCO, Interpolator and sfft (the .cpp files compiled where they lie;
lorabits.h included from the reference tree; Qt headers of the build image for qint16 & co.) and records
tests/golden/lora_golden.npz for the cases of tests/lora_cases.py.

    python tests/golden/make_golden_lora.py [--ref /root/reference]
    python tests/golden/make_golden_lora.py --random        writes tests/golden/lora_random_golden.npz instead: for the 100 random
        cases and the named ones of tests/lora_cases.py the recorder's sha256 of the input and of all Samples, the text, the last
        feed's state and the events -- what ties tests/lora_oracle.cpp to the reference where there is none.  The maker asserts
        on the recorder's counters what the random cases have to reach (lora_cases.assert_coverage)

Per case the fixture keeps the sha256 of the input (the generator is tests/lora_cases.py's, seeded), per feed the Sample count, the
Samples, the text dumpRaw printed and the state (m_tune, m_time, m_result, m_bin, m_count, lines so far), the recorder's event
counters after the last feed, and once the design products.  The case marked `trace` also keeps the per-fetch trace (mag, rev, the
result before and after the squelch, m_time, m_tune, m_result), for tests/test_lora_host.py.

The maker asserts on the recording itself that the cases do what they are for: the preamble locks and the lines a case claims; the
dump clipped at 140 symbols; m_time past 1023; a squelch closure with m_time at or below 70; both signs of the finetune sum across
the set; feeds ending on 63 .. 65 and 127 .. 129 outputs of the stream; a lock on bin 0 in silence; and that 7813 is a bandwidth whose cutoff differs as a float."""
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
SOURCES = (("dsp", "nco.cpp"), ("dsp", "interpolator.cpp"), ("dsp", "fftfilt.cpp"))
TRACE_W = 261
# the recorder's `end` record: six state values (kept per feed), then five event counters (kept once per case)
STATE = ("tune", "time", "result", "bin", "count", "lines")
EVENTS = ("tuned_up", "tuned_plain", "short_closes", "locks", "wraps")


def available(ref: str) -> bool:
    return os.path.isfile(os.path.join(ref, "plugins", "channelrx", "demodlora", "lorabits.h")) and os.path.isfile(os.path.join(QTINC, "QtCore", "QtGlobal"))


def build_recorder(ref: str, out_dir: str | None = None) -> str:
    d = out_dir or tempfile.mkdtemp()
    exe = os.path.join(d, "lora_rec")
    # strict IEEE, scalar Interpolator (USE_SSE2 undefined)
    flags = ["-O2", "-std=c++11", "-fPIC", "-fno-fast-math", "-ffp-contract=off", "-w", "-DQT_NO_VERSION_TAGGING", "-DQT_NO_DEBUG_OUTPUT",
             "-Dsdrangel_STATIC", "-I" + QTINC, "-I" + os.path.join(QTINC, "QtCore"), "-I" + os.path.join(ref, "sdrbase"), "-I" + os.path.join(ref, "exports"),
             "-I" + os.path.join(ref, "plugins", "channelrx", "demodlora")]
    srcs = [os.path.join(ref, "sdrbase", *s) for s in SOURCES]
    subprocess.check_call(["g++"] + flags + [os.path.join(HERE, "lora_rec.cpp")] + srcs + ["-o", exe])
    return exe


def record(exe: str, case: dict, iq: np.ndarray, splits=None) -> dict:
    """runs the recorder on one demodulator: the stream iq cut into the case's feeds, `end` after every one"""
    cfg, splits = case["cfg"], splits or case["splits"]
    d = tempfile.mkdtemp()
    fin, fout, ftr = os.path.join(d, "in.bin"), os.path.join(d, "out.bin"), os.path.join(d, "trace.bin")
    with open(fin, "wb") as f:
        f.write(np.ascontiguousarray(iq, np.int16).tobytes())
    cmds = ["new %d %d %d" % tuple(cfg), "design"]
    for m in splits:
        cmds += [f"feed {int(m)}", "end"]
    subprocess.run([exe, fin, fout, ftr], input="\n".join(cmds) + "\n", text=True, check=True, timeout=600)
    raw = open(fout, "rb").read()
    pos = 0
    nt = int(np.frombuffer(raw, np.int64, 1, pos)[0]); pos += 8
    taps = np.frombuffer(raw, np.float32, 16 * nt, pos).copy(); pos += 64 * nt
    vrot = np.frombuffer(raw, np.float32, 256, pos).copy(); pos += 1024
    k2 = np.frombuffer(raw, np.float32, 1, pos).copy(); pos += 4
    chirp = np.frombuffer(raw, np.float32, 512, pos).copy(); pos += 2048
    sample = np.frombuffer(raw, np.int16, 256, pos).copy().reshape(128, 2); pos += 512
    feeds, texts, state = [], [], []
    for _ in splits:
        k = int(np.frombuffer(raw, np.int64, 1, pos)[0]); pos += 8
        feeds.append(np.frombuffer(raw, np.int16, 2 * k, pos).copy().reshape(k, 2)); pos += 4 * k
        nb = int(np.frombuffer(raw, np.int64, 1, pos)[0]); pos += 8
        texts.append(raw[pos:pos + nb].decode("latin-1")); pos += nb
        state.append(np.frombuffer(raw, np.int64, 11, pos).copy()); pos += 88
    assert pos == len(raw)
    return {"feeds": feeds, "texts": texts, "state": np.array(state, np.int64).reshape(-1, 11), "ntaps": nt, "taps": taps, "vrot": vrot, "k2": k2,
            "chirp": chirp, "sample": sample, "trace": np.fromfile(ftr, np.float32).reshape(-1, TRACE_W)}


def pack_texts(texts) -> tuple[np.ndarray, np.ndarray]:
    """the feeds' texts as one uint8 array and the byte count of each"""
    return np.frombuffer("".join(texts).encode("latin-1"), np.uint8).copy(), np.array([len(t) for t in texts], np.int64)


def float_cutoff_taps(in_rate: int, bw: int) -> bool:
    """does Interpolator::create's design differ when the cutoff float(bw) / 1.9 passes through a float?  (the design of
    sdrangel_amd/csrc/backend_design.hpp, restated)"""
    def design(cutoff):
        ntaps = int(4.5 * 16)
        ntaps += ntaps % 2
        ntaps *= 16
        n = np.arange(ntaps)
        w = (0.54 - 0.46 * np.cos(2 * np.pi * n / (ntaps - 1))).astype(np.float32)
        M = (ntaps - 1) // 2
        k = np.arange(-M, M + 1)
        w0 = 2 * np.pi * cutoff / (16.0 * in_rate)
        with np.errstate(invalid="ignore", divide="ignore"):
            t = np.where(k == 0, w0 / np.pi, np.sin(k * w0) / (k * np.pi)) * w[k + M]
        return t.astype(np.float32)
    exact = float(np.float32(bw)) / 1.9
    return not np.array_equal(design(exact), design(float(np.float32(exact))))


def digest(lc, r: dict, x: np.ndarray) -> dict:
    """what lora_random_golden.npz keeps of one recording"""
    return {"in_sha256": lc.sha(x), "samples_sha256": lc.sha(np.concatenate(r["feeds"]).astype(np.int16)), "text": "".join(r["texts"]),
            "state": r["state"][-1, :6].copy(), "events": r["state"][-1, 6:].copy()}


def main_random(exe: str, out: str):
    """the recorder's digests of the random cases and of the named ones (tests/lora_cases.py: random_cases(), NAMED), so that
    tests/lora_oracle.cpp stays tied to the reference where there is none"""
    from tests import lora_cases as lc
    cases = lc.random_cases() + lc.NAMED
    ds = []
    for c in cases:
        x = lc.inputs(c)
        ds.append(digest(lc, record(exe, c, x), x))
    n_random = len(cases) - len(lc.NAMED)
    counters = [dict(zip(STATE + EVENTS, (int(v) for v in np.concatenate([d["state"], d["events"]])))) for d in ds]
    lc.assert_coverage(cases[:n_random], counters[:n_random], [d["text"] for d in ds[:n_random]], probes=False)
    text, text_bytes = pack_texts([d["text"] for d in ds])
    np.savez_compressed(out, names=np.array([c["name"] for c in cases]), in_sha256=np.array([d["in_sha256"] for d in ds]),
                        samples_sha256=np.array([d["samples_sha256"] for d in ds]), text=text, text_bytes=text_bytes,
                        state=np.array([d["state"] for d in ds], np.int64), events=np.array([d["events"] for d in ds], np.int64))
    print(f"wrote {out}: {len(cases)} cases, {os.path.getsize(out)} bytes")


def main():
    from tests import lora_cases as lc
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=None)
    ap.add_argument("--random", action="store_true", help="write lora_random_golden.npz: the recorder's digests of the random and the named cases")
    args = ap.parse_args()
    if not available(args.ref):
        sys.exit("reference tree or Qt headers not found")
    exe = build_recorder(args.ref)
    if args.random:
        return main_random(exe, args.out or os.path.join(HERE, "lora_random_golden.npz"))
    args.out = args.out or os.path.join(HERE, "lora_golden.npz")
    arrays, up, plain, short = {}, 0, 0, 0
    for c in lc.CASES:
        name, ex = c["name"], c["expect"]
        x = lc.inputs(c)
        r = record(exe, c, x)
        st, last = r["state"], r["state"][-1]
        text = "".join(r["texts"])
        lines = text.split("\n")[:-1]
        counts = np.array([f.shape[0] for f in r["feeds"]], np.int64)
        print(f"{name}: {int(counts.sum())} Samples, locks {int(last[9])} (finetune below zero {int(last[6])}, not {int(last[7])}), short closes {int(last[8])}, "
              f"wraps {int(last[10])}, tune {int(last[0])}, lines {lines}")
        assert int(last[5]) == len(lines) and int(last[4]) == int(counts.sum()), name
        if "locks" in ex:
            assert int(last[9]) >= ex["locks"], (name, int(last[9]))      # a preamble of eight symbols passes the test twice
        if "lines" in ex:
            assert len(lines) == ex["lines"], (name, lines)
        if ex.get("clip"):
            assert len(lines[0]) == 140 // 2 - 1, (name, len(lines[0]))
        if ex.get("wrap"):
            assert int(last[10]) >= 1, name
        if ex.get("short_close"):
            assert int(last[8]) >= 1, name
        if ex.get("silence"):
            assert int(last[9]) >= 1 and int(last[0]) == 0 and not np.concatenate(r["feeds"])[:, 1].any(), name
        if ex.get("edges"):
            ends = set(np.cumsum(counts).tolist())
            assert {63, 64, 65, 127, 128, 129} <= ends and 0 in counts and 1 in counts, (name, sorted(ends)[:16])
        up += int(last[6]); plain += int(last[7]); short += int(last[8])
        arrays[f"{name}/in_sha256"] = np.array(lc.sha(x))
        arrays[f"{name}/counts"] = counts
        arrays[f"{name}/samples"] = np.concatenate(r["feeds"]).astype(np.int16)
        arrays[f"{name}/text"], arrays[f"{name}/text_bytes"] = pack_texts(r["texts"])
        arrays[f"{name}/state"] = st[:, :6]
        arrays[f"{name}/events"] = last[6:]
        arrays[f"{name}/ntaps"] = np.array(r["ntaps"], np.int64)
        arrays[f"{name}/taps"] = r["taps"]
        if ex.get("trace"):
            arrays[f"{name}/trace"] = r["trace"]
    arrays["design/vrot"], arrays["design/k2"], arrays["design/chirp"], arrays["design/sample"] = r["vrot"], r["k2"], r["chirp"], r["sample"]
    assert up >= 1 and plain >= 1 and short >= 1, (up, plain, short)
    used = {c["cfg"][2] for c in lc.CASES}
    assert used >= set(lc.BANDWIDTHS), used
    assert float_cutoff_taps(7813, 7813), "7813's cutoff survives the float: pick another bandwidth for the cutoff test"
    np.savez_compressed(args.out, **arrays)
    print(f"wrote {args.out}: {len(lc.CASES)} cases, {os.path.getsize(args.out)} bytes")


if __name__ == "__main__":
    main()
