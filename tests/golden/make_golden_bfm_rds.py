"""Builds tests/golden/bfm_rds_rec.cpp against the reference's own classes (what make_golden_bfm.py compiles, plus
plugins/channelrx/demodbfm/rdsdemod.cpp with its moc output and rdsdecoder.cpp, linked against QtCore for QObject) and records
tests/golden/bfm_rds_golden.npz for the cases of tests/bfm_rds_cases.py and its frameSync streams.

    python tests/golden/make_golden_bfm_rds.py [--ref /root/reference]
    python tests/golden/make_golden_bfm_rds.py --search      looks for the long case's phase, level, lead and cuts (prints them)
    python tests/golden/make_golden_bfm_rds.py --random      records tests/golden/bfm_rds_random_golden.npz for bfm_rds_cases.random_cases()

Per case and feed the fixture keeps the bits, the groups, the RDS sample count, the report and the state words
(bfm_rds_cases.STATE_FIELDS); subcarr_bb in full for cases up to BB_FULL samples, beyond that per feed its sha256 and the first
and last BB_EDGE values; audio and sink stream for AUDIO_CASE.  Inputs are kept as their sha256: the generator is portable.
The recorder also runs rds_mix.hpp on its own demod and phase: no case may have an unsure sample, and rds_mix's product must
equal the host's on every sample (asserted here).  `host` notes the libm the recorder ran on.

The random draw's fixture keeps every case the long cases' way (subcarr_bb as sha256, head and tail).  A draw whose recording has an
unsure sample is not recorded: the run stops and names the index for bfm_rds_cases.RANDOM_SKIP.  The indices already there are
recorded too, to see that each does have such a sample; `unsure_skipped` is their number.  Fixed zip timestamps: the same recording
gives the same bytes."""
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
sys.path.insert(0, HERE)

import make_golden_bfm as mg                     # noqa: E402

QTLIB = os.environ.get("QTLIB", "/opt/conda/lib")
MOC = os.environ.get("MOC", "/opt/conda/bin/moc")
RDS_DIR = ("plugins", "channelrx", "demodbfm")


def available(ref: str) -> bool:
    return mg.available(ref) and os.path.isfile(os.path.join(ref, *RDS_DIR, "rdsdemod.cpp")) and os.path.isfile(os.path.join(QTLIB, "libQt5Core.so.5"))


def build_recorder(ref: str) -> str:
    d = tempfile.mkdtemp()
    exe = os.path.join(d, "bfm_rds_rec")
    rds = os.path.join(ref, *RDS_DIR)
    inc = ["-I" + mg.QTINC, "-I" + os.path.join(mg.QTINC, "QtCore"), "-I" + os.path.join(ref, "sdrbase"), "-I" + os.path.join(ref, "exports"), "-I" + rds]
    moc_out = os.path.join(d, "moc_rdsdemod.cpp")
    subprocess.check_call([MOC] + inc + [os.path.join(rds, "rdsdemod.h"), "-o", moc_out])
    flags = ["-O2", "-std=c++11", "-fPIC", "-fno-fast-math", "-ffp-contract=off", "-w", "-DQT_NO_VERSION_TAGGING", "-DQT_NO_DEBUG_OUTPUT",
             "-Dsdrangel_STATIC", "-I" + os.path.join(ROOT, "sdrangel_amd", "csrc")] + inc
    srcs = [os.path.join(ref, "sdrbase", "dsp", s) for s in mg.SOURCES] + [os.path.join(rds, "rdsdemod.cpp"), os.path.join(rds, "rdsdecoder.cpp"), moc_out]
    subprocess.check_call(["g++"] + flags + [os.path.join(HERE, "bfm_rds_rec.cpp")] + srcs +
                          [os.path.join(QTLIB, "libQt5Core.so.5"), "-Wl,-rpath," + QTLIB, "-Wl,-rpath-link," + QTLIB, "-o", exe])
    return exe


def record(exe: str, cfg: dict, rds: int, iq: np.ndarray, splits) -> dict:
    from tests.bfm_cases import FIELDS
    from tests.bfm_rds_cases import STATE_FIELDS
    d = tempfile.mkdtemp()
    fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
    with open(fin, "wb") as f:
        f.write(np.ascontiguousarray(iq, np.int16).tobytes())
    word = lambda k: "%.9g" % float(np.float32(cfg[k])) if k in ("rf", "af", "vol", "sq") else str(int(cfg[k]))
    cmds = ["new " + " ".join(word(k) for k in FIELDS) + f" {int(rds)}"] + [f"feed {int(m)}" for m in splits]
    subprocess.run([exe, fin, fout], input="\n".join(cmds) + "\n", text=True, check=True, timeout=900)
    raw = open(fout, "rb").read()
    os.remove(fin); os.remove(fout)
    res = {k: [] for k in ("audio", "sink", "bits", "bit_at", "groups", "group_at", "bb", "cr", "unsure", "differs", "report", "state")}
    pos = 0

    def take(dtype, n):
        nonlocal pos
        a = np.frombuffer(raw, dtype, n, pos).copy()
        pos += a.nbytes
        return a

    for _ in splits:
        k = int(take(np.int64, 1)[0]); res["audio"].append(take(np.int16, 2 * k).reshape(k, 2))
        m = int(take(np.int64, 1)[0]); res["sink"].append(take(np.int16, m))
        nb = int(take(np.int64, 1)[0]); res["bits"].append(take(np.uint8, nb)); res["bit_at"].append(take(np.int32, nb))
        ng = int(take(np.int64, 1)[0]); res["groups"].append(take(np.uint16, 4 * ng).reshape(ng, 4)); res["group_at"].append(take(np.int32, ng))
        nr = int(take(np.int64, 1)[0]); res["bb"].append(take(np.float32, nr)); res["cr"].append(take(np.float32, nr))
        res["unsure"].append(int(take(np.int64, 1)[0])); res["differs"].append(int(take(np.int64, 1)[0]))
        res["report"].append(take(np.uint32, 5))
        res["state"].append(take(np.uint64, len(STATE_FIELDS)))
    assert pos == len(raw)
    return res


def record_framesync(exe: str, bits: np.ndarray) -> np.ndarray:
    d = tempfile.mkdtemp()
    fin, fout = os.path.join(d, "bits.bin"), os.path.join(d, "out.bin")
    with open(fin, "wb") as f:
        f.write(np.ascontiguousarray(bits, np.uint8).tobytes())
    subprocess.check_call([exe, "--framesync", fin, fout])
    raw = np.frombuffer(open(fout, "rb").read(), np.uint8).reshape(-1, 10)
    out = np.empty((raw.shape[0], 6), np.uint16)
    out[:, 0], out[:, 1] = raw[:, 0], raw[:, 1]
    out[:, 2:] = raw[:, 2:].copy().view(np.uint16)
    return out


def walk_of(res: dict, sync_col: int) -> str:
    """which decoder states the feeds ended in"""
    return "".join("S" if int(s[sync_col]) else "n" for s in res["state"])


def search(exe: str):
    """the long case: one feed per block, so that every block's end is a feed's end; the decoder must leave SYNC (the 50-block
    count), come back (presync, sync), complete at least three groups behind that, one of them on a block's last RDS sample"""
    from tests import bfm_rds_cases as rc
    from tests import bfm_cases as bc
    cfg = rc.LONG_CFG
    sync_col = rc.STATE_FIELDS.index("sync")
    nblk = rc.LONG_N // 512
    for level in (4000.0, 6000.0, 3000.0):
        for phi in (np.pi / 2, 0.0, np.pi, 3 * np.pi / 2, np.pi / 4):
            for lead in range(0, 4096, 37):
                sig = dict(rc.LONG_SIG, rds=level, rds_phi=float(phi), lead=lead)
                x = rc.signal(sig, rc.LONG_N, cfg["in_rate"], rc.LONG_SEED)
                r = record(exe, cfg, 1, x, [512] * nblk)
                w = walk_of(r, sync_col)
                ngroups = [g.shape[0] for g in r["groups"]]
                lost = w.find("n")
                back = w.find("S", lost) if lost >= 0 else -1
                after = sum(ngroups[back:]) if back >= 0 else 0
                print(f"level {level} phi {phi:.3f} lead {lead}: lost at block {lost}, back at {back}, groups after {after}, unsure {sum(r['unsure'])}", flush=True)
                if back < 0 or after < 3:
                    break                                  # this phase and level do not decode: next phase
                if sum(r["unsure"]):
                    continue
                g_last = [i for i in range(back, nblk) if ngroups[i] and r["group_at"][i][-1] == r["bb"][i].size - 1]
                b_last = [i for i in range(nblk) if r["bits"][i].size and r["bit_at"][i][-1] == r["bb"][i].size - 1 and not (ngroups[i] and r["group_at"][i][-1] == r["bb"][i].size - 1)]
                if g_last and b_last:
                    print("FOUND", sig, "group on the last sample of blocks", g_last, "bit on the last sample of blocks", b_last[:8])
                    return
    print("nothing found")


def case_arrays(arrays: dict, c: dict, x: np.ndarray, r: dict, bb_full: bool):
    """one case's bits, groups, RDS sample counts, subcarr_bb (in full or as digests and edges), report and state words"""
    from tests import bfm_rds_cases as rc
    from tests import bfm_cases as bc
    name = c["name"]
    arrays[f"{name}/in_sha256"] = np.array(bc.sha(x))
    arrays[f"{name}/bit_counts"] = np.array([b.size for b in r["bits"]], np.int64)
    arrays[f"{name}/bits"] = np.concatenate(r["bits"])
    arrays[f"{name}/group_counts"] = np.array([g.shape[0] for g in r["groups"]], np.int64)
    arrays[f"{name}/groups"] = np.concatenate(r["groups"]).reshape(-1, 4)
    arrays[f"{name}/rds_counts"] = np.array([b.size for b in r["bb"]], np.int64)
    if bb_full:
        arrays[f"{name}/bb"] = np.concatenate(r["bb"])
    else:
        arrays[f"{name}/bb_sha256"] = np.array([rc.sha_f32(b) for b in r["bb"]])
        arrays[f"{name}/bb_head"] = np.array([np.resize(b[:rc.BB_EDGE], rc.BB_EDGE) if b.size else np.zeros(rc.BB_EDGE, np.float32) for b in r["bb"]], np.float32)
        arrays[f"{name}/bb_tail"] = np.array([np.resize(b[-rc.BB_EDGE:], rc.BB_EDGE) if b.size else np.zeros(rc.BB_EDGE, np.float32) for b in r["bb"]], np.float32)
    arrays[f"{name}/report"] = np.array(r["report"], np.uint32).reshape(-1, 5)
    arrays[f"{name}/state"] = np.array(r["state"], np.uint64).reshape(-1, len(rc.STATE_FIELDS))


def record_random(exe: str, out: str):
    from tests import bfm_rds_cases as rc
    kept, left = rc.random_draws()
    for c in left:
        r = record(exe, c["cfg"], c["rds"], rc.inputs(c), c["splits"])
        assert sum(r["unsure"]) > 0, (c["name"], "is in RANDOM_SKIP and has no unsure sample")
    results = []
    for c in kept:
        r = record(exe, c["cfg"], c["rds"], rc.inputs(c), c["splits"])
        if sum(r["unsure"]):
            sys.exit(f"{c['name']} has {sum(r['unsure'])} unsure sample(s): add its index to bfm_rds_cases.RANDOM_SKIP and record again")
        assert sum(r["differs"]) == 0, (c["name"], "rds_mix differs from the host's product", r["differs"])
        results.append(r)
        print(f"{c['name']}: {c['cfg']['in_rate']} S/s, {len(c['splits'])} feeds, rds samples {sum(b.size for b in r['bb'])}, "
              f"bits {sum(b.size for b in r['bits'])}, groups {sum(g.shape[0] for g in r['groups'])}", flush=True)
    arrays = rc.pack_random(kept, results)
    arrays.update(host=np.array(mg.host_note()), state_fields=np.array(rc.STATE_FIELDS), unsure_skipped=np.array(len(left), np.int64))
    mg.save_npz(out, arrays)
    print(f"wrote {out}: {len(kept)} cases, {len(left)} skipped, {os.path.getsize(out)} bytes")
    print(rc.random_shares(kept, rc.load_random_golden(out)))


def main():
    from tests import bfm_rds_cases as rc
    from tests import bfm_cases as bc
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=None)
    ap.add_argument("--search", action="store_true")
    ap.add_argument("--random", action="store_true")
    args = ap.parse_args()
    if not available(args.ref):
        sys.exit("reference tree, Qt headers or QtCore not found")
    exe = build_recorder(args.ref)
    if args.search:
        return search(exe)
    if args.random:
        return record_random(exe, args.out or rc.RANDOM_GOLDEN)
    args.out = args.out or rc.GOLDEN
    arrays = {"host": np.array(mg.host_note()), "state_fields": np.array(rc.STATE_FIELDS)}
    sync_col = rc.STATE_FIELDS.index("sync")
    for c in rc.CASES:
        x = rc.inputs(c)
        r = record(exe, c["cfg"], c["rds"], x, c["splits"])
        name = c["name"]
        assert sum(r["unsure"]) == 0, (name, "unsure samples: pick another seed", r["unsure"])
        assert sum(r["differs"]) == 0, (name, "rds_mix differs from the host's product", r["differs"])
        case_arrays(arrays, c, x, r, bb_full=c["n"] <= rc.BB_FULL)
        if name == rc.CR_CASE:                       # what RDSDemod::process was given: the CPU test drives bfm_rds.hpp with it
            arrays[f"{name}/cr"] = np.concatenate(r["cr"])
        if name == rc.AUDIO_CASE:
            arrays[f"{name}/audio_counts"] = np.array([a.shape[0] for a in r["audio"]], np.int64)
            arrays[f"{name}/audio"] = np.concatenate(r["audio"])
            arrays[f"{name}/sink_counts"] = np.array([s.size for s in r["sink"]], np.int64)
            arrays[f"{name}/sink"] = np.concatenate(r["sink"])
        print(f"{name}: rds samples {sum(b.size for b in r['bb'])}, bits {sum(b.size for b in r['bits'])}, groups {sum(g.shape[0] for g in r['groups'])}, "
              f"sync per feed {walk_of(r, sync_col)}")
    for name, bits in rc.framesync_streams().items():
        out = record_framesync(exe, bits)
        arrays[f"fs/{name}/out"] = out
        print(f"framesync {name}: {bits.size} bits, groups {int(out[:, 0].sum())}, synced at the end {int(out[-1, 1])}, ever unsynced {int((out[:, 1] == 0).any())}")
    np.savez_compressed(args.out, **arrays)
    print(f"wrote {args.out}: {len(rc.CASES)} cases on {mg.host_note()}, {os.path.getsize(args.out)} bytes")


if __name__ == "__main__":
    main()
