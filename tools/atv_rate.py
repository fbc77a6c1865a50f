"""Rate of the ATV demodulator bank (sdrx_atv_*) on device-resident samples.

--channels x --samples of channel-rate int16 I/Q (a synthetic picture per channel, tests/atv_cases.py: 64 lines of 100 samples)
sit in HBM; each feed is a feed_dev of all of them.  One bank per modulation (FM1, FM2, FM3, AM) and bank width (64 and 256
channels), then FM1 and AM with the decimator, with the FFT filter and with both: 3 warm-up feeds, then --feeds timed ones (>=
12): HIP events around each feed's kernels (set_timing), median, lowest and highest.  Clocks are left alone.  The walk is the only serial kernel and every channel has a wave of its own, so a feed's time
over its samples is an upper bound of the walk's time per sample (the front and the video kernel are in it); a kernel trace of
this tool, taken in a run of its own, gives the walk alone:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/atv_rate.py --feeds 12
    python tools/atv_rate.py [--out profiles/atv_rate.txt]            one JSON line + a text report

From the time per sample: how many PAL-625 channels at their own rate (--pal-rate, 10 MS/s) one walk wave per channel carries in
real time -- the samples of one second of one channel must pass the walk in under a second, whatever the bank's width.

--cpu: the CPU figure instead, no GPU needed: the reference recorder (tests/golden/atv_rec.cpp around the reference's own
ATVDemod, -O2, one thread) over one channel, where the reference tree is at hand.

    python tools/atv_rate.py --cpu [--ref DIR]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import atv_cases as ac  # noqa: E402

MODS = (("fm1", ac.FM1), ("fm2", ac.FM2), ("fm3", ac.FM3), ("am", ac.AM))
#: (name, modulation, what differs from the plain configuration): the plain banks, then the two optional stages
BANKS = tuple((name, mod, {}) for name, mod in MODS) + (
    ("fm1_decimator", ac.FM1, dict(decimator_enable=1)), ("fm1_fftfilter", ac.FM1, dict(fft_filtering=1)),
    ("fm1_decimator_fftfilter", ac.FM1, dict(decimator_enable=1, fft_filtering=1)),
    ("am_decimator", ac.AM, dict(decimator_enable=1)), ("am_fftfilter", ac.AM, dict(fft_filtering=1)))


def stream(mod: int, c: int, n: int):
    k = ac.cfg(modulation=mod)
    return ac.signal({"kind": "video", "fields": [ac.SMALL_LINES], "sigma": 60.0, "lead": 13 * (c % 7)}, k, n, 500 + c)


def cpu_report(args):
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_golden_atv as mk
    if not mk.available(args.ref):
        sys.exit("reference tree, moc or Qt not found")
    exe = mk.build_recorder(args.ref)
    res = {"tool": "atv_rate --cpu", "samples": args.samples, "note": "process start, file input and output and one feed() call per sample are in the time"}
    for name, mod in MODS:
        case = {"cfg": ac.cfg(modulation=mod, scope=0), "splits": [args.samples]}
        x = stream(mod, 0, args.samples)
        best = None
        for _ in range(5):
            t0 = time.perf_counter()
            mk.record(exe, case, x)
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        res[f"{name}_recorder_s_best_of_5"] = round(best, 4)
        res[f"{name}_recorder_msamples_per_second"] = round(args.samples / best / 1e6, 3)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--samples", type=int, default=160000)
    ap.add_argument("--feeds", type=int, default=12)
    ap.add_argument("--pal-rate", type=float, default=10.0e6)
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.cpu:
        return cpu_report(args)

    import torch

    import sdrangel_amd as sa

    feeds, n = max(args.feeds, 12), args.samples
    res = {"tool": "atv_rate", "samples_per_channel": n, "feeds": feeds, "in_rate": ac.SMALL_RATE, "lines": ac.SMALL_LINES}
    for name, mod, extra in BANKS:
        uniq = [torch.from_numpy(stream(mod, c, n)).cuda() for c in range(8)]          # eight different pictures, repeated over the channels
        torch.cuda.synchronize()
        for n_ch in args.channels:
            bank = sa.ATVBank([ac.as_struct(ac.cfg(modulation=mod, scope=0, frames_cap=2, **extra), sa.AtvCfg) for _ in range(n_ch)])
            ptrs, cnts = [uniq[c % 8].data_ptr() for c in range(n_ch)], [n] * n_ch
            for _ in range(3):
                bank.feed_dev(ptrs, cnts)
            bank.sync()
            bank.set_timing(True)
            t = []
            for _ in range(feeds):
                bank.feed_dev(ptrs, cnts)
                ms, cnt = bank.get_timing(reset=True)
                assert cnt == 1
                t.append(ms)
            key = f"{name}_{n_ch}ch"
            med = statistics.median(t)
            res[f"{key}_ms_per_feed"] = round(med, 4)
            res[f"{key}_ms_min"], res[f"{key}_ms_max"] = round(min(t), 4), round(max(t), 4)
            res[f"{key}_msamples_per_second"] = round(n_ch * n / med / 1000.0, 2)
            res[f"{key}_ns_per_sample_of_a_channel_upper_bound"] = round(med * 1e6 / n, 2)
            res[f"{key}_renders_in_last_feed"] = sum(bank.frames(c)[1] for c in range(n_ch))
            res["kernel"] = bank.last_launch()
            del bank
    worst = max(v for k, v in res.items() if k.endswith("_ns_per_sample_of_a_channel_upper_bound"))
    for stage in ("decimator", "fftfilter", "decimator_fftfilter"):
        for n_ch in args.channels:
            a, b = f"fm1_{stage}_{n_ch}ch_ms_per_feed", f"fm1_{n_ch}ch_ms_per_feed"
            if a in res:
                res[f"fm1_{stage}_{n_ch}ch_ms_over_plain"] = round(res[a] - res[b], 4)
    res["pal625_rate"] = args.pal_rate
    res["pal625_realtime"] = bool(worst * 1e-9 * args.pal_rate < 1.0)
    res["pal625_seconds_of_walk_per_second_of_signal"] = round(worst * 1e-9 * args.pal_rate, 3)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write("# tools/atv_rate.py: banks of %s channels x %d samples at %d S/s, device resident, median of %d feeds after 3 warm-up feeds\n"
                    % (args.channels, n, ac.SMALL_RATE, feeds))
            for k, v in res.items():
                f.write(f"{k}: {v}\n")


if __name__ == "__main__":
    main()
