"""Rate of the DATV receiver bank (sdrx_datv_*) on device-resident samples.

--channels (64 and 256) x one second at 1 MS/s of channel-rate int16 I/Q (a QPSK signal per channel, tests/datv_cases.py) sit in
HBM; each feed is a feed_dev of all of them.  One bank per Fs / Fm (2 and 4), sampler (nearest, linear, RRC) and width; the ATV
bank takes turns on the same streams (FM3, its plain configuration), so that both are timed under the same clocks.  3 warm-up
feeds, then --feeds timed ones (>= 12): HIP events around each feed's kernels (set_timing), median, lowest and highest.  Clocks are
left alone.  The walk is the only serial kernel and every channel has a wave of its own, so a feed's time over its symbols is an
upper bound of the walk's time per symbol step (the front's mix and FFT filter are in it).

    python tools/datv_rate.py [--out profiles/datv_rate.txt]            one JSON line + a text report

From the time per sample: how many channels at 1 MS/s one bank carries in real time, and whether one channel at 2 MS/s runs in
real time on its one wave -- the samples of one second of one channel must pass the walk in under a second, whatever the bank's
width.

--cpu: the CPU figure instead, no GPU needed: the reference recorder (tests/golden/datv_rec.cpp around the reference's own NCO,
fftfilt and cstln_receiver, -O2, one thread) over one channel, where the reference tree is at hand.  It is not the same machine
as the GPU figures' host, and process start and file input and output are in its time.

    python tools/datv_rate.py --cpu [--ref DIR]
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
from tests import datv_cases as dc  # noqa: E402

SAMPLERS = (("nearest", dc.NEAREST), ("linear", dc.LINEAR), ("rrc", dc.RRC))
RATIOS = (2, 4)
RATE = 1000000


def config(ratio: int, sampler: int) -> dict:
    return dc.cfg(symbol_rate=RATE // ratio, rf_bandwidth=int(1.4 * RATE / ratio), sampler=sampler, finfo=0.0)


def stream(ratio: int, c: int, n: int):
    return dc.signal(dict(dc.PSK, start=0.1 * (c % 7), f0=500.0 * (c % 5)), config(ratio, dc.RRC), n, 700 + c)


def cpu_report(args):
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_golden_datv as mk
    if not mk.available(args.ref):
        sys.exit("reference tree or Qt headers not found")
    exe = mk.build_recorder(args.ref)
    res = {"tool": "datv_rate --cpu", "samples": args.samples,
           "note": "one core of the machine that has the reference, not the GPU figures' host; process start and file input and output are in the time"}
    for ratio in RATIOS:
        x = stream(ratio, 0, args.samples)
        for name, sampler in SAMPLERS:
            case = {"cfg": config(ratio, sampler), "splits": [args.samples]}
            best = None
            for _ in range(5):
                t0 = time.perf_counter()
                mk.record(exe, case, x)
                dt = time.perf_counter() - t0
                best = dt if best is None else min(best, dt)
            res[f"ratio{ratio}_{name}_recorder_s_best_of_5"] = round(best, 4)
            res[f"ratio{ratio}_{name}_recorder_msamples_per_second"] = round(args.samples / best / 1e6, 3)
    print(json.dumps(res))


def timed(bank, ptrs, cnts, feeds):
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
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--samples", type=int, default=RATE)
    ap.add_argument("--feeds", type=int, default=12)
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.cpu:
        return cpu_report(args)

    import torch

    import sdrangel_amd as sa

    feeds, n = max(args.feeds, 12), args.samples
    res = {"tool": "datv_rate", "samples_per_channel": n, "feeds": feeds, "msps": RATE, "modulation": "QPSK"}
    for ratio in RATIOS:
        uniq = [torch.from_numpy(stream(ratio, c, n)).cuda() for c in range(8)]         # eight different signals, repeated over the channels
        torch.cuda.synchronize()
        for n_ch in args.channels:
            ptrs, cnts = [uniq[c % 8].data_ptr() for c in range(n_ch)], [n] * n_ch
            banks = [(name, sa.DatvBank([dc.as_struct(config(ratio, sampler), sa.DatvCfg) for _ in range(n_ch)])) for name, sampler in SAMPLERS]
            banks.append(("atv_fm3", sa.ATVBank([ac.as_struct(ac.cfg(in_rate=RATE, scope=0, frames_cap=1), sa.AtvCfg) for _ in range(n_ch)])))
            for name, bank in banks:                        # in turns on the same streams
                t = timed(bank, ptrs, cnts, feeds)
                key = f"ratio{ratio}_{name}_{n_ch}ch"
                med = statistics.median(t)
                res[f"{key}_ms_per_feed"] = round(med, 4)
                res[f"{key}_ms_min"], res[f"{key}_ms_max"] = round(min(t), 4), round(max(t), 4)
                res[f"{key}_msamples_per_second"] = round(n_ch * n / med / 1000.0, 2)
                res[f"{key}_channels_in_real_time_at_1msps"] = round(n_ch * (n / RATE) / (med / 1000.0), 1)
                if name != "atv_fm3":
                    nsym = bank.last_dev(0)[2]
                    res[f"{key}_symbols_per_channel"] = nsym
                    res[f"{key}_ns_per_symbol_step_upper_bound"] = round(med * 1e6 / max(nsym, 1), 1)
                    res[f"{key}_seconds_per_second_of_one_channel_at_2msps"] = round(2.0 * med / 1000.0 / (n / RATE), 3)
                    res["kernel"] = bank.last_launch()
            del banks
    worst = max(v for k, v in res.items() if k.endswith("_seconds_per_second_of_one_channel_at_2msps"))
    res["one_channel_at_2msps_in_real_time_on_one_wave"] = bool(worst < 1.0)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write("# tools/datv_rate.py: banks of %s channels x %d samples at %d S/s, QPSK, device resident, median of %d feeds after 3 warm-up feeds\n"
                    % (args.channels, n, RATE, feeds))
            for k, v in res.items():
                f.write(f"{k}: {v}\n")


if __name__ == "__main__":
    main()
