"""Rate of the LoRa demodulator bank (sdrx_lora_*) on device-resident samples, next to the ChannelAnalyzer bank on the same streams.

--channels (256) x 1 s of channel-rate int16 I/Q at 62500 S/s (a LoRa-like frame over noise per channel, tests/lora_cases.py) sit
in HBM; each feed is a feed_dev of the whole second.  The LoRa bank at bandwidth 62500 (distance step 1: every input is one output,
one dependent step of the two sliding FFTs: 2 x 127 complex multiply-adds) and the ChannelAnalyzer bank with its PLL off and on
(one dependent step of PhaseLockComplex::feed per sample) take turns, feed by feed: 3 warm-up rounds, then --feeds timed ones (>=
12): HIP events around each feed's kernels (set_timing), median, lowest and highest.  Clocks are left alone.  The walk is the only
serial kernel and every channel has a wave of its own, so the LoRa feed's time over its steps is an upper bound of the time per
dependent step (the front, the dechirp and the carry are in it).

The question of one wave per channel against two or four is put to tools/ubench_lora_walk (the recurrence alone, the waves of a
channel meeting through LDS and a barrier every 64 steps), started as a child process; its line is merged in.

    python tools/lora_rate.py [--out profiles/lora_rate.txt]          one JSON line + a text report

--cpu: the CPU figure instead, no GPU needed: the reference recorder (tests/golden/lora_rec.cpp around the reference's own classes,
-O2, one thread) over one channel's second, where the reference tree is at hand.

    python tools/lora_rate.py --cpu [--ref DIR]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import lora_cases as lc  # noqa: E402

RATE = 62500


def stream(c: int):
    return lc.signal({"kind": "frames", "frames": [lc.frame(200, 40 + c % 90)], "lead": 0}, RATE, (RATE, 0, RATE), 700 + c)


def cpu_report(args):
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_golden_lora as mk
    if not mk.available(args.ref):
        sys.exit("reference tree or Qt headers not found")
    exe = mk.build_recorder(args.ref)
    case = {"cfg": (RATE, 0, RATE), "splits": [RATE]}
    x = stream(0)
    mk.record(exe, case, x[: 2 * 4096], splits=[4096])                      # warm the page cache
    best = None
    for _ in range(5):
        t0 = time.perf_counter()
        mk.record(exe, case, x)
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    res = {"tool": "lora_rate --cpu", "samples": RATE, "recorder_s_best_of_5": round(best, 4), "recorder_samples_per_second": round(RATE / best, 1),
           "note": "process start, file input and output and the per-fetch trace are in the time"}
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=256)
    ap.add_argument("--feeds", type=int, default=12)
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--no-ubench", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.cpu:
        return cpu_report(args)

    import torch

    import sdrangel_amd as sa
    from tests import chana_pll_cases as pc

    n_ch, feeds, n = args.channels, max(args.feeds, 12), RATE
    uniq = [stream(c) for c in range(min(n_ch, 8))]                         # eight different frames, repeated over the channels
    dev = [torch.from_numpy(uniq[c % len(uniq)]).cuda() for c in range(n_ch)]
    torch.cuda.synchronize()
    ptrs, cnts = [t.data_ptr() for t in dev], [n] * n_ch

    def chana(**kw):
        cfgs = [pc._cfg(RATE, nco_freq=-2950 - (c % 97), **kw) for c in range(n_ch)]
        return sa.ChannelAnalyzerBank([sa.ChanaCfg(**{k: v for k, v in k_.items() if k != "psk_order"}) for k_ in cfgs], psk_order=[1] * n_ch)

    banks = {"lora": sa.LoraDemodBank([sa.LoraCfg(in_rate=RATE, nco_freq=0, bandwidth=RATE) for _ in range(n_ch)]),
             "chana_pll_off": chana(), "chana_pll_on": chana(pll=1)}
    for _ in range(3):
        for b in banks.values():
            b.feed_dev(ptrs, cnts)
    times = {k: [] for k in banks}
    for b in banks.values():
        b.sync()
        b.set_timing(True)
    for _ in range(feeds):
        for k, b in banks.items():
            b.feed_dev(ptrs, cnts)
            ms, cnt = b.get_timing(reset=True)
            assert cnt == 1
            times[k].append(ms)
    res = {"tool": "lora_rate", "channels": n_ch, "in_rate": RATE, "bandwidth": RATE, "samples_per_channel": n, "feeds": feeds}
    for k, t in times.items():
        res[f"{k}_ms_per_feed"] = round(statistics.median(t), 4)
        res[f"{k}_ms_min"] = round(min(t), 4)
        res[f"{k}_ms_max"] = round(max(t), 4)
        res[f"{k}_kernel"] = banks[k].last_launch()
    steps = banks["lora"].last_dev(0)[1]
    res["lora_steps_per_channel_and_feed"] = steps
    res["lora_lines_so_far"] = sum(banks["lora"].state(c).lines for c in range(n_ch))
    res["lora_ns_per_dependent_step_upper_bound"] = round(res["lora_ms_per_feed"] * 1e6 / max(steps, 1), 2)
    res["lora_realtime_channels_per_feed_second"] = round(n_ch * 1000.0 / res["lora_ms_per_feed"], 1)
    res["lora_msamples_per_second"] = round(n_ch * steps / res["lora_ms_per_feed"] / 1000.0, 2)
    csteps = banks["chana_pll_on"].last_dev(0)[1]
    res["chana_walk_ns_per_dependent_step"] = round((res["chana_pll_on_ms_per_feed"] - res["chana_pll_off_ms_per_feed"]) * 1e6 / max(csteps, 1), 2)
    if not args.no_ubench:
        exe = os.path.join(ROOT, "tools", "ubench_lora_walk")
        out = subprocess.run([exe, str(n_ch), str(n), "9"], capture_output=True, text=True, timeout=300, check=True).stdout
        res["wave_split"] = json.loads(out)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write("# tools/lora_rate.py: %d channels x 1 s at %d S/s, device resident, three handles taking turns, median of %d feeds after 3 warm-up rounds\n"
                    % (n_ch, RATE, feeds))
            for k, v in res.items():
                f.write(f"{k}: {v}\n")


if __name__ == "__main__":
    main()
