"""Rate of the ChannelAnalyzer bank (sdrx_chana_*) on device-resident samples, next to the SSB demodulator bank on the same streams.

--channels (32) x 1 s of channel-rate int16 I/Q at 48 kS/s (a tone over noise per channel) sit in HBM; each feed is a feed_dev of
the whole second.  Three analyzer configurations and the SSB bank take turns, feed by feed: 3 warm-up rounds, then --feeds timed
ones (>= 12): HIP events around each feed's kernels (set_timing), median, lowest and highest.  Clocks are left alone.
    signal_bypass      SSB filter, no Interpolator, span_log2 3
    signal_down        the same behind the Interpolator, 48000 -> 24000
    autocorrelation    the bypass configuration with input_type 2: 6000 calls per channel and second, a pair of 8192-point
                       transforms every 4096 of them
    ssb                sdrx_ssb_*, 48000 -> 48000, AGC on: the same NCO / Interpolator / runSSB front plus its audio tail

    python tools/chana_rate.py [--out profiles/chana_rate.txt]          one JSON line + a text report

--pll: the PLL row instead (sdrx_chanapll_*).  --channels (256 there) x 1 s at 48 kS/s, DSB filter, span_log2 0, so every sample is
one dependent step of PhaseLockComplex::feed (or FreqLockComplex::feed).  Three handles made by sdrx_chanapll_create on the same
streams take turns as above: pll_off (no loop: the parent's kernels), pll_on (order 1) and fll_on.  The walk kernel is the only
serial one, one wave per channel, so (on - off) / steps is the time of one dependent step with the post kernel's share in it.
The same work single-threaded on this machine's CPU: tests/chana_pll_oracle.c (the strict-IEEE restatement, -O2) on --cpu-channels
of the streams, front and filter included, next to the same oracle with the loop off.

    python tools/chana_rate.py --pll [--out profiles/chana_pll_rate.txt]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import sdrangel_amd as sa  # noqa: E402
from tests import chana_cases as cc  # noqa: E402
from tests import ssb_cases as sc  # noqa: E402
from tests import synth  # noqa: E402


def pll_report(args):
    import time

    import numpy as np

    from tests import chana_pll_cases as pc
    n_ch, feeds, in_rate = args.channels or 256, max(args.feeds, 12), args.in_rate
    n = in_rate
    host = [synth.mix(n, 900 + c, 30, 8000, 1) for c in range(n_ch)]
    dev = [torch.from_numpy(x).cuda() for x in host]
    torch.cuda.synchronize()
    ptrs, cnts = [t.data_ptr() for t in dev], [n] * n_ch

    def cfg(c, **kw):
        return pc._cfg(in_rate, nco_freq=-2950 - (c % 97), **kw)           # the tone sits 50 .. -46 Hz from the loop's centre

    def bank(**kw):
        return sa.ChannelAnalyzerBank([sa.ChanaCfg(**{k: v for k, v in cfg(c, **kw).items() if k != "psk_order"}) for c in range(n_ch)], psk_order=[1] * n_ch)

    banks = {"pll_off": bank(), "pll_on": bank(pll=1), "fll_on": bank(pll=1, fll=1)}
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
    res = {"tool": "chana_rate --pll", "channels": n_ch, "in_rate": in_rate, "samples_per_channel": n, "feeds": feeds}
    steps = banks["pll_on"].last_dev(0)[1]
    res["steps_per_channel_and_feed"] = steps
    for k, t in times.items():
        res[f"{k}_ms_per_feed"] = round(statistics.median(t), 4)
        res[f"{k}_ms_min"] = round(min(t), 4)
        res[f"{k}_ms_max"] = round(max(t), 4)
        res[f"{k}_kernel"] = banks[k].last_launch()
    res["locked_channels_after_the_last_feed"] = sum(int(banks["pll_on"].pll_state(c)[0]) for c in range(n_ch))
    for k in ("pll_on", "fll_on"):
        extra = res[f"{k}_ms_per_feed"] - res["pll_off_ms_per_feed"]
        res[f"{k}_walk_and_post_ms"] = round(extra, 4)
        res[f"{k}_walk_and_post_share"] = round(extra / res[f"{k}_ms_per_feed"], 4)
        res[f"{k}_ns_per_dependent_step"] = round(extra * 1e6 / max(steps, 1), 2)
        res[f"{k}_realtime_channels_per_feed_second"] = round(n_ch * 1000.0 / res[f"{k}_ms_per_feed"], 1)
    # one CPU thread on the same work
    L = pc.build_oracle()
    m = max(1, min(args.cpu_channels, n_ch))
    for k, kw in (("pll_off", {}), ("pll_on", dict(pll=1)), ("fll_on", dict(pll=1, fll=1))):
        oras = [pc.OraclePll(L, cfg(c, **kw)) for c in range(m)]
        for c in range(m):
            oras[c].feed(host[c][:2048])
        t0 = time.perf_counter()
        for c in range(m):
            oras[c].feed(host[c])
        res[f"cpu_oracle_{k}_ms_per_channel_second"] = round((time.perf_counter() - t0) * 1000.0 / m, 4)
    res["cpu_oracle_channels_timed"] = m
    for k in ("pll_on", "fll_on"):
        res[f"cpu_oracle_{k}_ns_per_step"] = round((res[f"cpu_oracle_{k}_ms_per_channel_second"] - res["cpu_oracle_pll_off_ms_per_channel_second"]) * 1e6 / max(steps, 1), 2)
        res[f"{k}_gpu_feed_over_one_cpu_thread"] = round(res[f"cpu_oracle_{k}_ms_per_channel_second"] * n_ch / res[f"{k}_ms_per_feed"], 2)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write("# tools/chana_rate.py --pll: %d channels x 1 s at %d S/s, device resident, three handles taking turns, median of %d feeds after 3 warm-up rounds\n"
                    % (n_ch, in_rate, feeds))
            for k, v in res.items():
                f.write(f"{k}: {v}\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=0)
    ap.add_argument("--pll", action="store_true")
    ap.add_argument("--cpu-channels", type=int, default=8)
    ap.add_argument("--in-rate", type=int, default=48000)
    ap.add_argument("--feeds", type=int, default=12)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.pll:
        return pll_report(args)
    n_ch, feeds, in_rate = args.channels or 32, max(args.feeds, 12), args.in_rate
    n = in_rate                                              # one second

    dev = [torch.from_numpy(synth.mix(n, 900 + c, 300, 6000, 1 + c % 3)).cuda() for c in range(n_ch)]
    torch.cuda.synchronize()
    ptrs, cnts = [t.data_ptr() for t in dev], [n] * n_ch

    def chana(**kw):
        cfgs = [dict(cc._cfg(in_rate, nco_freq=-500 - 37 * c, ssb=1, span_log2=3, **kw), pll=0, fll=0) for c in range(n_ch)]
        return sa.ChannelAnalyzerBank([sa.ChanaCfg(**k) for k in cfgs])

    banks = {"signal_bypass": chana(), "signal_down": chana(down_sample=1, down_sample_rate=in_rate // 2),
             "autocorrelation": chana(input_type=cc.AUTOCORR),
             "ssb": sa.SsbDemodBank([sa.SsbCfg(**sc._cfg(in_rate, in_rate, nco_freq=-500 - 37 * c, agc=1)) for c in range(n_ch)])}
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
    res = {"tool": "chana_rate", "channels": n_ch, "in_rate": in_rate, "samples_per_channel": n, "feeds": feeds}
    for k, t in times.items():
        res[f"{k}_ms_per_feed"] = round(statistics.median(t), 4)
        res[f"{k}_ms_min"] = round(min(t), 4)
        res[f"{k}_ms_max"] = round(max(t), 4)
        res[f"{k}_outputs_per_feed"] = sum(banks[k].last_dev(c)[1] for c in range(n_ch))
        res[f"{k}_kernel"] = banks[k].last_launch()
    for k in ("signal_bypass", "signal_down", "autocorrelation"):
        res[f"ratio_{k}_over_ssb"] = round(res[f"{k}_ms_per_feed"] / res["ssb_ms_per_feed"], 4)

    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write("# tools/chana_rate.py: %d channels x 1 s at %d S/s, device resident, four handles taking turns, median of %d feeds after 3 warm-up rounds\n"
                    % (n_ch, in_rate, feeds))
            for k, v in res.items():
                f.write(f"{k}: {v}\n")


if __name__ == "__main__":
    main()
