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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=32)
    ap.add_argument("--in-rate", type=int, default=48000)
    ap.add_argument("--feeds", type=int, default=12)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    n_ch, feeds, in_rate = args.channels, max(args.feeds, 12), args.in_rate
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
