"""Rate of the broadcast-FM stereo demodulator bank (sdrx_bfm_*) on device-resident samples, next to its yardsticks.

256 channels x 1 s of channel-rate int16 I/Q at 240 kS/s -> 48 kS/s (a stereo multiplex per channel: L+R, the 19 kHz pilot, L-R on
38 kHz, FM-modulated, plus noise; tests/bfm_cases.py) sit in HBM.  Three handles take turns feed by feed on the same streams: the
BFM bank with audio_stereo set in every channel, the BFM bank in mono, and the WFM bank (sdrx_wfm_*).  Each feed is feed_dev of the
whole second.  2 warm-up rounds, then --feeds timed ones: HIP events around each feed's kernels (set_timing), median.  Clocks are
left alone.

What the figures are for:
  walk share      stereo minus mono: the pilot walk (bfm_walk_kernel) and the two parallel kernels only a stereo channel needs
  per step        the walk share over the dependent steps of one channel (all channels walk at once, one wave each), next to the
                  ChannelAnalyzer walk's figure measured in the same run (tools/chana_rate.py's PLL handle against its loops-off handle,
                  256 channels x 48000 steps)
  mono over WFM   the mono handle against the WFM bank: the exact atan2f and the two de-emphasis walks are the difference

Also prints the single-thread time of the CPU restatement (tests/bfm_oracle.c) for one channel's second: a baseline, not a target.

    python tools/bfm_rate.py [--out profiles/bfm_rate.txt]

--rds measures RDS instead (sdrx_bfmrds_*): the stereo handle with RDS off and with RDS on in every channel take turns on the same
256 streams, which then carry a 57 kHz RDS subcarrier (tests/bfm_rds_cases.py), next to the mono handle.  The RF filter is 200 kHz
wide so that the subcarrier passes.
  rds share       RDS on minus RDS off: the mixer, the RDS resampler and its schedule, the RDS walk (bfm_rds_walk_kernel), the
                  phases the pilot walk stores
  per step        the RDS share over one channel's RDS samples (250 000 a second), next to the pilot walk's share over its steps

    python tools/bfm_rate.py --rds [--in-rate 384000] [--out profiles/bfm_rds_rate.txt]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import sdrangel_amd as sa  # noqa: E402
from tests import bfm_cases as bc  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=256)
    ap.add_argument("--in-rate", type=int, default=240000)
    ap.add_argument("--feeds", type=int, default=8)
    ap.add_argument("--distinct", type=int, default=8, help="distinct streams synthesised; the channels cycle through them")
    ap.add_argument("--no-baseline", action="store_true", help="skip the ChannelAnalyzer walk and the CPU oracle")
    ap.add_argument("--rds", action="store_true", help="RDS on against RDS off (see above)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.rds:
        return rds_main(args)
    n_ch, feeds, in_rate = args.channels, max(args.feeds, 5), args.in_rate
    n = in_rate                                              # one second
    rf, af = 80000.0, 15000.0

    host, dev = [], []
    for c in range(min(args.distinct, n_ch)):
        f0 = -20000.0 + 5000.0 * c
        x = bc.signal({"kind": "mpx", "f0": f0, "fs": 400.0 + 100.0 * c, "amp": 6000.0}, n, in_rate, 900 + c)
        host.append(x); dev.append(torch.from_numpy(x).cuda())
    torch.cuda.synchronize()
    k = len(dev)
    ptrs, cnts = [dev[c % k].data_ptr() for c in range(n_ch)], [n] * n_ch
    ncos = [-int(-20000.0 + 5000.0 * (c % k)) for c in range(n_ch)]

    def bfm(stereo):
        return sa.BfmBank([sa.BfmCfg(in_rate=in_rate, nco_freq=ncos[c], audio_rate=48000, rf_bandwidth=rf, af_bandwidth=af, volume=2.0,
                                     squelch_db=-60.0, audio_stereo=stereo, lsb_stereo=0, show_pilot=0) for c in range(n_ch)])
    handles = {"stereo": bfm(1), "mono": bfm(0),
               "wfm": sa.WfmDemodBank([sa.WfmCfg(in_rate=in_rate, nco_freq=ncos[c], audio_rate=48000, rf_bandwidth=rf, af_bandwidth=af, volume=2.0,
                                                 squelch_db=-60.0, audio_mute=0) for c in range(n_ch)])}
    chana_n = 48000
    if not args.no_baseline:
        # the ChannelAnalyzer walk re-measured here: 256 channels x 48000 dependent steps of PhaseLockComplex::feed (span 0, PLL on)
        cc = sa.ChanaCfg(in_rate=48000, nco_freq=0, down_sample=0, down_sample_rate=0, bandwidth=5000, low_cutoff=300, span_log2=0, ssb=0, rrc=0,
                         rrc_rolloff=35, input_type=0, pll=1, fll=0)
        handles["chana_pll"] = sa.ChannelAnalyzerBank([cc] * n_ch, psk_order=[1] * n_ch)
        cc0 = sa.ChanaCfg(in_rate=48000, nco_freq=0, down_sample=0, down_sample_rate=0, bandwidth=5000, low_cutoff=300, span_log2=0, ssb=0, rrc=0,
                          rrc_rolloff=35, input_type=0, pll=0, fll=0)
        handles["chana_off"] = sa.ChannelAnalyzerBank([cc0] * n_ch, psk_order=[1] * n_ch)
    args_of = {name: (ptrs, [chana_n] * n_ch if name.startswith("chana") else cnts) for name in handles}

    for _ in range(2):
        for name, h in handles.items():
            h.feed_dev(*args_of[name])
    for h in handles.values():
        h.sync(); h.set_timing(True)
    times = {name: [] for name in handles}
    for _ in range(feeds):
        for name, h in handles.items():
            h.feed_dev(*args_of[name])
            ms, cnt = h.get_timing(reset=True)
            assert cnt == 1
            times[name].append(ms)
    med = {name: statistics.median(t) for name, t in times.items()}
    res = {"tool": "bfm_rate", "channels": n_ch, "in_rate": in_rate, "samples_per_channel": n, "feeds": feeds}
    for name, t in times.items():
        res[f"{name}_ms_per_feed"] = round(med[name], 4)
        res[f"{name}_ms_min_max"] = [round(min(t), 4), round(max(t), 4)]
    walk = med["stereo"] - med["mono"]
    res["walk_share_ms"] = round(walk, 4)
    res["walk_us_per_dependent_step"] = round(walk * 1e3 / n, 5)
    res["mono_minus_wfm_ms"] = round(med["mono"] - med["wfm"], 4)
    res["mono_over_wfm"] = round(med["mono"] / med["wfm"], 4)
    res["stereo_kernel"] = handles["stereo"].last_launch()
    locked = sum(int(handles["stereo"].pilot(c)[0]) for c in range(n_ch))
    res["stereo_channels_locked"] = locked
    if not args.no_baseline:
        cw = med["chana_pll"] - med["chana_off"]
        res["chana_walk_share_ms"] = round(cw, 4)
        res["chana_walk_us_per_dependent_step"] = round(cw * 1e3 / chana_n, 5)
        L = bc.build_oracle()
        o = bc.OracleBfm(L, dict(in_rate=in_rate, nco_freq=ncos[0], audio_rate=48000, rf=rf, af=af, vol=2.0, sq=-60.0, stereo=1, lsb=0, pilot=0))
        t0 = time.perf_counter()
        o.feed(host[0])
        res["oracle_cpu_single_thread_s_per_channel_second"] = round(time.perf_counter() - t0, 4)

    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write("# tools/bfm_rate.py: %d channels x 1 s at %d S/s -> 48 kS/s, device resident, the handles taking turns, median of %d feeds "
                    "after 2 warm-up rounds (HIP events around each feed's kernels)\n" % (n_ch, in_rate, feeds))
            for key, v in res.items():
                f.write(f"{key}: {v}\n")


def rds_main(args):
    from tests import bfm_rds_cases as rc
    n_ch, feeds, in_rate = args.channels, max(args.feeds, 5), args.in_rate
    n = in_rate
    rf, af = 200000.0 if in_rate >= 250000 else 0.75 * in_rate, 15000.0
    dev = []
    for c in range(min(args.distinct, n_ch)):
        x = rc.signal({"kind": "mpx", "rds": 4000.0, "rds_phi": 1.5707963267948966, "fs": 400.0 + 100.0 * c, "sum": 8000.0, "diff": 4000.0, "amp": 6000.0},
                      n, in_rate, 900 + c)
        dev.append(torch.from_numpy(x).cuda())
    torch.cuda.synchronize()
    k = len(dev)
    ptrs, cnts = [dev[c % k].data_ptr() for c in range(n_ch)], [n] * n_ch

    def bfm(stereo, rds):
        cfgs = [sa.BfmCfg(in_rate=in_rate, nco_freq=0, audio_rate=48000, rf_bandwidth=rf, af_bandwidth=af, volume=2.0, squelch_db=-60.0,
                          audio_stereo=stereo, lsb_stereo=0, show_pilot=0) for _ in range(n_ch)]
        return sa.BfmBank(cfgs, rds=[1] * n_ch) if rds else sa.BfmBank(cfgs)
    handles = {"stereo": bfm(1, 0), "stereo_rds": bfm(1, 1), "mono": bfm(0, 0)}
    for _ in range(2):
        for h in handles.values():
            h.feed_dev(ptrs, cnts)
    for h in handles.values():
        h.sync(); h.set_timing(True)
    times = {name: [] for name in handles}
    n_rds = 0
    for _ in range(feeds):
        for name, h in handles.items():
            h.feed_dev(ptrs, cnts)
            ms, cnt = h.get_timing(reset=True)
            assert cnt == 1
            times[name].append(ms)
        n_rds = handles["stereo_rds"].rds_state(0).n_rds
    med = {name: statistics.median(t) for name, t in times.items()}
    res = {"tool": "bfm_rate --rds", "channels": n_ch, "in_rate": in_rate, "samples_per_channel": n, "rds_samples_per_channel_and_feed": n_rds, "feeds": feeds}
    for name, t in times.items():
        res[f"{name}_ms_per_feed"] = round(med[name], 4)
        res[f"{name}_ms_series"] = [round(v, 4) for v in t]
    res["rds_share_ms"] = round(med["stereo_rds"] - med["stereo"], 4)
    res["rds_us_per_dependent_step"] = round((med["stereo_rds"] - med["stereo"]) * 1e3 / max(n_rds, 1), 5)
    res["walk_share_ms"] = round(med["stereo"] - med["mono"], 4)
    res["walk_us_per_dependent_step"] = round((med["stereo"] - med["mono"]) * 1e3 / n, 5)
    h = handles["stereo_rds"]
    res["bits_in_the_last_feed"] = int(h.rds_bits(0).size)
    res["groups_in_the_last_feed"] = int(h.rds_groups(0).shape[0])
    res["channels_synced"] = sum(int(h.rds_report(c)[4]) for c in range(n_ch))
    res["unsure_samples_all_channels"] = sum(h.rds_unsure(c) for c in range(n_ch))
    print(json.dumps(res))
    if args.out:
        with open(args.out, "a") as f:
            f.write("# tools/bfm_rate.py --rds: %d channels x 1 s at %d S/s, device resident, RDS off / RDS on / mono taking turns, median of %d feeds "
                    "after 2 warm-up rounds (HIP events around each feed's kernels)\n" % (n_ch, in_rate, feeds))
            for key, v in res.items():
                f.write(f"{key}: {v}\n")


if __name__ == "__main__":
    main()
