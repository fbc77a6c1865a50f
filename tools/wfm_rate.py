"""Rate of the wideband-FM demodulator bank (sdrx_wfm_*) on device-resident samples, next to its yardstick.

32 channels x 1 s of channel-rate int16 I/Q (an FM-modulated tone plus noise per channel, 120 kS/s by default: the channel
bank's output rate for WFMDemod::requiredBW(80000) on a 61.44 MS/s stream) sit in HBM; each feed is sdrx_wfm_feed_dev of
the whole second.  3 warm-up feeds, then --feeds timed ones (>= 10): HIP events around each feed's kernels (set_timing),
median.  Clocks are left alone.

Yardstick, same process, same streams: sdrx_backend_* with filt_mode = 1 (runFilt), discri = 1, out_rate = in_rate and the
same f1 / f2.  It runs the same number of 1024-point filter blocks, plus a 72-tap complex FIR at the full channel rate and a
separate mix pass, so it does strictly more arithmetic and traffic.  The back-end has no event timer, so the ratio compares
like with like: both handles under the same wall-clock bracket around a synchronised feed (device idle before, sync after).

Also prints the single-thread rate of the CPU restatement (tests/wfm_oracle.c) on this box: a baseline, not a target.

    python tools/wfm_rate.py [--out profiles/r06_wfm_rate.txt]            one JSON line + a text report
    rocprofv3 --kernel-trace --stats -- python tools/wfm_rate.py --feeds 10 --no-baseline     per-kernel times (a run of its own)
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
from tests import wfm_cases as wc  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=32)
    ap.add_argument("--in-rate", type=int, default=0, help="channel rate; 0: the bank's output rate for requiredBW(80000) at 61.44 MS/s")
    ap.add_argument("--feeds", type=int, default=12)
    ap.add_argument("--no-baseline", action="store_true", help="skip the back-end yardstick and the CPU oracle (profiling runs)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    n_ch, feeds = args.channels, max(args.feeds, 10)
    in_rate = args.in_rate or sa.chan_plan(61_440_000, sa.wfm_required_bw(80000), 0)[1]
    n = in_rate                                              # one second
    rf, af = 80000.0, 15000.0

    host, dev = [], []
    for c in range(n_ch):
        f0 = -20000.0 + 1300.0 * c
        x = wc.signal({"kind": "fm", "f0": f0, "dev": 50000.0, "fa": 400.0 + 100.0 * c, "amp": 6000.0}, n, in_rate, 900 + c)
        host.append(x); dev.append(torch.from_numpy(x).cuda())
    torch.cuda.synchronize()
    ptrs, cnts = [t.data_ptr() for t in dev], [n] * n_ch
    ncos = [-int(-20000.0 + 1300.0 * c) for c in range(n_ch)]

    wfm = sa.WfmDemodBank([sa.WfmCfg(in_rate=in_rate, nco_freq=ncos[c], audio_rate=48000, rf_bandwidth=rf, af_bandwidth=af, volume=2.0,
                                     squelch_db=-60.0, audio_mute=0) for c in range(n_ch)])
    for _ in range(3):
        wfm.feed_dev(ptrs, cnts)
    wfm.sync()
    wfm.set_timing(True)
    t_wfm = []
    for _ in range(feeds):
        wfm.feed_dev(ptrs, cnts)
        ms, k = wfm.get_timing(reset=True)
        assert k == 1
        t_wfm.append(ms)
    audio = sum(wfm.last_dev(c)[1] for c in range(n_ch))
    wfm_ms = statistics.median(t_wfm)
    res = {"tool": "wfm_rate", "channels": n_ch, "in_rate": in_rate, "samples_per_channel": n, "feeds": feeds,
           "wfm_ms_per_feed": round(wfm_ms, 4), "wfm_ms_min": round(min(t_wfm), 4), "wfm_ms_max": round(max(t_wfm), 4),
           "channel_rate_ms_per_s": round(n_ch * n / wfm_ms / 1e3, 1), "audio_ks_per_s": round(audio / wfm_ms, 1),
           "audio_samples_per_feed": audio, "kernel": wfm.last_launch()}

    if not args.no_baseline:
        f1 = float(np.float32(-(rf / 2.0) / in_rate)); f2 = float(np.float32((rf / 2.0) / in_rate))
        be = sa.BackendBank([sa.BackendCfg(in_rate=in_rate, nco_freq=ncos[c], out_rate=in_rate, interp_cutoff=af, taps_per_phase=4.5,
                                           filt_mode=1, f1=f1, f2=f2, discri=1, fm_scaling=in_rate / rf) for c in range(n_ch)])
        for _ in range(3):
            be.feed_dev(ptrs, cnts)
        be.sync()
        t_be = []
        for _ in range(feeds):
            # the back-end has no event timer and runs on its own non-blocking stream: wall time around a synchronised feed
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            be.feed_dev(ptrs, cnts)
            be.sync()
            t_be.append((time.perf_counter() - t0) * 1e3)
        be_ms = statistics.median(t_be)
        # the same wall-clock bracket on the WFM handle, so that the ratio compares like with like
        wfm.set_timing(False)
        t_wfm_wall = []
        for _ in range(feeds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            wfm.feed_dev(ptrs, cnts)
            wfm.sync()
            t_wfm_wall.append((time.perf_counter() - t0) * 1e3)
        wfm_wall = statistics.median(t_wfm_wall)
        res.update({"backend_wall_ms_per_feed": round(be_ms, 4), "wfm_wall_ms_per_feed": round(wfm_wall, 4),
                    "ratio_wfm_over_backend_wall": round(wfm_wall / be_ms, 4)})
        # CPU restatement, one thread, one channel's second
        L = wc.build_oracle()
        o = wc.OracleWfm(L, (in_rate, ncos[0], 48000, rf, af, 2.0, -60.0, 0))
        t0 = time.perf_counter()
        o.feed(host[0])
        dt = time.perf_counter() - t0
        res["oracle_cpu_single_thread_ms_per_s"] = round(n / dt / 1e6, 3)

    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write("# tools/wfm_rate.py: %d channels x 1 s at %d S/s, device resident, median of %d feeds after 3 warm-up feeds\n" % (n_ch, in_rate, feeds))
            for k, v in res.items():
                f.write(f"{k}: {v}\n")


if __name__ == "__main__":
    main()
