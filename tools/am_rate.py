"""Rate of the AM demodulator bank (sdrx_am_*) on device-resident samples, next to the nearest composition of older handles.

256 channels x 1 s of channel-rate int16 I/Q at 60 kS/s (a tone-modulated carrier plus noise per channel, every fourth a
burst; half the channels with the Bandpass) sit in HBM; each feed is sdrx_am_feed_dev of the whole second.  3 warm-up feeds,
then --feeds timed ones (>= 10): HIP events around each feed's kernels (set_timing), median.  Clocks are left alone.

Yardstick, same process, same streams, alternating with the AM feeds: sdrx_backend_* (filt_mode 0, discri 0, the same
interpolator) feeding sdrx_audiotail_* kind = 0 on the device.  It runs the same front and a tail whose 301-tap Bandpass
sits in the serial lane.  Neither of those handles has an event timer, so the ratio compares like with like: both paths
under the same wall-clock bracket around a synchronised feed (device idle before, sync after).

    python tools/am_rate.py [--out profiles/r06_am_rate.txt]            one JSON line + a text report
    rocprofv3 --kernel-trace --stats -- python tools/am_rate.py --feeds 10 --no-baseline     per-kernel times (a run of its own)

--sync: synchronous AM (sdrx_am_create_ex).  256 channels x 1 s at 48 kS/s in and out (a carrier 20 Hz off centre with a tone in
either sideband), the squelch open from the first 2400 samples on: an envelope handle, a sync-DSB handle and a sync-USB handle on the
same streams, taking turns, HIP events around each feed's kernels.  The sync chain's only serial part is the loop walk, one wave per
channel: (sync - envelope) / open samples bounds the time of one dependent step from above (the parallel kernels of the chain are in
it).  Next to it, in the same run, the ChannelAnalyzer bank's walk measured the same way (pll on minus pll off, tools/chana_rate.py).

    python tools/am_rate.py --sync [--out profiles/am_sync_rate.txt]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import sdrangel_amd as sa  # noqa: E402
from tests import am_cases as ac  # noqa: E402


def sync_report(args):
    from tests import am_sync_cases as sc
    from tests import chana_pll_cases as pc
    from tests import synth
    n_ch, feeds, rate = args.channels, max(args.feeds, 10), 48000
    n = rate
    dev = []
    for c in range(n_ch):
        sig = {"kind": "am2", "f0": 20.0 + (c % 13), "fu": 400.0 + 5.0 * c, "fl": 650.0 + 3.0 * c, "amp": 5000.0, "noise": 10.0}
        dev.append(torch.from_numpy(sc.signal(sig, n, rate, 900 + c)).cuda())
    torch.cuda.synchronize()
    ptrs, cnts = [t.data_ptr() for t in dev], [n] * n_ch
    cfgs = [sa.AmCfg(in_rate=rate, nco_freq=0, audio_rate=rate, rf_bandwidth=5000.0, volume=0.25, squelch_db=-40.0, audio_mute=0, bandpass_enable=c % 2)
            for c in range(n_ch)]
    banks = {"envelope": sa.AmDemodBank(cfgs),
             "sync_dsb": sa.AmDemodBank(cfgs, sync=[sa.AmSyncCfg(pll=1, sync_op=0)] * n_ch),
             "sync_usb": sa.AmDemodBank(cfgs, sync=[sa.AmSyncCfg(pll=1, sync_op=1)] * n_ch)}
    # the ChannelAnalyzer walk, as tools/chana_rate.py --pll measures it
    cdev = [torch.from_numpy(synth.mix(n, 900 + c, 30, 8000, 1)).cuda() for c in range(n_ch)]
    torch.cuda.synchronize()
    cptrs = [t.data_ptr() for t in cdev]

    def chana(**kw):
        return sa.ChannelAnalyzerBank([sa.ChanaCfg(**{k: v for k, v in pc._cfg(rate, nco_freq=-2950 - (c % 97), **kw).items() if k != "psk_order"})
                                       for c in range(n_ch)], psk_order=[1] * n_ch)

    banks.update({"chana_pll_off": chana(), "chana_pll_on": chana(pll=1)})
    feed = lambda k, b: b.feed_dev(cptrs if k.startswith("chana") else ptrs, cnts)
    for _ in range(3):
        for k, b in banks.items():
            feed(k, b)
    times = {k: [] for k in banks}
    for b in banks.values():
        b.sync()
        b.set_timing(True)
    for _ in range(feeds):
        for k, b in banks.items():                           # taking turns
            feed(k, b)
            ms, cnt = b.get_timing(reset=True)
            assert cnt == 1
            times[k].append(ms)
    res = {"tool": "am_rate --sync", "channels": n_ch, "rate": rate, "samples_per_channel": n, "feeds": feeds}
    for k, t in times.items():
        res[f"{k}_ms_per_feed"] = round(statistics.median(t), 4)
        res[f"{k}_ms_min"] = round(min(t), 4)
        res[f"{k}_ms_max"] = round(max(t), 4)
    steps = n - rate // 20                                   # open samples of a steady feed: all but the first rate / 20
    res["open_samples_per_channel_and_feed"] = steps
    res["locked_channels_after_the_last_feed"] = {k: sum(int(banks[k].pll(c)[0]) for c in range(n_ch)) for k in ("sync_dsb", "sync_usb")}
    for k in ("sync_dsb", "sync_usb"):
        extra = res[f"{k}_ms_per_feed"] - res["envelope_ms_per_feed"]
        res[f"{k}_chain_ms"] = round(extra, 4)
        res[f"{k}_us_per_dependent_step_upper_bound"] = round(extra * 1e3 / steps, 4)
        res[f"{k}_realtime_channels_per_feed_second"] = round(n_ch * 1000.0 / res[f"{k}_ms_per_feed"], 1)
    csteps = banks["chana_pll_on"].last_dev(0)[1]
    res["chana_steps_per_channel_and_feed"] = csteps
    res["chana_walk_us_per_dependent_step"] = round((res["chana_pll_on_ms_per_feed"] - res["chana_pll_off_ms_per_feed"]) * 1e3 / max(csteps, 1), 4)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write("# tools/am_rate.py --sync: %d channels x 1 s at %d S/s, device resident, median of %d feeds after 3 warm-up feeds, handles taking turns\n" % (n_ch, rate, feeds))
            for k, v in res.items():
                f.write(f"{k}: {v}\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=256)
    ap.add_argument("--in-rate", type=int, default=60000)
    ap.add_argument("--feeds", type=int, default=12)
    ap.add_argument("--no-baseline", action="store_true", help="skip the composition yardstick (profiling runs)")
    ap.add_argument("--out", default="")
    ap.add_argument("--sync", action="store_true", help="synchronous AM next to envelope mode and the ChannelAnalyzer walk")
    args = ap.parse_args()
    if args.sync:
        return sync_report(args)
    n_ch, feeds, in_rate = args.channels, max(args.feeds, 10), args.in_rate
    n = in_rate                                              # one second
    rf, audio_rate = 5000.0, 48000

    dev, ncos = [], []
    for c in range(n_ch):
        f0 = float(-6000 + (12000 * c) // max(n_ch, 1))
        sig = {"kind": "am", "f0": f0, "depth": 0.5, "fa": 300.0 + 7.0 * c, "amp": 6000.0, "noise": 10.0}
        if c % 4 == 0:
            sig.update(runs=[9000 + 10 * c, 2000, 14000, 7000, 4000, 3500], amps=[8000.0, 30.0])
        dev.append(torch.from_numpy(ac.signal(sig, n, in_rate, 900 + c)).cuda())
        ncos.append(-int(f0))
    torch.cuda.synchronize()
    ptrs, cnts = [t.data_ptr() for t in dev], [n] * n_ch

    am = sa.AmDemodBank([sa.AmCfg(in_rate=in_rate, nco_freq=ncos[c], audio_rate=audio_rate, rf_bandwidth=rf, volume=2.0, squelch_db=-40.0,
                                  audio_mute=0, bandpass_enable=c % 2) for c in range(n_ch)])
    for _ in range(3):
        am.feed_dev(ptrs, cnts)
    am.sync()
    am.set_timing(True)
    t_am = []
    for _ in range(feeds):
        am.feed_dev(ptrs, cnts)
        ms, k = am.get_timing(reset=True)
        assert k == 1
        t_am.append(ms)
    audio = sum(am.last_dev(c)[1] for c in range(n_ch))
    am_ms = statistics.median(t_am)
    res = {"tool": "am_rate", "channels": n_ch, "in_rate": in_rate, "samples_per_channel": n, "feeds": feeds,
           "am_ms_per_feed": round(am_ms, 4), "am_ms_min": round(min(t_am), 4), "am_ms_max": round(max(t_am), 4),
           "channel_rate_ms_per_s": round(n_ch * n / am_ms / 1e3, 1), "audio_ks_per_s": round(audio / am_ms, 1),
           "audio_samples_per_feed": audio, "kernel": am.last_launch()}

    if not args.no_baseline:
        am.set_timing(False)
        be = sa.BackendBank([sa.BackendCfg(in_rate=in_rate, nco_freq=ncos[c], out_rate=audio_rate, interp_cutoff=float(np.float32(rf) / np.float32(2.2)),
                                           taps_per_phase=4.5, filt_mode=0, f1=0.0, f2=0.0, discri=0, fm_scaling=1.0) for c in range(n_ch)])
        tail = sa.AudioTail([sa.AudioTailCfg(kind=0, audio_rate=audio_rate, volume=2.0, fm_scaling=1.0, squelch_level=1e-4, squelch_gate=5,
                                             af_bandwidth=rf / 2.0) for _ in range(n_ch)])
        outs = [torch.zeros(n + 16, dtype=torch.int16, device="cuda") for _ in range(n_ch)]
        torch.cuda.synchronize()
        po = (C.c_void_p * n_ch)(*[t.data_ptr() for t in outs])

        def composition():
            be.feed_dev(ptrs, cnts)
            views = [be.last_dev(c) for c in range(n_ch)]    # the counts come back to the host here, as a caller of both handles needs them
            pi = (C.c_void_p * n_ch)(*[v[0] for v in views])
            ns = (C.c_int64 * n_ch)(*[v[1] // 2 for v in views])
            rc = sa.lib().sdrx_audiotail_feed_dev(tail._h, pi, ns, po)
            assert rc == 0, sa.lib().sdrx_last_error().decode()
            assert sa.lib().sdrx_audiotail_sync(tail._h) == 0

        def am_feed():
            am.feed_dev(ptrs, cnts)
            am.sync()

        for _ in range(3):
            composition()
        t_comp, t_wall = [], []
        for _ in range(feeds):                               # alternating, each under the same bracket
            for fn, acc in ((composition, t_comp), (am_feed, t_wall)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                acc.append((time.perf_counter() - t0) * 1e3)
        comp_ms, wall_ms = statistics.median(t_comp), statistics.median(t_wall)
        res.update({"composition_wall_ms_per_feed": round(comp_ms, 4), "composition_wall_ms_min": round(min(t_comp), 4),
                    "composition_wall_ms_max": round(max(t_comp), 4), "am_wall_ms_per_feed": round(wall_ms, 4),
                    "am_wall_ms_min": round(min(t_wall), 4), "am_wall_ms_max": round(max(t_wall), 4),
                    "ratio_am_over_composition_wall": round(wall_ms / comp_ms, 4)})

    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write("# tools/am_rate.py: %d channels x 1 s at %d S/s, device resident, median of %d feeds after 3 warm-up feeds\n" % (n_ch, in_rate, feeds))
            for k, v in res.items():
                f.write(f"{k}: {v}\n")


if __name__ == "__main__":
    main()
