"""Rate of the SSB demodulator bank (sdrx_ssb_*) on device-resident samples, next to the composition of older handles that
computes the same audio.

256 channels x 1 s of channel-rate int16 I/Q at 60 kS/s (a tone in the upper sideband plus noise per channel, every fourth in
bursts that take the AGC down and up again) sit in HBM; each feed is sdrx_ssb_feed_dev of the whole second.  3 warm-up feeds,
then --feeds timed ones (>= 12): HIP events around each feed's kernels (set_timing), median.  Clocks are left alone.

Yardstick, same process, same streams, alternating with the SSB feeds: sdrx_backend_* (filt_mode 2, the same interpolator and
filter) feeding sdrx_audiotail_* kind = 1 on the device with the same derived parameters -- bit for bit the same mono audio
(tests/test_ssb_gpu.py), from a tail that walks one lane per channel through MagAGC::feedAndGetValue.  Neither of those handles
has an event timer, so the ratio compares like with like: both paths under the same wall-clock bracket around a synchronised
feed (device idle before, sync after).  The two outputs are compared once after the timed feeds, from fresh state.

    python tools/ssb_rate.py [--out profiles/r10_ssb_rate.txt]          one JSON line + a text report
    rocprofv3 --kernel-trace --stats -- python tools/ssb_rate.py --feeds 12 --no-baseline     per-kernel times (a run of its own)
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
from tests import ssb_cases as sc  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=256)
    ap.add_argument("--in-rate", type=int, default=60000)
    ap.add_argument("--feeds", type=int, default=12)
    ap.add_argument("--no-baseline", action="store_true", help="skip the composition yardstick (profiling runs)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    n_ch, feeds, in_rate = args.channels, max(args.feeds, 12), args.in_rate
    n = in_rate                                              # one second
    audio_rate = 48000
    base = sc._cfg(in_rate, audio_rate, agc=1)               # the settings' defaults with the AGC on: hn 6144, gate 192

    dev, cfgs = [], []
    for c in range(n_ch):
        f0 = float(-6000 + (12000 * c) // max(n_ch, 1))
        sig = {"kind": "tone", "f0": f0 + 500.0 + 7.0 * c, "amp": 6000.0, "noise": 10.0}
        if c % 4 == 0:
            sig.update(runs=[9000 + 10 * c, 14000, 100, 3000, 4000, 3500], amps=[8000.0, 30.0])
        dev.append(torch.from_numpy(sc.signal(sig, n, in_rate, 900 + c)).cuda())
        cfgs.append(dict(base, nco_freq=-int(f0)))
    torch.cuda.synchronize()
    ptrs, cnts = [t.data_ptr() for t in dev], [n] * n_ch

    ssb = sa.SsbDemodBank([sa.SsbCfg(**k) for k in cfgs])
    for _ in range(3):
        ssb.feed_dev(ptrs, cnts)
    ssb.sync()
    ssb.set_timing(True)
    t_ev = []
    for _ in range(feeds):
        ssb.feed_dev(ptrs, cnts)
        ms, k = ssb.get_timing(reset=True)
        assert k == 1
        t_ev.append(ms)
    audio = sum(ssb.last_dev(c)[1] for c in range(n_ch))
    ev_ms = statistics.median(t_ev)
    res = {"tool": "ssb_rate", "channels": n_ch, "in_rate": in_rate, "samples_per_channel": n, "feeds": feeds,
           "ssb_ms_per_feed": round(ev_ms, 4), "ssb_ms_min": round(min(t_ev), 4), "ssb_ms_max": round(max(t_ev), 4),
           "channel_rate_ms_per_s": round(n_ch * n / ev_ms / 1e3, 1), "audio_ks_per_s": round(audio / ev_ms, 1),
           "audio_samples_per_feed": audio, "kernel": ssb.last_launch()}

    if not args.no_baseline:
        ssb.set_timing(False)
        rate, band, low = np.float32(audio_rate), np.float32(base["rf_bandwidth"]), np.float32(base["low_cutoff"])
        be = sa.BackendBank([sa.BackendCfg(in_rate=in_rate, nco_freq=k["nco_freq"], out_rate=audio_rate, interp_cutoff=float(band * np.float32(1.5)),
                                           taps_per_phase=2.0, filt_mode=2, f1=float(low / rate), f2=float(band / rate), discri=0, fm_scaling=1.0)
                             for k in cfgs])
        tail = sa.AudioTail([sa.AudioTailCfg(kind=1, audio_rate=audio_rate, volume=float(np.float32(base["volume"] / 4.0)), agc_active=1,
                                             agc_nb_samples=sc.hn_of(base), agc_threshold_enable=1, agc_gate=sc.gate_of(base), agc_clamping=0,
                                             agc_threshold=10.0 ** (base["agc_power_threshold"] / 10.0) * (32768.0 * 32768.0)) for _ in range(n_ch)])
        outs = [torch.zeros(n + 1040, dtype=torch.int16, device="cuda") for _ in range(n_ch)]
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

        def ssb_feed():
            ssb.feed_dev(ptrs, cnts)
            ssb.sync()

        for _ in range(3):
            composition()
        t_comp, t_wall = [], []
        for _ in range(feeds):                               # alternating, each under the same bracket
            for fn, acc in ((composition, t_comp), (ssb_feed, t_wall)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                acc.append((time.perf_counter() - t0) * 1e3)
        comp_ms, wall_ms = statistics.median(t_comp), statistics.median(t_wall)
        # the two paths have been fed different numbers of seconds by now: from fresh state, one feed each, then compare
        ssb.reset()
        assert sa.lib().sdrx_audiotail_reset(tail._h) == 0
        be = sa.BackendBank(be.cfgs)                         # the back-end has no reset of its own
        composition()
        ssb_feed()
        same, loud = 0, 0
        for c in range(n_ch):
            k = ssb.last_dev(c)[1]
            got, want = ssb.read(c), outs[c][:k].cpu().numpy()
            same += int(np.array_equal(got[:, 0], want) and np.array_equal(got[:, 1], want))
            loud += int(got.any())
        res["channels_equal_to_composition"] = same
        res["channels_with_audio"] = loud
        res.update({"composition_wall_ms_per_feed": round(comp_ms, 4), "composition_wall_ms_min": round(min(t_comp), 4),
                    "composition_wall_ms_max": round(max(t_comp), 4), "ssb_wall_ms_per_feed": round(wall_ms, 4),
                    "ssb_wall_ms_min": round(min(t_wall), 4), "ssb_wall_ms_max": round(max(t_wall), 4),
                    "ratio_ssb_over_composition_wall": round(wall_ms / comp_ms, 4),
                    "ssb_range_wholly_below_composition": bool(max(t_wall) < min(t_comp))})

    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write("# tools/ssb_rate.py: %d channels x 1 s at %d S/s, device resident, median of %d feeds after 3 warm-up feeds\n" % (n_ch, in_rate, feeds))
            for k, v in res.items():
                f.write(f"{k}: {v}\n")


if __name__ == "__main__":
    main()
