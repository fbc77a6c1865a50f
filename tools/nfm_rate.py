"""Rate of the NFM demodulator bank (sdrx_nfm_*) on device-resident samples, next to the composition of older handles that
computes the same audio.

256 channels x 1 s of channel-rate int16 I/Q at 60 kS/s (a tone-modulated FM carrier plus noise per channel, every fourth a
burst) sit in HBM; each feed is sdrx_nfm_feed_dev of the whole second.  3 warm-up feeds, then --feeds timed ones (>= 10): HIP
events around each feed's kernels (set_timing), median.  Clocks are left alone.

Yardstick, same process, same streams, alternating with the NFM feeds: sdrx_backend_* (filt_mode 0, discri 0, the same
interpolator) feeding sdrx_audiotail_* kind = 0 on the device with the same derived parameters -- bit for bit the same audio
(tests/test_nfm_gpu.py), from a tail that walks one lane per channel with the 301-tap Bandpass inside the serial lane.  Neither
of those handles has an event timer, so the ratio compares like with like: both paths under the same wall-clock bracket around
a synchronised feed (device idle before, sync after).  The two outputs are compared once after the timed feeds.

    python tools/nfm_rate.py [--out profiles/r09_nfm_rate.txt]          one JSON line + a text report
    rocprofv3 --kernel-trace --stats -- python tools/nfm_rate.py --feeds 10 --no-baseline     per-kernel times (a run of its own)
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
from tests import nfm_cases as nc  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=256)
    ap.add_argument("--in-rate", type=int, default=60000)
    ap.add_argument("--feeds", type=int, default=12)
    ap.add_argument("--no-baseline", action="store_true", help="skip the composition yardstick (profiling runs)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    n_ch, feeds, in_rate = args.channels, max(args.feeds, 10), args.in_rate
    n = in_rate                                              # one second
    rf, af, fmdev, vol, sq, gate, audio_rate = 12500.0, 3000.0, 2000, 2.0, -300.0, 5, 48000

    dev, ncos = [], []
    for c in range(n_ch):
        f0 = float(-6000 + (12000 * c) // max(n_ch, 1))
        sig = {"kind": "nfm", "f0": f0, "dev": 2000.0, "fa": 300.0 + 7.0 * c, "amp": 6000.0, "noise": 10.0}
        if c % 4 == 0:
            sig.update(runs=[9000 + 10 * c, 2000, 14000, 7000, 4000, 3500], amps=[8000.0, 30.0])
        dev.append(torch.from_numpy(nc.signal(sig, n, in_rate, 900 + c)).cuda())
        ncos.append(-int(f0))
    torch.cuda.synchronize()
    ptrs, cnts = [t.data_ptr() for t in dev], [n] * n_ch

    am = sa.NfmDemodBank([sa.NfmCfg(in_rate=in_rate, nco_freq=ncos[c], audio_rate=audio_rate, rf_bandwidth=rf, af_bandwidth=af, fm_deviation=fmdev,
                                    volume=vol, squelch=sq, squelch_gate=gate, audio_mute=0) for c in range(n_ch)])
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
    res = {"tool": "nfm_rate", "channels": n_ch, "in_rate": in_rate, "samples_per_channel": n, "feeds": feeds,
           "nfm_ms_per_feed": round(am_ms, 4), "nfm_ms_min": round(min(t_am), 4), "nfm_ms_max": round(max(t_am), 4),
           "channel_rate_ms_per_s": round(n_ch * n / am_ms / 1e3, 1), "audio_ks_per_s": round(audio / am_ms, 1),
           "audio_samples_per_feed": audio, "kernel": am.last_launch()}

    if not args.no_baseline:
        am.set_timing(False)
        be = sa.BackendBank([sa.BackendCfg(in_rate=in_rate, nco_freq=ncos[c], out_rate=audio_rate, interp_cutoff=float(np.float32(rf) / np.float32(2.2)),
                                           taps_per_phase=4.5, filt_mode=0, f1=0.0, f2=0.0, discri=0, fm_scaling=1.0) for c in range(n_ch)])
        tail = sa.AudioTail([sa.AudioTailCfg(kind=0, audio_rate=audio_rate, volume=vol, fm_scaling=float(np.float32(8.0) * np.float32(audio_rate) / np.float32(fmdev)),
                                             squelch_level=float(np.float32(10.0 ** (sq / 100.0))), squelch_gate=(audio_rate // 100) * gate,
                                             af_bandwidth=af) for _ in range(n_ch)])
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
        # the two paths have been fed different numbers of seconds by now: from fresh state, one feed each, then compare
        am.reset()
        assert sa.lib().sdrx_audiotail_reset(tail._h) == 0
        be = sa.BackendBank(be.cfgs)                         # the back-end has no reset of its own
        composition()
        am_feed()
        same = 0
        for c in range(n_ch):
            k = am.last_dev(c)[1]
            same += int(np.array_equal(am.read(c), outs[c][:k].cpu().numpy()))
        res["channels_equal_to_composition"] = same
        res.update({"composition_wall_ms_per_feed": round(comp_ms, 4), "composition_wall_ms_min": round(min(t_comp), 4),
                    "composition_wall_ms_max": round(max(t_comp), 4), "nfm_wall_ms_per_feed": round(wall_ms, 4),
                    "nfm_wall_ms_min": round(min(t_wall), 4), "nfm_wall_ms_max": round(max(t_wall), 4),
                    "ratio_nfm_over_composition_wall": round(wall_ms / comp_ms, 4)})

    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write("# tools/nfm_rate.py: %d channels x 1 s at %d S/s, device resident, median of %d feeds after 3 warm-up feeds\n" % (n_ch, in_rate, feeds))
            for k, v in res.items():
                f.write(f"{k}: {v}\n")


if __name__ == "__main__":
    main()
