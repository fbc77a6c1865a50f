"""What CTCSS and the AF squelch add to a feed of the NFM demodulator bank (sdrx_nfm_create_ex), on device-resident samples.

256 channels x 1 s of channel-rate int16 I/Q at 60 kS/s -> 48 kS/s audio (tools/nfm_rate.py's shape; every carrier also carries
one of the 32 EIA tones, every fourth channel is a burst) sit in HBM; each feed is sdrx_nfm_feed_dev of the whole second.  Five
handles on the same streams: `plain` (sdrx_nfm_create), `off` (create_ex, every option off: the same launch sequence), `ctcss`
(CTCSS on in every channel, the channel's own tone selected in the even channels, its neighbour in the odd ones), `af` (the AF
squelch in every channel; squelch -300 is then the threshold 0.3) and `both`.
3 warm-up feeds each, then --feeds rounds (>= 10) in which the handles take turns: HIP events around each feed's kernels
(set_timing), median, minimum and maximum per handle.  Clocks are left alone.

    python tools/nfm_tone_rate.py [--out profiles/nfm_tone_rate.txt]                      one JSON line + a text report
    rocprofv3 --kernel-trace --stats -- python tools/nfm_tone_rate.py --only ctcss        per-kernel times (a run of its own)
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import sdrangel_amd as sa  # noqa: E402
from tests import nfm_tone_cases as tc  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=256)
    ap.add_argument("--in-rate", type=int, default=60000)
    ap.add_argument("--feeds", type=int, default=12)
    ap.add_argument("--only", default="", help="time one handle alone: plain, off, ctcss, af or both (profiling runs)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    n_ch, feeds, in_rate = args.channels, max(args.feeds, 10), args.in_rate
    n = in_rate                                              # one second
    rf, af, fmdev, vol, sq, gate, audio_rate = 12500.0, 3000.0, 2000, 2.0, -300.0, 5, 48000

    dev, cfgs, tones = [], [], []
    for c in range(n_ch):
        f0 = float(-6000 + (12000 * c) // max(n_ch, 1))
        t = c % 32
        sig = {"kind": "tone", "tones": [(n, tc.TONES[t])], "tdev": 400.0, "f0": f0, "dev": 2000.0, "fa": 300.0 + 7.0 * c, "amp": 6000.0, "noise": 10.0}
        if c % 4 == 0:
            sig.update(runs=[9000 + 10 * c, 2000, 14000, 7000, 4000, 3500], amps=[8000.0, 30.0])
        dev.append(torch.from_numpy(tc.signal(sig, n, in_rate, 900 + c)).cuda())
        cfgs.append(sa.NfmCfg(in_rate=in_rate, nco_freq=-int(f0), audio_rate=audio_rate, rf_bandwidth=rf, af_bandwidth=af, fm_deviation=fmdev,
                              volume=vol, squelch=sq, squelch_gate=gate, audio_mute=0))
        tones.append(sa.NfmToneCfg(ctcss_on=1, ctcss_index=1 + (t if c % 2 == 0 else (t + 1) % 32)))
    torch.cuda.synchronize()
    ptrs, cnts = [t.data_ptr() for t in dev], [n] * n_ch

    make = {"plain": lambda: sa.NfmDemodBank(cfgs), "off": lambda: sa.NfmDemodBank(cfgs, tone=[sa.NfmToneCfg()] * n_ch),
            "ctcss": lambda: sa.NfmDemodBank(cfgs, tone=tones),
            "af": lambda: sa.NfmDemodBank(cfgs, tone=[sa.NfmToneCfg(delta_squelch=1)] * n_ch),
            "both": lambda: sa.NfmDemodBank(cfgs, tone=[sa.NfmToneCfg(delta_squelch=1, ctcss_on=1, ctcss_index=t.ctcss_index) for t in tones])}
    names = [args.only] if args.only else list(make)
    banks = {k: make[k]() for k in names}
    for b in banks.values():
        for _ in range(3):
            b.feed_dev(ptrs, cnts)
        b.sync()
        b.set_timing(True)
    times = {k: [] for k in names}
    for _ in range(feeds):                                   # the handles take turns
        for k in names:
            banks[k].feed_dev(ptrs, cnts)
            ms, cnt = banks[k].get_timing(reset=True)
            assert cnt == 1
            times[k].append(ms)
    res = {"tool": "nfm_tone_rate", "channels": n_ch, "in_rate": in_rate, "audio_rate": audio_rate, "samples_per_channel": n, "feeds": feeds}
    for k in names:
        res[f"{k}_ms_per_feed"] = round(statistics.median(times[k]), 4)
        res[f"{k}_ms_min"] = round(min(times[k]), 4)
        res[f"{k}_ms_max"] = round(max(times[k]), 4)
    if "ctcss" in banks:
        b = banks["ctcss"]
        res["ctcss_channels_with_a_tone_detected"] = sum(b.ctcss(c)[0] > 0 for c in range(n_ch))
        res["ctcss_blocks_per_channel_max"] = max(b.ctcss_powers(c)[3] for c in range(n_ch))
        if "plain" in banks:
            res["ctcss_added_ms_per_feed"] = round(res["ctcss_ms_per_feed"] - res["plain_ms_per_feed"], 4)
    for k in ("af", "both"):
        if k in banks:
            res[f"{k}_channels_open"] = sum(banks[k].af_squelch(c)[0] for c in range(n_ch))
            if "plain" in banks:
                res[f"{k}_added_ms_per_feed"] = round(res[f"{k}_ms_per_feed"] - res["plain_ms_per_feed"], 4)
    if "off" in banks and "plain" in banks:
        res["off_minus_plain_ms_per_feed"] = round(res["off_ms_per_feed"] - res["plain_ms_per_feed"], 4)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write("# tools/nfm_tone_rate.py: %d channels x 1 s at %d S/s, device resident, median of %d feeds after 3 warm-up feeds, handles taking turns\n"
                    % (n_ch, in_rate, feeds))
            for k, v in res.items():
                f.write(f"{k}: {v}\n")


if __name__ == "__main__":
    main()
