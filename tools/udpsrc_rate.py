"""Rate of the UDPSrc bank (sdrx_udpsrc_*) on device-resident samples, per sample format, next to the NFM demodulator bank on
the same streams.

256 channels x 1 s of channel-rate int16 I/Q at 48 kS/s (a tone-modulated carrier plus noise per channel, every fourth a burst)
sit in HBM; each feed is sdrx_udpsrc_feed_dev of the whole second at 48000 -> 48000 (step 1).  One handle per format (the AM formats
also with MagAGC on: format8agc ...), all channels of a handle in that format.  3 warm-up feeds each, then --feeds timed ones (>= 10), interleaved round robin over the
formats and the NFM bank so that all see the same clocks: HIP events around each feed's kernels (set_timing), median.  Clocks are
left alone.

Yardstick: sdrx_nfm_* at 48000 -> 48000 on the same streams.  Format 0 does a subset of its work (the same front, one serial
prefix sum, no Bandpass), so its median should not exceed the NFM bank's by more than 10 %; the report states the ratio.
The CPU figure is tests/udpsrc_oracle.c on one core for one channel's second, times the channel count.

    python tools/udpsrc_rate.py [--out profiles/r11_udpsrc_rate.txt]          one JSON line + a text report
    rocprofv3 --kernel-trace --stats -- python tools/udpsrc_rate.py --feeds 10 --no-baseline     per-kernel times (a run of its own)
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import sdrangel_amd as sa  # noqa: E402
from tests import udpsrc_cases as uc  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=256)
    ap.add_argument("--in-rate", type=int, default=48000)
    ap.add_argument("--feeds", type=int, default=12)
    ap.add_argument("--formats", default="0,1,2,3,8,9,10,8a,9a,10a", help="sample formats; a trailing a: m_agc on (the SSB formats: 4,5,6,7,4a,6a)")
    ap.add_argument("--no-baseline", action="store_true", help="skip the NFM bank and the CPU oracle (profiling runs)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    n_ch, feeds, in_rate = args.channels, max(args.feeds, 10), args.in_rate
    formats = [(int(v.rstrip("a")), int(v.endswith("a"))) for v in args.formats.split(",")]
    label = lambda fmt, agc: f"format{fmt}" + ("agc" if agc else "")
    n = in_rate                                              # one second
    rf, fmdev, gain, sqdb, gate = 12500.0, 2500, 1.0, -60, 5

    dev, ncos, sigs = [], [], []
    for c in range(n_ch):
        f0 = float(-6000 + (12000 * c) // max(n_ch, 1))
        sig = {"kind": "nfm", "f0": f0, "dev": 2000.0, "fa": 300.0 + 7.0 * c, "amp": 6000.0, "noise": 10.0}
        if c % 4 == 0:
            sig.update(runs=[9000 + 10 * c, 2000, 14000, 7000, 4000, 3500], amps=[8000.0, 3.0])
        sigs.append(sig)
        dev.append(torch.from_numpy(uc.signal(sig, n, in_rate, 900 + c)).cuda())
        ncos.append(-int(f0))
    torch.cuda.synchronize()
    ptrs, cnts = [t.data_ptr() for t in dev], [n] * n_ch

    banks = {}
    for fmt, agc in formats:
        banks[label(fmt, agc)] = sa.UdpSrcBank([sa.UdpSrcCfg(in_rate=in_rate, nco_freq=ncos[c], output_sample_rate=float(in_rate), sample_format=fmt,
                                                            rf_bandwidth=rf, fm_deviation=fmdev, gain=gain, squelch_db=sqdb, squelch_gate=gate,
                                                            squelch_enabled=1, agc=agc) for c in range(n_ch)])
    if not args.no_baseline:
        banks["nfm"] = sa.NfmDemodBank([sa.NfmCfg(in_rate=in_rate, nco_freq=ncos[c], audio_rate=in_rate, rf_bandwidth=rf, af_bandwidth=3000.0,
                                                  fm_deviation=2000, volume=2.0, squelch=-300.0, squelch_gate=gate, audio_mute=0) for c in range(n_ch)])
    for b in banks.values():
        for _ in range(3):
            b.feed_dev(ptrs, cnts)
        b.sync()
        b.set_timing(True)
    times = {k: [] for k in banks}
    for _ in range(feeds):                                   # interleaved: every handle once per round
        for k, b in banks.items():
            b.feed_dev(ptrs, cnts)
            ms, cnt = b.get_timing(reset=True)
            assert cnt == 1
            times[k].append(ms)
    res = {"tool": "udpsrc_rate", "channels": n_ch, "in_rate": in_rate, "output_sample_rate": in_rate, "samples_per_channel": n, "feeds": feeds}
    for k, t in times.items():
        med = statistics.median(t)
        res[f"{k}_ms_per_feed"] = round(med, 4)
        res[f"{k}_ms_min"] = round(min(t), 4)
        res[f"{k}_ms_max"] = round(max(t), 4)
        res[f"{k}_channel_rate_ms_per_s"] = round(n_ch * n / med / 1e3, 1)
    for k, b in banks.items():
        if k != "nfm":
            res[f"{k}_samples_per_feed"] = sum(b.last_dev(c)[1] for c in range(n_ch))
            res[f"{k}_channels_open"] = sum(int(b.squelch_open(c)) for c in range(n_ch))
    if "format0" in banks:
        res["kernel"] = banks["format0"].last_launch()
    if "nfm" in times and "format0" in times:
        res["ratio_format0_over_nfm"] = round(statistics.median(times["format0"]) / statistics.median(times["nfm"]), 4)
    if not args.no_baseline:
        L = uc.build_oracle()
        x = uc.signal(sigs[1], n, in_rate, 901)
        for fmt, agc in formats:
            cfg = (in_rate, ncos[1], float(in_rate), fmt, rf, fmdev, gain, sqdb, gate, 1, agc)
            if 4 <= fmt <= 7:                               # the SSB formats have an oracle of their own
                from tests import udpsrc_ssb_cases as sc
                o = sc.OracleSsb(sc.build_oracle(), cfg)
            else:
                o = uc.OracleUdp(L, cfg)
            t0 = time.perf_counter()
            o.feed(x)
            res[f"{label(fmt, agc)}_cpu_oracle_ms_all_channels_one_core"] = round((time.perf_counter() - t0) * 1e3 * n_ch, 1)
            o.close()

    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write("# tools/udpsrc_rate.py: %d channels x 1 s at %d S/s -> %d S/s, device resident, median of %d interleaved feeds after 3 warm-up feeds\n"
                    % (n_ch, in_rate, in_rate, feeds))
            for k, v in res.items():
                f.write(f"{k}: {v}\n")


if __name__ == "__main__":
    main()
