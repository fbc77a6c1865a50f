"""Rate of the spectrum sink (sdrx_spectrum_*) on device-resident samples: one JSON line.

For N in {1024, 4096}, without averaging and with a moving average (depth 8), 256 Mi samples already in HBM are fed with
sdrx_spectrum_feed_dev; HIP events around each feed's kernels give the kernel time (best of --reps).  Bytes per sample:
4 in + 4 * N * frames / samples out (the queued frames); the moving average also writes and reads the raw powers and its
depth x N state, which is not counted.  Roofline fraction: those bytes over the time, against 8 TB/s."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import sdrangel_amd as sa  # noqa: E402

HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=256 << 20)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    n = args.samples
    g = torch.Generator(device="cuda:0").manual_seed(1)
    iq = torch.randint(-32768, 32768, (2 * n,), dtype=torch.int32, device="cuda:0", generator=g).to(torch.int16)
    torch.cuda.synchronize()
    res = []
    for n_fft in (1024, 4096):
        for avg in ("none", "moving"):
            cfg = (n_fft, 0, 8 if avg == "moving" else 0, sa.AVG_MOVING if avg == "moving" else sa.AVG_NONE, sa.WIN_BLACKMAN_HARRIS, False)
            s = sa.SpectrumVis(*cfg)
            s.feed_dev(iq); s.sync(); s.skip()              # warm-up: code objects, queue and scratch buffers
            s.set_timing(True)
            best = None
            for _ in range(args.reps):
                s.feed_dev(iq)
                ms, feeds = s.get_timing(reset=True)
                frames = s.skip()
                best = ms if best is None else min(best, ms)
            bps = 4 + 4 * n_fft * frames / n
            res.append({"fft_size": n_fft, "avg": avg, "samples": n, "frames": frames, "kernel_ms": round(best, 3),
                        "ms_per_s": round(n / best / 1e3, 1), "gs_per_s": round(n / best / 1e6, 2),
                        "bytes_per_sample": round(bps, 3), "hbm_fraction": round(n * bps / (best * 1e-3) / HBM_PEAK, 4),
                        "kernel": s.last_launch()["kernel"]})
            s.close()
    print(json.dumps({"tool": "spectrum_rate", "results": res}))


if __name__ == "__main__":
    main()
