#!/usr/bin/env python3
"""Channel analyzers behind a recording with the pieces of libsdrx.so, shaped like an SDRangel FileSource device set with
ChannelAnalyzer channels:

    .sdriq file (FileRecord header + int16 I/Q)  ->  SampleSinkFifo  ->  engine drain loop
        ->  DownChannelizer bank, one channel per slice of the band, requested rate 48000
        ->  (device hand-over, no host round trip)  ChannelAnalyzer bank: NCOF -> optional Interpolator -> fftfilt (SSB, DSB or
            root raised cosine) -> span decimation -> the Samples the analyzer's scope and spectrum see, or their autocorrelation
        ->  one .npy file of Samples (re, im) per slice

    python examples/filesource_to_chanalyzer.py [out_dir] [--pll]   # writes a synthetic recording, replays it, saves the Samples

The slices are an upper-sideband view, a lower-sideband view, a root-raised-cosine view behind the Interpolator and the
autocorrelation of a slice.  With --pll the first slice becomes a DSB view with the PLL on (its tone is followed and mixed down to
0 Hz; the lock state is printed) and the third a view of the FLL's own oscillator (input type 1).  Everything numeric runs on the MI355X through the C ABI (include/sdrx.h); this script is host glue
only."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sdrangel_amd as sa  # noqa: E402

FS = 2_400_000
CENTRES = [-825_000, -200_000, 312_500, 900_000]            # slice centres, offsets from the recording's centre
TONES = [700.0, -1100.0, 1500.0, 900.0]                     # one tone inside each slice
REQ_RATE = 48000
#: per slice: what differs from the defaults below
KINDS = [dict(ssb=1), dict(ssb=1, bandwidth=-5000, low_cutoff=-300), dict(rrc=1, down_sample=1, down_sample_rate=24000, span_log2=1),
         dict(input_type=2)]
COMMON = dict(down_sample=0, down_sample_rate=0, bandwidth=5000, low_cutoff=300, span_log2=0, ssb=0, rrc=0, rrc_rolloff=35, input_type=0,
              pll=0, fll=0)


def synth_recording(path, seconds=0.4):
    """one tone inside each slice, plus noise, as a .sdriq file"""
    n = int(FS * seconds)
    t = np.arange(n) / FS
    x = np.zeros(n, np.complex128)
    for fc, tone in zip(CENTRES, TONES):
        x += 420.0 * np.exp(2j * np.pi * (fc + tone) * t)
    rng = np.random.default_rng(3)
    x += rng.normal(0, 20, n) + 1j * rng.normal(0, 20, n)
    iq = np.empty(2 * n, np.int16)
    iq[0::2] = np.clip(np.round(x.real), -2048, 2047); iq[1::2] = np.clip(np.round(x.imag), -2048, 2047)
    with open(path, "wb") as f:
        f.write(sa.sdriq_header_bytes(FS, 14_200_000, 1_700_000_000, 16))
        f.write(iq.tobytes())
    return n


#: --pll: what the first and the third slice become
PLL_KINDS = {0: dict(pll=1), 2: dict(pll=1, fll=1, input_type=1)}


def channel_settings(c, out_rate, ofs, pll=False):
    """the sdrx_chana_cfg fields of slice c behind a channelizer that delivers out_rate with the slice's centre at ofs"""
    d = dict(COMMON); d.update(PLL_KINDS[c] if pll and c in PLL_KINDS else KINDS[c])
    d.update(in_rate=out_rate, nco_freq=-ofs)
    if pll and c == 0:
        d["nco_freq"] -= int(TONES[0]) - 10                 # the slice's tone 10 Hz above the loop's centre
    return d


def main(out_dir, pll=False):
    os.makedirs(out_dir, exist_ok=True)
    rec = os.path.join(out_dir, "synthetic_chanalyzer.sdriq")
    n = synth_recording(rec)

    hdr, payload = sa.sdriq_parse(open(rec, "rb").read())   # FileRecord::readHeader + the samples behind it
    assert hdr.sample_rate == FS and hdr.sample_size == 16

    fifo = sa.SampleSinkFifo(FS // 4)
    bank = sa.ChannelizerBank(FS, [REQ_RATE] * len(CENTRES), CENTRES)
    ana = sa.ChannelAnalyzerBank([sa.ChanaCfg(**channel_settings(c, *bank.info(c)[1:], pll=pll)) for c in range(len(CENTRES))])

    samples = [[] for _ in CENTRES]
    spans = []
    block = 2 * 100_000                                     # int16 per "FileSourceThread tick"
    for pos in range(0, payload.size, block):
        fifo.write(payload[pos: pos + block])
        while fifo.fill:                                    # DSPDeviceSourceEngine::work: drain, feed the sinks
            span = fifo.read(fifo.fill)
            spans.append(span.size // 2)
            bank.feed(span)
            ana.feed_bank(bank)                             # ordered on the device against the bank's stream
            for c in range(len(CENTRES)):
                bank.skip(c)
                samples[c].append(ana.read(c))              # many feeds hand out nothing: the filter works in blocks of 512 / 1024
    paths = []
    for c, fc in enumerate(CENTRES):
        s = np.concatenate(samples[c])                      # [n, 2]: re, im
        p = os.path.join(out_dir, f"chanalyzer_ch{c}.npy")
        np.save(p, s)
        paths.append(p)
        what = "autocorrelation" if KINDS[c].get("input_type") == 2 else "signal"
        print(f"slice {c}: {fc:+8d} Hz  {s.shape[0]} Samples ({what}, positive only: {ana.positive_only(c)}), magsq {ana.magsq(c):.3e}, "
              f"peak |re| {int(np.abs(s[:, 0].astype(np.int32)).max()) if s.size else 0} -> {p}")
    if pll:
        locked, freq, dphi, phi = ana.pll_state(0)
        print(f"slice 0: PLL locked {locked}, frequency {float(freq) * bank.info(0)[1] / (2 * np.pi):+.1f} Hz, delta phi {float(dphi):+.4f}, phase {float(phi):+.4f}")
    print(f"{n} input samples replayed from {rec}")
    return {"recording": rec, "npy": paths, "spans": spans, "pll_state": ana.pll_state(0) if pll else None}


if __name__ == "__main__":
    _args = [a for a in sys.argv[1:] if a != "--pll"]
    main(_args[0] if _args else "examples_out", pll="--pll" in sys.argv[1:])
