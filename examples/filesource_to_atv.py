#!/usr/bin/env python3
"""ATV receive path with the pieces of libsdrx.so, shaped like an SDRangel FileSource device set with ATV demodulators:

    .sdriq file (FileRecord header + int16 I/Q)  ->  SampleSinkFifo  ->  engine drain loop
        ->  DownChannelizer bank, one channel per carrier
        ->  (device hand-over, no host round trip)  ATV demodulator bank: NCO -> FM / AM video demodulation -> sync detection ->
            pixels into the channel's screen, a snapshot at every renderImage
        ->  one .pgm per stored frame, and the screen as it stands at the end

    python examples/filesource_to_atv.py [out_dir]        # writes a synthetic recording, replays it, writes the frames

Everything numeric runs on the MI355X through the C ABI (include/sdrx.h); this script is host glue only."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sdrangel_amd as sa  # noqa: E402

FS = 640_000
CARRIERS = [-160_000, 160_000]                              # offsets from the centre frequency
REQ_RATES = [160_000, 160_000]                              # what each demodulator asks its channelizer for
MODULATIONS = [2, 3]                                        # ATV_FM3, ATV_AM
LINES, FPS, SPL, SPT = 64, 25.0, 100, 7                     # a small picture: 64 lines of 100 samples at the channel rate, tops of 7
FRAMES = 6


def video(n_frames):
    """levels (0 sync, 0.3 black, 1 white) at the channel rate: two broad-pulse lines, then lines with a sync pulse, a porch and a
    picture of diagonal bars"""
    line = np.full(SPL, 0.3)
    line[:SPT + 1] = 0.0
    wide = np.full(SPL, 0.3)
    wide[:(9 * SPL) // 10] = 0.0
    x = np.arange(2 * (SPT + 1), SPL - 3)
    rows = []
    for r in range(LINES):
        if r < 2:
            rows.append(wide)
        else:
            row = line.copy()
            row[x] = 0.3 + 0.7 * (((x + 2 * r) // 12) % 2) * (0.5 + 0.5 * r / LINES)
            rows.append(row)
    return np.tile(np.concatenate(rows), n_frames)


def synth_recording(path, signal=None):
    """one ATV signal per carrier plus noise, as a .sdriq file; `signal`: complex samples at FS to use instead"""
    if signal is None:
        rng = np.random.default_rng(7)
        v = np.repeat(video(FRAMES), FS // REQ_RATES[0])
        t = np.arange(v.size) / FS
        fm = np.exp(1j * np.cumsum((v - 0.5) * np.pi * REQ_RATES[0] / FS))
        am = 0.1 + 0.9 * v
        signal = 5000.0 * fm * np.exp(2j * np.pi * CARRIERS[0] * t) + 5000.0 * am * np.exp(2j * np.pi * CARRIERS[1] * t)
        signal = signal + rng.normal(0, 30, v.size) + 1j * rng.normal(0, 30, v.size)
    iq = np.empty(2 * signal.size, np.int16)
    iq[0::2] = np.clip(np.round(signal.real), -32768, 32767); iq[1::2] = np.clip(np.round(signal.imag), -32768, 32767)
    with open(path, "wb") as f:
        f.write(sa.sdriq_header_bytes(FS, 1_255_000_000, 1_700_000_000, 16))
        f.write(iq.tobytes())
    return signal.size


def demod_cfgs(bank):
    cfgs = []
    for c, mod in enumerate(MODULATIONS):
        _modes, out_rate, ofs = bank.info(c)
        cfgs.append(sa.AtvCfg(in_rate=out_rate, nco_freq=-ofs, modulation=mod, rf_bw=60000.0, rf_opp_bw=10000.0, fft_filtering=0, decimator_enable=0,
                              fm_deviation=1.0, line_duration=(SPL + 0.25) / out_rate, top_duration=(SPT + 0.25) / out_rate, frames_per_s=FPS,
                              standard=4, n_lines=LINES, level_synchro_top=0.1, level_black=0.3, hsync=1, vsync=1, invert_video=0, scope=0, frames_cap=8))
    return cfgs


def write_pgm(path, img):
    with open(path, "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (img.shape[1], img.shape[0]))
        f.write(np.ascontiguousarray(img, np.uint8).tobytes())


def main(out_dir, signal=None):
    os.makedirs(out_dir, exist_ok=True)
    rec = os.path.join(out_dir, "synthetic_atv.sdriq")
    n = synth_recording(rec, signal)

    hdr, payload = sa.sdriq_parse(open(rec, "rb").read())   # FileRecord::readHeader + the samples behind it
    assert hdr.sample_rate == FS and hdr.sample_size == 16

    fifo = sa.SampleSinkFifo(FS // 4)
    bank = sa.ChannelizerBank(FS, REQ_RATES, CARRIERS)
    cfgs = demod_cfgs(bank)
    atv = sa.ATVBank(cfgs)

    frames = [[] for _ in CARRIERS]
    events = [[] for _ in CARRIERS]
    spans = []
    block = 2 * 100_000                                     # int16 per "FileSourceThread tick"
    for pos in range(0, payload.size, block):
        fifo.write(payload[pos: pos + block])
        while fifo.fill:                                    # DSPDeviceSourceEngine::work: drain, feed the sinks
            span = fifo.read(fifo.fill)
            spans.append(span.size // 2)
            bank.feed(span)
            atv.feed_bank(bank)                             # ordered on the device against the bank's stream
            for c in range(len(CARRIERS)):
                bank.skip(c)
                stored, rendered = atv.frames(c)
                events[c].append(atv.events(c))
                for k in range(stored):
                    p = os.path.join(out_dir, f"atv_ch{c}_frame{len(frames[c]):03d}.pgm")
                    write_pgm(p, atv.frame(c, k))
                    frames[c].append(p)
    screens = []
    for c, fc in enumerate(CARRIERS):
        p = os.path.join(out_dir, f"atv_ch{c}_screen.pgm")
        write_pgm(p, atv.screen(c))
        screens.append(p)
        st = atv.state(c)
        print(f"carrier {c}: {fc:+8d} Hz, modulation {MODULATIONS[c]}: {len(frames[c])} frames stored, image index {st.image_index} -> {p}")
    print(f"{n} input samples replayed from {rec}")
    return {"recording": rec, "frames": frames, "screens": screens, "events": events, "spans": spans, "cfgs": cfgs,
            "state": [atv.state(c) for c in range(len(CARRIERS))]}


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "examples_out")
