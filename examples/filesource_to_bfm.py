#!/usr/bin/env python3
"""Broadcast-FM stereo receive path with the pieces of libsdrx.so, shaped like an SDRangel FileSource device set with BFM demodulators:

    .sdriq file (FileRecord header + int16 I/Q)  ->  SampleSinkFifo  ->  engine drain loop
        ->  DownChannelizer bank, one channel per station at 240 kS/s
        ->  (device hand-over, no host round trip)  BFM demodulator bank: NCO -> fftfilt at the channel rate -> squelch -> gated
            discriminator -> 19 kHz pilot loop -> mono and stereo-difference resamplers -> de-emphasis -> qint16 l, r
        ->  one stereo WAV file per station (standard library `wave`), the pilot lock printed

    python examples/filesource_to_bfm.py [out_dir]          # writes a synthetic recording, replays it, saves the audio

Everything numeric runs on the MI355X through the C ABI (include/sdrx.h); this script is host glue only.  RDS is not decoded here: the bank
can (sdrx_bfmrds_*, BfmBank(cfgs, rds=[...])), but it needs 250 kS/s or more per station and seconds of signal."""
import os
import sys
import wave

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sdrangel_amd as sa  # noqa: E402

FS = 1_920_000
STATIONS = [-600_000, 150_000, 700_000]                     # offsets from the centre frequency
CHANNEL_RATE = 240_000
RF_BW, AF_BW, VOLUME, SQUELCH_DB, AUDIO_RATE = 100000.0, 15000.0, 4.0, -70.0, 48000


def synth_recording(path, seconds=0.04):
    """a few stereo stations as a .sdriq file: per station a left and a right tone, the 19 kHz pilot at a tenth of the deviation and
    L - R on the suppressed 38 kHz carrier, frequency-modulated with 50 kHz of deviation; plus noise"""
    n = int(FS * seconds)
    t = np.arange(n) / FS
    x = np.zeros(n, np.complex128)
    for i, fc in enumerate(STATIONS):
        left, right = np.sin(2 * np.pi * (500.0 + 400.0 * i) * t), np.sin(2 * np.pi * (1300.0 + 300.0 * i) * t)
        pil = 2 * np.pi * 19000.0 * t
        m = 0.45 * (left + right) + 0.1 * np.sin(pil) + 0.45 * (left - right) * np.sin(2 * pil)
        x += 450.0 * np.exp(1j * (2 * np.pi * fc * t + 2 * np.pi * 50000.0 * np.cumsum(m) / FS))
    rng = np.random.default_rng(3)
    x += rng.normal(0, 5, n) + 1j * rng.normal(0, 5, n)
    iq = np.empty(2 * n, np.int16)
    iq[0::2] = np.clip(np.round(x.real), -2048, 2047); iq[1::2] = np.clip(np.round(x.imag), -2048, 2047)
    with open(path, "wb") as f:
        f.write(sa.sdriq_header_bytes(FS, 98_000_000, 1_700_000_000, 16))
        f.write(iq.tobytes())
    return n


def demod_cfgs(bank):
    cfgs = []
    for c in range(len(STATIONS)):
        _modes, out_rate, ofs = bank.info(c)
        cfgs.append(sa.BfmCfg(in_rate=out_rate, nco_freq=-ofs, audio_rate=AUDIO_RATE, rf_bandwidth=RF_BW, af_bandwidth=AF_BW, volume=VOLUME,
                              squelch_db=SQUELCH_DB, audio_stereo=1, lsb_stereo=c % 2, show_pilot=0))
    return cfgs


def main(out_dir):
    os.makedirs(out_dir, exist_ok=True)
    rec = os.path.join(out_dir, "synthetic_bfm.sdriq")
    n = synth_recording(rec)

    hdr, payload = sa.sdriq_parse(open(rec, "rb").read())   # FileRecord::readHeader + the samples behind it
    assert hdr.sample_rate == FS and hdr.sample_size == 16

    fifo = sa.SampleSinkFifo(FS // 4)
    bank = sa.ChannelizerBank(FS, [CHANNEL_RATE] * len(STATIONS), STATIONS)
    bfm = sa.BfmBank(demod_cfgs(bank))

    audio = [[] for _ in STATIONS]
    spans = []
    block = 2 * 20_000                                      # int16 per "FileSourceThread tick"
    for pos in range(0, payload.size, block):
        fifo.write(payload[pos: pos + block])
        while fifo.fill:                                    # DSPDeviceSourceEngine::work: drain, feed the sinks
            span = fifo.read(fifo.fill)
            spans.append(span.size // 2)
            bank.feed(span)
            bfm.feed_bank(bank)                             # ordered on the device against the bank's stream
            for c in range(len(STATIONS)):
                bank.skip(c)
                audio[c].append(bfm.read(c))
    paths, pilots = [], []
    for c, fc in enumerate(STATIONS):
        pcm = np.concatenate(audio[c])
        p = os.path.join(out_dir, f"bfm_ch{c}.wav")
        with wave.open(p, "wb") as w:
            w.setnchannels(2); w.setsampwidth(2); w.setframerate(AUDIO_RATE)
            w.writeframes(pcm.astype("<i2").tobytes())
        paths.append(p)
        locked, level, _f, _p = bfm.pilot(c)
        pilots.append((locked, level))
        print(f"station {c}: {fc:+8d} Hz  {pcm.shape[0]} l, r pairs at {AUDIO_RATE} S/s, squelch {'open' if bfm.squelch_open(c) else 'closed'}, "
              f"pilot {'locked' if locked else 'not locked (0.4 s of pilot needed)'}, pilot level {level:.4f} -> {p}")
    print(f"{n} input samples replayed from {rec}")
    return {"recording": rec, "wav": paths, "spans": spans, "pilot": pilots}


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "examples_out")
