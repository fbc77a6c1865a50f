#!/usr/bin/env python3
"""Broadcast-FM receive path with the pieces of libsdrx.so, shaped like an SDRangel FileSource device set with WFM demodulators:

    .sdriq file (FileRecord header + int16 I/Q)  ->  SampleSinkFifo  ->  engine drain loop
        ->  DownChannelizer bank, one channel per station, requested rate = WFMDemod::requiredBW(rfBandwidth)
        ->  (device hand-over, no host round trip)  WFM demodulator bank: NCO -> fftfilt at the channel rate -> squelch ->
            gated discriminator -> Interpolator -> qint16 mono audio
        ->  one WAV file per station (standard library `wave`)

    python examples/filesource_to_wfm.py [out_dir]          # writes a synthetic recording, replays it, saves the audio

Everything numeric runs on the MI355X through the C ABI (include/sdrx.h); this script is host glue only."""
import os
import sys
import wave

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sdrangel_amd as sa  # noqa: E402

FS = 2_400_000
STATIONS = [-800_000, -200_000, 300_000, 900_000]          # offsets from the centre frequency
RF_BW, AF_BW, VOLUME, SQUELCH_DB, AUDIO_RATE = 80000.0, 15000.0, 2.0, -60.0, 48000


def synth_recording(path, seconds=0.2, dev_hz=50000.0):
    """a few broadcast-FM carriers, each modulated by its own tone (500 Hz, 900 Hz ...), plus noise, as a .sdriq file"""
    n = int(FS * seconds)
    t = np.arange(n) / FS
    x = np.zeros(n, np.complex128)
    for i, fc in enumerate(STATIONS):
        tone = 500.0 + 400.0 * i
        x += 450.0 * np.exp(1j * (2 * np.pi * fc * t + (dev_hz / tone) * np.sin(2 * np.pi * tone * t)))
    rng = np.random.default_rng(2)
    x += rng.normal(0, 20, n) + 1j * rng.normal(0, 20, n)
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
        cfgs.append(sa.WfmCfg(in_rate=out_rate, nco_freq=-ofs, audio_rate=AUDIO_RATE, rf_bandwidth=RF_BW, af_bandwidth=AF_BW,
                              volume=VOLUME, squelch_db=SQUELCH_DB, audio_mute=0))
    return cfgs


def main(out_dir):
    os.makedirs(out_dir, exist_ok=True)
    rec = os.path.join(out_dir, "synthetic_fm.sdriq")
    n = synth_recording(rec)

    hdr, payload = sa.sdriq_parse(open(rec, "rb").read())   # FileRecord::readHeader + the samples behind it
    assert hdr.sample_rate == FS and hdr.sample_size == 16

    fifo = sa.SampleSinkFifo(FS // 4)
    req = sa.wfm_required_bw(int(RF_BW))                    # what WFMDemod asks its channelizer for
    bank = sa.ChannelizerBank(FS, [req] * len(STATIONS), STATIONS)
    wfm = sa.WfmDemodBank(demod_cfgs(bank))

    audio = [[] for _ in STATIONS]
    spans = []
    block = 2 * 100_000                                     # int16 per "FileSourceThread tick"
    for pos in range(0, payload.size, block):
        fifo.write(payload[pos: pos + block])
        while fifo.fill:                                    # DSPDeviceSourceEngine::work: drain, feed the sinks
            span = fifo.read(fifo.fill)
            spans.append(span.size // 2)
            bank.feed(span)
            wfm.feed_bank(bank)                             # ordered on the device against the bank's stream
            for c in range(len(STATIONS)):
                bank.skip(c)
                audio[c].append(wfm.read(c))
    paths = []
    for c, fc in enumerate(STATIONS):
        pcm = np.concatenate(audio[c])
        p = os.path.join(out_dir, f"wfm_ch{c}.wav")
        with wave.open(p, "wb") as w:
            w.setnchannels(1); w.setsampwidth(2); w.setframerate(AUDIO_RATE)
            w.writeframes(pcm.astype("<i2").tobytes())
        paths.append(p)
        z = pcm.astype(np.float64)[2000:]
        spec = np.abs(np.fft.rfft(z - z.mean()))
        f_peak = np.argmax(spec) * AUDIO_RATE / (2 * (spec.size - 1))
        print(f"station {c}: {fc:+8d} Hz  {pcm.size} samples at {AUDIO_RATE} S/s, squelch {'open' if wfm.squelch_open(c) else 'closed'}, "
              f"dominant tone {f_peak:7.1f} Hz (sent {500 + 400 * c} Hz) -> {p}")
    print(f"{n} input samples replayed from {rec}")
    return {"recording": rec, "wav": paths, "spans": spans}


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "examples_out")
