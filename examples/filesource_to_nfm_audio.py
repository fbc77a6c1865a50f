#!/usr/bin/env python3
"""Narrowband-FM receive path down to audio with the pieces of libsdrx.so, shaped like an SDRangel FileSource device set with
NFM demodulators:

    .sdriq file (FileRecord header + int16 I/Q)  ->  SampleSinkFifo  ->  engine drain loop
        ->  DownChannelizer bank, one channel per carrier, requested rate 48000 (what NFMDemod asks its channelizer for)
        ->  (device hand-over, no host round trip)  NFM demodulator bank: NCO -> Interpolator -> phase discriminator ->
            power squelch with gate -> delay line -> Bandpass -> qint16 mono audio
        ->  one WAV file per carrier (standard library `wave`)

    python examples/filesource_to_nfm_audio.py [out_dir]   # writes a synthetic recording, replays it, saves the audio

examples/filesource_to_nfm.py stops at the discriminator (sdrx_backend_*); this one is the whole demodulator (sdrx_nfm_*).
Everything numeric runs on the MI355X through the C ABI (include/sdrx.h); this script is host glue only."""
import os
import sys
import wave

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sdrangel_amd as sa  # noqa: E402

FS = 2_400_000
CARRIERS = [-825_000, -200_000, 312_500, 900_000]           # offsets from the centre frequency
RF_BW, AF_BW, FM_DEV, VOLUME, SQUELCH, GATE, AUDIO_RATE, REQ_RATE = 12500.0, 3000.0, 2000, 5.0, -400.0, 2, 48000, 48000


def synth_recording(path, seconds=0.4, dev=2000.0):
    """a few FM carriers, each modulated by its own tone (500 Hz, 900 Hz ...), plus noise, as a .sdriq file"""
    n = int(FS * seconds)
    t = np.arange(n) / FS
    x = np.zeros(n, np.complex128)
    for i, fc in enumerate(CARRIERS):
        tone = 500.0 + 400.0 * i
        x += 420.0 * np.exp(1j * (2 * np.pi * fc * t - (dev / tone) * np.cos(2 * np.pi * tone * t)))
    rng = np.random.default_rng(3)
    x += rng.normal(0, 20, n) + 1j * rng.normal(0, 20, n)
    iq = np.empty(2 * n, np.int16)
    iq[0::2] = np.clip(np.round(x.real), -2048, 2047); iq[1::2] = np.clip(np.round(x.imag), -2048, 2047)
    with open(path, "wb") as f:
        f.write(sa.sdriq_header_bytes(FS, 145_500_000, 1_700_000_000, 16))
        f.write(iq.tobytes())
    return n


def demod_cfgs(bank):
    cfgs = []
    for c in range(len(CARRIERS)):
        _modes, out_rate, ofs = bank.info(c)
        cfgs.append(sa.NfmCfg(in_rate=out_rate, nco_freq=-ofs, audio_rate=AUDIO_RATE, rf_bandwidth=RF_BW, af_bandwidth=AF_BW, fm_deviation=FM_DEV,
                              volume=VOLUME, squelch=SQUELCH, squelch_gate=GATE, audio_mute=0))
    return cfgs


def main(out_dir):
    os.makedirs(out_dir, exist_ok=True)
    rec = os.path.join(out_dir, "synthetic_nfm.sdriq")
    n = synth_recording(rec)

    hdr, payload = sa.sdriq_parse(open(rec, "rb").read())   # FileRecord::readHeader + the samples behind it
    assert hdr.sample_rate == FS and hdr.sample_size == 16

    fifo = sa.SampleSinkFifo(FS // 4)
    bank = sa.ChannelizerBank(FS, [REQ_RATE] * len(CARRIERS), CARRIERS)
    nfm = sa.NfmDemodBank(demod_cfgs(bank))

    audio = [[] for _ in CARRIERS]
    spans = []
    block = 2 * 100_000                                     # int16 per "FileSourceThread tick"
    for pos in range(0, payload.size, block):
        fifo.write(payload[pos: pos + block])
        while fifo.fill:                                    # DSPDeviceSourceEngine::work: drain, feed the sinks
            span = fifo.read(fifo.fill)
            spans.append(span.size // 2)
            bank.feed(span)
            nfm.feed_bank(bank)                             # ordered on the device against the bank's stream
            for c in range(len(CARRIERS)):
                bank.skip(c)
                audio[c].append(nfm.read(c))
    paths = []
    for c, fc in enumerate(CARRIERS):
        pcm = np.concatenate(audio[c])
        p = os.path.join(out_dir, f"nfm_ch{c}.wav")
        with wave.open(p, "wb") as w:
            w.setnchannels(1); w.setsampwidth(2); w.setframerate(AUDIO_RATE)
            w.writeframes(pcm.astype("<i2").tobytes())
        paths.append(p)
        z = pcm.astype(np.float64)[AUDIO_RATE // 10:]       # behind the squelch opening (gate 960 samples) and the filter's fill
        spec = np.abs(np.fft.rfft(z - z.mean()))
        f_peak = np.argmax(spec) * AUDIO_RATE / (2 * (spec.size - 1))
        print(f"carrier {c}: {fc:+8d} Hz  {pcm.size} samples at {AUDIO_RATE} S/s, squelch {'open' if nfm.squelch_open(c) else 'closed'}, "
              f"dominant tone {f_peak:7.1f} Hz (sent {500 + 400 * c} Hz) -> {p}")
    print(f"{n} input samples replayed from {rec}")
    return {"recording": rec, "wav": paths, "spans": spans}


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "examples_out")
