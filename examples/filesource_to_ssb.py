#!/usr/bin/env python3
"""SSB receive path down to audio with the pieces of libsdrx.so, shaped like an SDRangel FileSource device set with SSB
demodulators:

    .sdriq file (FileRecord header + int16 I/Q)  ->  SampleSinkFifo  ->  engine drain loop
        ->  DownChannelizer bank, one channel per carrier, requested rate 48000 (what SSBDemod asks its channelizer for)
        ->  (device hand-over, no host round trip)  SSB demodulator bank: NCO -> Interpolator -> fftfilt sideband filter ->
            MagAGC with threshold and gate -> delay line -> step value -> qint16 l, r audio; the decimated sideband stream of
            the spectrum sink beside it
        ->  one stereo WAV file per carrier (standard library `wave`)

    python examples/filesource_to_ssb.py [out_dir]   # writes a synthetic recording, replays it, saves the audio

The carriers are an upper-sideband tone, a lower-sideband tone, a binaural USB channel and a DSB channel.  Everything numeric
runs on the MI355X through the C ABI (include/sdrx.h); this script is host glue only."""
import os
import sys
import wave

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sdrangel_amd as sa  # noqa: E402

FS = 2_400_000
CARRIERS = [-825_000, -200_000, 312_500, 900_000]           # suppressed-carrier frequencies, offsets from the centre
TONES = [700.0, -1100.0, 1500.0, 900.0]                     # audio tone beside each carrier: above (USB), below (LSB)
AUDIO_RATE, REQ_RATE = 48000, 48000
#: per carrier: what differs from the defaults below
KINDS = [dict(), dict(rf_bandwidth=-3000.0, low_cutoff=-300.0), dict(audio_binaural=1), dict(dsb=1)]
COMMON = dict(rf_bandwidth=3000.0, low_cutoff=300.0, volume=3.0, span_log2=3, audio_binaural=0, audio_flip=0, dsb=0, audio_mute=0,
              agc=1, agc_clamping=0, agc_time_log2=5, agc_power_threshold=-60, agc_threshold_gate=4)


def synth_recording(path, seconds=0.4):
    """one tone beside each suppressed carrier, plus noise, as a .sdriq file"""
    n = int(FS * seconds)
    t = np.arange(n) / FS
    x = np.zeros(n, np.complex128)
    for fc, tone in zip(CARRIERS, TONES):
        x += 420.0 * np.exp(2j * np.pi * (fc + tone) * t)
    rng = np.random.default_rng(3)
    x += rng.normal(0, 20, n) + 1j * rng.normal(0, 20, n)
    iq = np.empty(2 * n, np.int16)
    iq[0::2] = np.clip(np.round(x.real), -2048, 2047); iq[1::2] = np.clip(np.round(x.imag), -2048, 2047)
    with open(path, "wb") as f:
        f.write(sa.sdriq_header_bytes(FS, 14_200_000, 1_700_000_000, 16))
        f.write(iq.tobytes())
    return n


def channel_settings(c, out_rate, ofs):
    """the sdrx_ssb_cfg fields of carrier c behind a channelizer that delivers out_rate with the carrier at ofs"""
    d = dict(COMMON); d.update(KINDS[c])
    d.update(in_rate=out_rate, nco_freq=-ofs, audio_rate=AUDIO_RATE)
    return d


def main(out_dir):
    os.makedirs(out_dir, exist_ok=True)
    rec = os.path.join(out_dir, "synthetic_ssb.sdriq")
    n = synth_recording(rec)

    hdr, payload = sa.sdriq_parse(open(rec, "rb").read())   # FileRecord::readHeader + the samples behind it
    assert hdr.sample_rate == FS and hdr.sample_size == 16

    fifo = sa.SampleSinkFifo(FS // 4)
    bank = sa.ChannelizerBank(FS, [REQ_RATE] * len(CARRIERS), CARRIERS)
    ssb = sa.SsbDemodBank([sa.SsbCfg(**channel_settings(c, *bank.info(c)[1:])) for c in range(len(CARRIERS))])

    audio = [[] for _ in CARRIERS]
    n_spec = [0] * len(CARRIERS)
    spans = []
    block = 2 * 100_000                                     # int16 per "FileSourceThread tick"
    for pos in range(0, payload.size, block):
        fifo.write(payload[pos: pos + block])
        while fifo.fill:                                    # DSPDeviceSourceEngine::work: drain, feed the sinks
            span = fifo.read(fifo.fill)
            spans.append(span.size // 2)
            bank.feed(span)
            ssb.feed_bank(bank)                             # ordered on the device against the bank's stream
            for c in range(len(CARRIERS)):
                bank.skip(c)
                audio[c].append(ssb.read(c))                # many feeds hand out nothing: the filter works in blocks of 512 / 1024
                n_spec[c] += ssb.read_spectrum(c).shape[0]
    paths = []
    for c, fc in enumerate(CARRIERS):
        pcm = np.concatenate(audio[c])                      # [n, 2]: l, r
        p = os.path.join(out_dir, f"ssb_ch{c}.wav")
        with wave.open(p, "wb") as w:
            w.setnchannels(2); w.setsampwidth(2); w.setframerate(AUDIO_RATE)
            w.writeframes(pcm.astype("<i2").tobytes())
        paths.append(p)
        z = pcm[AUDIO_RATE // 10:, 0].astype(np.float64)    # behind the AGC's delay line (1536 samples) and its step up
        spec = np.abs(np.fft.rfft(z - z.mean()))
        f_peak = np.argmax(spec) * AUDIO_RATE / (2 * (spec.size - 1))
        print(f"carrier {c}: {fc:+8d} Hz  {pcm.shape[0]} stereo samples at {AUDIO_RATE} S/s, {n_spec[c]} spectrum samples, audio "
              f"{'active' if ssb.audio_active(c) else 'idle'}, dominant tone {f_peak:7.1f} Hz (sent {abs(TONES[c]):.0f} Hz) -> {p}")
    print(f"{n} input samples replayed from {rec}")
    return {"recording": rec, "wav": paths, "spans": spans}


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "examples_out")
