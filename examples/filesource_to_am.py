#!/usr/bin/env python3
"""Airband AM receive path with the pieces of libsdrx.so, shaped like an SDRangel FileSource device set with AM demodulators:

    .sdriq file (FileRecord header + int16 I/Q)  ->  SampleSinkFifo  ->  engine drain loop
        ->  DownChannelizer bank, one channel per carrier, requested rate 48000 (what AMDemod asks its channelizer for)
        ->  (device hand-over, no host round trip)  AM demodulator bank: NCO -> Interpolator -> power squelch -> delayed
            envelope -> volume AGC -> Bandpass -> qint16 mono audio
        ->  one WAV file per carrier (standard library `wave`)

    python examples/filesource_to_am.py [out_dir]          # writes a synthetic recording, replays it, saves the audio
    python examples/filesource_to_am.py [out_dir] --sync dsb|usb|lsb     # the same with synchronous AM (m_pll): prefilter -> PLL ->
                                                           # sideband filter -> AGC in place of the envelope; prints the PLL lock per carrier

Everything numeric runs on the MI355X through the C ABI (include/sdrx.h); this script is host glue only."""
import os
import sys
import wave

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sdrangel_amd as sa  # noqa: E402

FS = 2_400_000
CARRIERS = [-825_000, -200_000, 308_330, 900_000]          # offsets from the centre frequency
RF_BW, VOLUME, SQUELCH_DB, AUDIO_RATE, REQ_RATE = 5000.0, 2.0, -40.0, 48000, 48000


def synth_recording(path, seconds=0.4, depth=0.6):
    """a few AM carriers, each modulated by its own tone (500 Hz, 900 Hz ...), plus noise, as a .sdriq file"""
    n = int(FS * seconds)
    t = np.arange(n) / FS
    x = np.zeros(n, np.complex128)
    for i, fc in enumerate(CARRIERS):
        tone = 500.0 + 400.0 * i
        x += 420.0 * (1.0 + depth * np.sin(2 * np.pi * tone * t)) * np.exp(2j * np.pi * fc * t)
    rng = np.random.default_rng(2)
    x += rng.normal(0, 20, n) + 1j * rng.normal(0, 20, n)
    iq = np.empty(2 * n, np.int16)
    iq[0::2] = np.clip(np.round(x.real), -2048, 2047); iq[1::2] = np.clip(np.round(x.imag), -2048, 2047)
    with open(path, "wb") as f:
        f.write(sa.sdriq_header_bytes(FS, 121_500_000, 1_700_000_000, 16))
        f.write(iq.tobytes())
    return n


def demod_cfgs(bank):
    cfgs = []
    for c in range(len(CARRIERS)):
        _modes, out_rate, ofs = bank.info(c)
        cfgs.append(sa.AmCfg(in_rate=out_rate, nco_freq=-ofs, audio_rate=AUDIO_RATE, rf_bandwidth=RF_BW, volume=VOLUME, squelch_db=SQUELCH_DB,
                             audio_mute=0, bandpass_enable=1))
    return cfgs


SYNC_OPS = {"dsb": 0, "usb": 1, "lsb": 2}


def main(out_dir, sync=None):
    os.makedirs(out_dir, exist_ok=True)
    rec = os.path.join(out_dir, "synthetic_am.sdriq")
    n = synth_recording(rec)

    hdr, payload = sa.sdriq_parse(open(rec, "rb").read())   # FileRecord::readHeader + the samples behind it
    assert hdr.sample_rate == FS and hdr.sample_size == 16

    fifo = sa.SampleSinkFifo(FS // 4)
    bank = sa.ChannelizerBank(FS, [REQ_RATE] * len(CARRIERS), CARRIERS)
    # SSBFilter as an AMDemod constructed at this audio rate with the default bandwidth has it
    options = None if sync is None else [sa.AmSyncCfg(pll=1, sync_op=SYNC_OPS[sync], ssb_design_rate=AUDIO_RATE, ssb_design_bw=RF_BW)] * len(CARRIERS)
    am = sa.AmDemodBank(demod_cfgs(bank), sync=options)

    audio = [[] for _ in CARRIERS]
    spans = []
    block = 2 * 100_000                                     # int16 per "FileSourceThread tick"
    for pos in range(0, payload.size, block):
        fifo.write(payload[pos: pos + block])
        while fifo.fill:                                    # DSPDeviceSourceEngine::work: drain, feed the sinks
            span = fifo.read(fifo.fill)
            spans.append(span.size // 2)
            bank.feed(span)
            am.feed_bank(bank)                              # ordered on the device against the bank's stream
            for c in range(len(CARRIERS)):
                bank.skip(c)
                audio[c].append(am.read(c))
    paths = []
    for c, fc in enumerate(CARRIERS):
        pcm = np.concatenate(audio[c])
        p = os.path.join(out_dir, f"am_ch{c}.wav")
        with wave.open(p, "wb") as w:
            w.setnchannels(1); w.setsampwidth(2); w.setframerate(AUDIO_RATE)
            w.writeframes(pcm.astype("<i2").tobytes())
        paths.append(p)
        z = pcm.astype(np.float64)[AUDIO_RATE // 10:]       # behind the squelch opening and its attack
        spec = np.abs(np.fft.rfft(z - z.mean()))
        f_peak = np.argmax(spec) * AUDIO_RATE / (2 * (spec.size - 1))
        print(f"carrier {c}: {fc:+8d} Hz  {pcm.size} samples at {AUDIO_RATE} S/s, squelch {'open' if am.squelch_open(c) else 'closed'}, "
              f"dominant tone {f_peak:7.1f} Hz (sent {500 + 400 * c} Hz) -> {p}")
        if sync is not None:
            locked, freq = am.pll(c)
            print(f"carrier {c}: sync {sync}, PLL {'locked' if locked else 'not locked'}, loop frequency {freq * AUDIO_RATE / (2 * np.pi):+8.2f} Hz")
    print(f"{n} input samples replayed from {rec}")
    return {"recording": rec, "wav": paths, "spans": spans, "pll": None if sync is None else [am.pll(c) for c in range(len(CARRIERS))]}


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("out_dir", nargs="?", default="examples_out")
    ap.add_argument("--sync", choices=sorted(SYNC_OPS), default=None, help="synchronous AM with that sideband operation")
    a = ap.parse_args()
    main(a.out_dir, a.sync)
