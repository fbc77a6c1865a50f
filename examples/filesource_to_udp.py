#!/usr/bin/env python3
"""Channels out as UDP payloads with the pieces of libsdrx.so, shaped like an SDRangel FileSource device set with UDPSrc
channels:

    .sdriq file (FileRecord header + int16 I/Q)  ->  SampleSinkFifo  ->  engine drain loop
        ->  DownChannelizer bank, one channel per carrier, requested rate 48000
        ->  (device hand-over, no host round trip)  UDPSrc bank: NCO -> Interpolator -> input power average -> squelch with
            gate and release -> the channel's sample format (I/Q 16 bit, I/Q 24 bit, FM discriminator, AM without DC behind MagAGC) -> payload
            samples
        ->  cut into the 512-byte datagrams UDPSink<T>::write would send, appended to one file per channel

    python examples/filesource_to_udp.py [out_dir] [--format 0,1,3,9]
        writes a synthetic recording, replays it, saves the datagram payloads.  --format names the four channels' sample formats
        (UDPSrcSettings::SampleFormat, a trailing `a` turns m_agc on): `--format 4,5a,6,7a` sends the carriers out as LSB (with
        its interleaved raw I/Q), USB, LSB mono and USB mono in blocks of 256 elements from fftfilt's 512-point filter

NO socket is opened anywhere: the datagram payloads go to files (`udp_ch<N>.bin`, datagram after datagram, 512 bytes each);
sending them is one sendto() per 512 bytes for whoever has a network to send them on.
Everything numeric runs on the MI355X through the C ABI (include/sdrx.h); this script is host glue only."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sdrangel_amd as sa  # noqa: E402

FS = 2_400_000
CARRIERS = [-825_000, -200_000, 312_500, 900_000]           # offsets from the centre frequency
FORMATS = [0, 1, 3, 9]                                      # FormatIQ16, FormatIQ24, FormatNFMMono, FormatAMNoDCMono
AGC = [0, 0, 0, 1]                                          # m_agc: MagAGC in front of the AM channel's gain
RF_BW, FM_DEV, GAIN, SQUELCH_DB, GATE, OUT_RATE, REQ_RATE = 12500.0, 2500, 4.0, -50, 2, 24000.0, 48000


def synth_recording(path, seconds=0.4, dev=2000.0):
    """a few carriers, each frequency- and amplitude-modulated by its own tone (500 Hz, 900 Hz ...), plus noise, as a .sdriq file"""
    n = int(FS * seconds)
    t = np.arange(n) / FS
    x = np.zeros(n, np.complex128)
    for i, fc in enumerate(CARRIERS):
        tone = 500.0 + 400.0 * i
        x += 420.0 * (1.0 + 0.5 * np.sin(2 * np.pi * tone * t)) * np.exp(1j * (2 * np.pi * fc * t - (dev / tone) * np.cos(2 * np.pi * tone * t)))
    rng = np.random.default_rng(3)
    x += rng.normal(0, 20, n) + 1j * rng.normal(0, 20, n)
    iq = np.empty(2 * n, np.int16)
    iq[0::2] = np.clip(np.round(x.real), -2048, 2047); iq[1::2] = np.clip(np.round(x.imag), -2048, 2047)
    with open(path, "wb") as f:
        f.write(sa.sdriq_header_bytes(FS, 145_500_000, 1_700_000_000, 16))
        f.write(iq.tobytes())
    return n


def channel_cfgs(bank, formats=None, agc=None):
    formats, agc = formats or FORMATS, agc or AGC
    cfgs = []
    for c in range(len(CARRIERS)):
        _modes, out_rate, ofs = bank.info(c)
        cfgs.append(sa.UdpSrcCfg(in_rate=out_rate, nco_freq=-ofs, output_sample_rate=OUT_RATE, sample_format=formats[c], rf_bandwidth=RF_BW,
                                 fm_deviation=FM_DEV, gain=GAIN, squelch_db=SQUELCH_DB, squelch_gate=GATE, squelch_enabled=1, agc=agc[c]))
    return cfgs


def parse_formats(text):
    """`4,5a,6,7a` -> ([4, 5, 6, 7], [0, 1, 0, 1])"""
    items = text.split(",")
    if len(items) != len(CARRIERS):
        raise SystemExit(f"--format takes {len(CARRIERS)} comma-separated sample formats, one per carrier")
    return [int(v.rstrip("a")) for v in items], [int(v.endswith("a")) for v in items]


def main(out_dir, formats=None, agc=None):
    formats, agc = formats or FORMATS, agc or AGC
    os.makedirs(out_dir, exist_ok=True)
    rec = os.path.join(out_dir, "synthetic_udp.sdriq")
    n = synth_recording(rec)

    hdr, payload = sa.sdriq_parse(open(rec, "rb").read())   # FileRecord::readHeader + the samples behind it
    assert hdr.sample_rate == FS and hdr.sample_size == 16

    fifo = sa.SampleSinkFifo(FS // 4)
    bank = sa.ChannelizerBank(FS, [REQ_RATE] * len(CARRIERS), CARRIERS)
    udp = sa.UdpSrcBank(channel_cfgs(bank, formats, agc))     # sdrx_udpsrc_create_ex when a channel has an SSB format

    paths = [os.path.join(out_dir, f"udp_ch{c}.bin") for c in range(len(CARRIERS))]
    files = [open(p, "wb") for p in paths]
    sent = [0] * len(CARRIERS)
    spans = []
    block = 2 * 100_000                                     # int16 per "FileSourceThread tick"
    for pos in range(0, payload.size, block):
        fifo.write(payload[pos: pos + block])
        while fifo.fill:                                    # DSPDeviceSourceEngine::work: drain, feed the sinks
            span = fifo.read(fifo.fill)
            spans.append(span.size // 2)
            bank.feed(span)
            udp.feed_bank(bank)                             # ordered on the device against the bank's stream
            for c in range(len(CARRIERS)):
                bank.skip(c)
                for datagram in udp.payloads(c):            # where UDPSrc would call writeDatagram
                    files[c].write(datagram)
                    sent[c] += 1
    for f in files:
        f.close()
    for c, fc in enumerate(CARRIERS):
        print(f"carrier {c}: {fc:+8d} Hz  format {formats[c]}, {udp.total(c)} samples of {udp.sample_bytes(c)} bytes at {OUT_RATE:.0f} S/s, "
              f"{sent[c]} datagrams, squelch {'open' if udp.squelch_open(c) else 'closed'}, input power {udp.in_magsq(c):.3e} -> {paths[c]}")
    print(f"{n} input samples replayed from {rec}")
    return {"recording": rec, "payloads": paths, "spans": spans, "datagrams": sent, "totals": [udp.total(c) for c in range(len(CARRIERS))]}


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("out_dir", nargs="?", default="examples_out")
    ap.add_argument("--format", default=",".join(f"{f}{'a' if a else ''}" for f, a in zip(FORMATS, AGC)),
                    help="one sample format per carrier, 0 .. 10; a trailing a: m_agc on")
    args = ap.parse_args()
    main(args.out_dir, *parse_formats(args.format))
