#!/usr/bin/env python3
"""DATV receive path with the pieces of libsdrx.so, shaped like an SDRangel FileSource device set with DATV demodulators:

    .sdriq file (FileRecord header + int16 I/Q)  ->  SampleSinkFifo  ->  engine drain loop
        ->  DownChannelizer bank, one channel per carrier
        ->  (device hand-over, no host round trip)  DATV receiver bank: NCO -> RF filter -> sampler, PLL and timing loop ->
            soft symbols, one constellation point per chunk, a measurement every meas_decimation samples
        ->  symbols and measurements as .npy per carrier; lock printed as MER over time

    python examples/filesource_to_datv.py [out_dir]        # writes a synthetic recording, replays it, writes the arrays

The soft symbols are what leansdr's deconvol_sync_simple / viterbi_sync take: the byte-rate half of the receiver (deconvolution,
mpeg_sync, deinterleaver, Reed-Solomon, derandomizer) stays on the host and is not part of this script.  Everything numeric here
runs on the MI355X through the C ABI (include/sdrx.h); this script is host glue only."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sdrangel_amd as sa  # noqa: E402

FS = 4_000_000
CARRIERS = [-1_000_000, 1_000_000]                          # offsets from the centre frequency
REQ_RATES = [1_000_000, 1_000_000]                          # what each demodulator asks its channelizer for
SYMBOL_RATES = [250_000, 500_000]
SAMPLERS = [2, 1]                                           # RRC, linear
SECONDS = 0.1


def qpsk(n, sps, rng):
    """n samples of a QPSK symbol train at sps samples per symbol, raised-cosine shaped"""
    nsym = int(n / sps) + 12
    train = np.exp(1j * (np.pi / 4 + np.pi / 2 * rng.integers(0, 4, nsym)))
    t = (np.arange(n) + 0.3) / sps
    base = np.floor(t).astype(np.int64)
    acc = np.zeros(n, np.complex128)
    for d in range(-4, 5):
        idx = base + d
        x = t - idx
        den = 1.0 - (0.7 * x) ** 2
        h = np.sinc(x) * np.cos(np.pi * 0.35 * x) / np.where(np.abs(den) < 1e-9, 1e-9, den)
        acc += np.where((idx >= 0) & (idx < nsym), train[np.clip(idx, 0, nsym - 1)] * h, 0.0)
    return acc


def synth_recording(path):
    """one QPSK signal per carrier plus noise, as a .sdriq file"""
    rng = np.random.default_rng(7)
    n = int(FS * SECONDS)
    t = np.arange(n) / FS
    signal = sum(4000.0 * qpsk(n, FS / fm, rng) * np.exp(2j * np.pi * fc * t) for fc, fm in zip(CARRIERS, SYMBOL_RATES))
    signal = signal + rng.normal(0, 100, n) + 1j * rng.normal(0, 100, n)
    iq = np.empty(2 * n, np.int16)
    iq[0::2] = np.clip(np.round(signal.real), -32768, 32767); iq[1::2] = np.clip(np.round(signal.imag), -32768, 32767)
    with open(path, "wb") as f:
        f.write(sa.sdriq_header_bytes(FS, 1_255_000_000, 1_700_000_000, 16))
        f.write(iq.tobytes())
    return n


def demod_cfgs(bank):
    cfgs = []
    for c, (fm, sampler) in enumerate(zip(SYMBOL_RATES, SAMPLERS)):
        _modes, out_rate, ofs = bank.info(c)
        cfgs.append(sa.DatvCfg(msps=out_rate, sample_rate=out_rate, centre_frequency=ofs, rf_bandwidth=int(1.6 * fm), symbol_rate=fm, modulation=1, fec=0,
                               standard=0, sampler=sampler, rolloff=0.35, excursion=10, hard_metric=0, viterbi=0, allow_drift=0, notch_filters=0,
                               finfo=200.0))
    return cfgs


def main(out_dir):
    os.makedirs(out_dir, exist_ok=True)
    rec = os.path.join(out_dir, "synthetic_datv.sdriq")
    n = synth_recording(rec)

    hdr, payload = sa.sdriq_parse(open(rec, "rb").read())   # FileRecord::readHeader + the samples behind it
    assert hdr.sample_rate == FS and hdr.sample_size == 16

    fifo = sa.SampleSinkFifo(FS // 4)
    bank = sa.ChannelizerBank(FS, REQ_RATES, CARRIERS)
    datv = sa.DatvBank(demod_cfgs(bank))

    cost = [[] for _ in CARRIERS]
    symbol = [[] for _ in CARRIERS]
    meas = [[] for _ in CARRIERS]
    block = 2 * 100_000                                     # int16 per "FileSourceThread tick"
    for pos in range(0, payload.size, block):
        fifo.write(payload[pos: pos + block])
        while fifo.fill:                                    # DSPDeviceSourceEngine::work: drain, feed the sinks
            bank.feed(fifo.read(fifo.fill))
            datv.feed_bank(bank)                            # ordered on the device against the bank's stream
            for c in range(len(CARRIERS)):
                bank.skip(c)
                k, s = datv.read(c)
                cost[c].append(k); symbol[c].append(s); meas[c].append(datv.meas(c))
    out = {"recording": rec, "files": [], "meas": [], "symbols": []}
    for c, fc in enumerate(CARRIERS):
        k, s, m = np.concatenate(cost[c]), np.concatenate(symbol[c]), np.concatenate(meas[c])
        paths = [os.path.join(out_dir, f"datv_ch{c}_{what}.npy") for what in ("cost", "symbol", "meas")]
        for p, a in zip(paths, (k, s, m)):
            np.save(p, a)
        out["files"].append(paths); out["meas"].append(m); out["symbols"].append(s.size)
        d = datv.design(c)
        print(f"carrier {c}: {fc:+8d} Hz, {SYMBOL_RATES[c]} symbols/s: {s.size} soft symbols, {m.size} measurements (one per {d.meas_decimation} samples)")
        print("    MER over time (dB): " + " ".join(f"{v:.1f}" for v in m["mer"]))
        print("    frequency (cycles per sample): " + " ".join(f"{v:+.5f}" for v in m["freq"][-4:]))
    print(f"{n} input samples replayed from {rec}")
    return out


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "examples_out")
