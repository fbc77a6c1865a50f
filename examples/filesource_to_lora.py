#!/usr/bin/env python3
"""LoRa receive path with the pieces of libsdrx.so, shaped like an SDRangel FileSource device set with LoRa demodulators:

    .sdriq file (FileRecord header + int16 I/Q)  ->  SampleSinkFifo  ->  engine drain loop
        ->  DownChannelizer bank, one channel per carrier
        ->  (device hand-over, no host round trip)  LoRa demodulator bank: NCO -> Interpolator at the bandwidth -> dechirp ->
            two sliding FFTs -> detect / synch -> the lines dumpRaw prints, and the Samples of the spectrum sink
        ->  the lines on stdout, one .npy of Samples per carrier

    python examples/filesource_to_lora.py [out_dir]        # writes a synthetic recording, replays it, prints the lines

Everything numeric runs on the MI355X through the C ABI (include/sdrx.h); this script is host glue only."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sdrangel_amd as sa  # noqa: E402

FS = 500_000
CARRIERS = [-125_000, 93_750]                               # offsets from the centre frequency
BANDWIDTHS = [31250, 15625]                                 # m_Bandwidth per carrier
REQ_RATES = [62500, 31250]                                  # what each demodulator asks its channelizer for


def chirp_frame(n, bw, data, rot):
    """a LoRa-like frame of bandwidth bw at FS: eight up-chirps, data symbols 4 k, three down-chirps (tests/lora_cases.py has the
    same signal with its reasoning)"""
    tau = np.arange(n, dtype=np.float64) * (bw / FS)
    s = np.array([0] * 8 + [4 * k for k in data] + [0] * 3, np.float64)
    sign = np.array([1] * (8 + len(data)) + [-1] * 3, np.float64)
    length = 256.0 * s.size
    inside = tau < length
    u = np.mod(tau[inside] + rot, length)
    k = np.minimum((u // 256.0).astype(np.int64), s.size - 1)
    t, sk = u - 256.0 * k, s[k]
    ph = ((t + 1.0) * (t + 2.0) / 2.0 + sk * t) / 256.0
    tw, tw2 = np.ceil(126.5 - sk), np.ceil(382.5 - sk)
    ph = ph - np.where(t >= tw, t - tw, 0.0) - np.where(t >= tw2, t - tw2, 0.0)
    z = np.zeros(n, np.complex128)
    z[inside] = np.exp(2j * np.pi * ph * sign[k])
    return z


def synth_recording(path, signal=None):
    """one frame per carrier plus noise, as a .sdriq file; `signal`: complex samples at FS to use instead"""
    if signal is None:
        rng = np.random.default_rng(4)
        n = int(FS * (8 + 24 + 3 + 2) * 256 / min(BANDWIDTHS))
        t = np.arange(n) / FS
        signal = np.zeros(n, np.complex128)
        for i, (fc, bw) in enumerate(zip(CARRIERS, BANDWIDTHS)):
            signal += 3000.0 * chirp_frame(n, bw, rng.integers(0, 64, 24).tolist(), 60 + 30 * i) * np.exp(2j * np.pi * fc * t)
        signal += rng.normal(0, 100, n) + 1j * rng.normal(0, 100, n)
    iq = np.empty(2 * signal.size, np.int16)
    iq[0::2] = np.clip(np.round(signal.real), -32768, 32767); iq[1::2] = np.clip(np.round(signal.imag), -32768, 32767)
    with open(path, "wb") as f:
        f.write(sa.sdriq_header_bytes(FS, 868_100_000, 1_700_000_000, 16))
        f.write(iq.tobytes())
    return signal.size


def demod_cfgs(bank):
    cfgs = []
    for c, bw in enumerate(BANDWIDTHS):
        _modes, out_rate, ofs = bank.info(c)
        cfgs.append(sa.LoraCfg(in_rate=out_rate, nco_freq=-ofs, bandwidth=bw))
    return cfgs


def main(out_dir, signal=None):
    os.makedirs(out_dir, exist_ok=True)
    rec = os.path.join(out_dir, "synthetic_lora.sdriq")
    n = synth_recording(rec, signal)

    hdr, payload = sa.sdriq_parse(open(rec, "rb").read())   # FileRecord::readHeader + the samples behind it
    assert hdr.sample_rate == FS and hdr.sample_size == 16

    fifo = sa.SampleSinkFifo(FS // 4)
    bank = sa.ChannelizerBank(FS, REQ_RATES, CARRIERS)
    lora = sa.LoraDemodBank(demod_cfgs(bank))

    samples = [[] for _ in CARRIERS]
    lines = [[] for _ in CARRIERS]
    spans = []
    block = 2 * 100_000                                     # int16 per "FileSourceThread tick"
    for pos in range(0, payload.size, block):
        fifo.write(payload[pos: pos + block])
        while fifo.fill:                                    # DSPDeviceSourceEngine::work: drain, feed the sinks
            span = fifo.read(fifo.fill)
            spans.append(span.size // 2)
            bank.feed(span)
            lora.feed_bank(bank)                            # ordered on the device against the bank's stream
            for c in range(len(CARRIERS)):
                bank.skip(c)
                samples[c].append(lora.read(c))
                for line in lora.read_text(c).split("\n")[:-1]:
                    lines[c].append(line)
                    print(f"carrier {c}: {line}")
    paths = []
    for c, fc in enumerate(CARRIERS):
        p = os.path.join(out_dir, f"lora_ch{c}.npy")
        np.save(p, np.concatenate(samples[c]))
        paths.append(p)
        st = lora.state(c)
        print(f"carrier {c}: {fc:+8d} Hz, bandwidth {BANDWIDTHS[c]}: {st.count} Samples, {st.lines} lines, m_tune {st.tune} -> {p}")
    print(f"{n} input samples replayed from {rec}")
    return {"recording": rec, "npy": paths, "spans": spans, "lines": lines, "state": [lora.state(c) for c in range(len(CARRIERS))]}


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "examples_out")
