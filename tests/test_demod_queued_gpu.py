"""GPU: feeds of the demodulator banks queued back to back, the way feed_dev and feed_bank are meant to be used.  Every other
GPU test reads after every feed, and read / levels / last_dev / squelch_open synchronise the handle's stream; here nothing
synchronises between the feeds of a chain, so the double-buffered histories (cur ^= 1), the pinned per-feed pointer table with
its event, the growth of the work buffers in the middle of a chain and the front-to-tail hand-over are all more than one feed
deep when the results are looked at.  Per family (wfm, am, nfm, ssb, udpsrc), three named cases whose state matters across
feeds in one three-channel handle:

  a. a feed_dev chain of ten spans over streams uploaded once;
  b. the same chain on the caller's stream, every span copied from pinned memory on that stream right before its feed;
  c. bank.feed -> feed_bank -> bank.skip over six segments of a 61.44 MS/s stream.

Only the last feed's outputs and the final state are read; the oracle (tests/<family>_oracle.c) is fed the same spans.  The
comparison rules are those of tests/test_<family>_gpu.py."""
import functools

import numpy as np
import pytest

import sdrangel_amd as sa
from tests import oracle_py as orc
from tests import synth
from tests import udpsrc_cases as uc
from tests.demod_families import FAMILIES, naming

pytestmark = pytest.mark.gpu

#: the named cases of a chain: squelch or AGC transitions, serial and dyadic schedules, both block sizes, three formats
NAMES = {
    "wfm": ("burst_48k", "burst_240k_fraccap", "nondyadic_250k"),
    "am": ("burst_bandpass", "nondyadic_62500", "zero_gap"),
    "nfm": ("burst_gate5", "nondyadic_62500", "r96k_to_44k1"),
    "ssb": ("gate", "short_history", "dsb"),
    "udpsrc": ("iq16_burst_gate1", "nfm_burst", "am_agc_squelched"),
}
#: stream lengths other than the named case's: one more turn of its burst runs, so that the last span is not all silence behind
#: a closed squelch but holds the next opening
LENGTHS = {("am", "burst_bandpass"): 125500 + 9000 + 2000 + 8000, ("nfm", "burst_gate5"): 115500 + 9000 + 2000 + 8000}
#: the shape of a chain before its last span, in parts of 15514: short spans, an empty one, a one-sample one, and one 4.5 times
#: as long as any before it -- the work buffers (a power of two, at most twice the longest feed so far) grow there
HEAD = (1300, 700, 0, 2000, 1, 900, 9000, 1100, 513)
BIG = 6
#: outputs the last span has to produce at the least: it depends on everything carried
LAST_OUT = 4096


def out_rate(fam, cfg):
    return cfg["audio_rate"] if fam.name == "ssb" else cfg[2]


def in_rate(fam, cfg):
    return cfg["in_rate"] if fam.name == "ssb" else cfg[0]


def chain_case(fam, name, ch):
    """the named case with its stream cut into ten spans: HEAD stretched over everything but the last span, the last span long
    enough for LAST_OUT + 512 outputs (a block of 1024 may be held back).  A case too short for that gets a longer stream of
    the same signal."""
    case = {c["name"]: c for c in fam.cm.CASES}[name]
    per_out = -(-in_rate(fam, case["cfg"]) // int(out_rate(fam, case["cfg"])))
    last = (LAST_OUT + 512) * per_out
    body = max(LENGTHS.get((fam.name, name), case["n"]) - last, sum(HEAD))
    scale = body / sum(HEAD)
    spans = [m if m <= 1 else int(m * scale) + 17 * ch for m in HEAD]
    if ch == 1:
        spans[2], spans[4] = spans[4], spans[2]             # the empty and the one-sample span of the channels do not all coincide
    spans[BIG] += body - sum(spans)
    assert spans[BIG] > 4096 and spans[BIG] > 4 * max(spans[:BIG]) and min(spans) == 0 and 1 in spans
    spans.append(last)
    return dict(case, n=body + last, splits=spans)


@functools.lru_cache(maxsize=None)
def chain_setup(family):
    """(cases, inputs, oracle results over the same spans) of a family's chain, computed once"""
    fam = FAMILIES[family]
    cases = [chain_case(fam, name, ch) for ch, name in enumerate(NAMES[family])]
    xs = [fam.cm.inputs(c) for c in cases]
    L = fam.cm.build_oracle()
    wants = [fam.run_spans(L, c["cfg"], fam.cm.cut(x, c["splits"])) for c, x in zip(cases, xs)]
    for x in xs:
        x.setflags(write=False)
    return cases, xs, wants, L


def offsets(case):
    return np.concatenate(([0], np.cumsum(case["splits"]))).tolist()


def run_chain(fam, cases, xs, stream=None):
    """the whole chain without a synchronising call between its feeds; returns the bank and what is alive behind it"""
    import torch
    bank = fam.Bank([fam.gcfg(c["cfg"]) for c in cases])
    offs = [offsets(c) for c in cases]
    if stream is None:
        dev = [torch.from_numpy(x.copy()).cuda() for x in xs]
        torch.cuda.synchronize()                            # once, before the first feed: the uploads are not on the handle's stream
        pinned = None
    else:
        bank.set_stream(stream.cuda_stream)
        pinned = [torch.from_numpy(x.copy()).pin_memory() for x in xs]
        with torch.cuda.stream(stream):
            dev = [torch.empty(x.size, dtype=torch.int16, device="cuda") for x in xs]
    for r in range(len(cases[0]["splits"])):
        if stream is not None:
            with torch.cuda.stream(stream):
                for d, p, o in zip(dev, pinned, offs):
                    if o[r + 1] > o[r]:
                        d[2 * o[r]: 2 * o[r + 1]].copy_(p[2 * o[r]: 2 * o[r + 1]], non_blocking=True)
        bank.feed_dev([d.data_ptr() + 4 * o[r] for d, o in zip(dev, offs)], [o[r + 1] - o[r] for o in offs])
    return bank, (dev, pinned)


def check_chain(fam, bank, cases, wants, where):
    got = [fam.read(bank, ch) for ch in range(len(cases))]
    for ch, (case, want) in enumerate(zip(cases, wants)):
        with naming(case, ch, where):
            last = fam.last_feed(want)
            rows = [v[0].shape[0] for k, v in last.items() if isinstance(v, list) and k != "masks"]
            assert max(rows) >= LAST_OUT and any(v[0].any() for k, v in last.items() if isinstance(v, list)), rows
            fam.check_feeds(case, [got[ch]], last, f"{where} channel {ch}")
            fam.check_state(bank, ch, want, f"{where} channel {ch}")
    return got


@pytest.mark.parametrize("family", list(FAMILIES))
def test_feed_dev_chain(family):
    fam = FAMILIES[family]
    cases, xs, wants, _ = chain_setup(family)
    assert all(8 <= len(c["splits"]) <= 12 for c in cases)
    bank, alive = run_chain(fam, cases, xs)
    check_chain(fam, bank, cases, wants, f"{family} feed_dev chain")
    bank.close()


@pytest.mark.parametrize("family", list(FAMILIES))
def test_feed_dev_chain_on_the_callers_stream(family):
    import torch
    fam = FAMILIES[family]
    cases, xs, wants, L = chain_setup(family)
    stream = torch.cuda.Stream()
    bank, alive = run_chain(fam, cases, xs, stream)
    got = check_chain(fam, bank, cases, wants, f"{family} chain on the caller's stream")
    own, own_alive = run_chain(fam, cases, xs)
    for ch, case in enumerate(cases):                       # the same device code on either stream: equal to the last bit
        with naming(case, ch, f"{family} caller's stream against the handle's own"):
            for g, w in zip(got[ch], fam.read(own, ch)):
                assert g.dtype == w.dtype and np.array_equal(g, w)
    own.close()
    bank.set_stream(None)
    bank.reset()
    heads = [x[: 2 * c["splits"][-1]] for c, x in zip(cases, xs)]
    bank.feed(heads)
    for ch, case in enumerate(cases):
        with naming(case, ch, f"{family} one feed after reset"):
            want = fam.run_spans(L, case["cfg"], [heads[ch]])
            fam.check_feeds(case, [fam.read(bank, ch)], want, f"{family} after reset, channel {ch}")
            fam.check_state(bank, ch, want, f"{family} after reset, channel {ch}")
    bank.close()


# ---------------------------------------------------------------- feed_bank
FS, N_CH = 61_440_000, 4
SEGMENTS = (400_001, 520_000, 450_003, 380_000, 550_000, 699_996)


def bank_cfg(family, c, rate, ofs):
    """the configurations of test_feed_bank_device_handover in tests/test_<family>_gpu.py"""
    if family == "wfm":
        return (rate, -ofs, 48000, 80000.0, 15000.0, 2.0, -60.0, 0)
    if family == "am":
        return (rate, -ofs, 48000, 5000.0, 2.0, -90.0, 0, c % 2)
    if family == "nfm":
        return (rate, -ofs, 48000, 12500.0, 3000.0, 2000, 2.0, -900.0, 1 + c % 2, 0)
    if family == "ssb":
        return FAMILIES["ssb"].cm._cfg(rate, 48000, nco_freq=-ofs, agc=1, agc_time_log2=3 + c, dsb=int(c == 3), span_log2=1 + 2 * c,
                                       rf_bandwidth=-3000.0 if c == 1 else 3000.0, low_cutoff=-300.0 if c == 1 else 300.0, audio_binaural=int(c == 2))
    return (rate, -ofs, 8000.0, (uc.IQ16, uc.AM_BPF_MONO, uc.AM_NODC_MONO, uc.IQ24)[c], 5000.0, 2500, 1.0, -90, c % 2, 1, c % 2)


@pytest.mark.parametrize("family", list(FAMILIES))
def test_feed_bank_pipeline(family):
    """bank.feed; feed_bank; bank.skip, six times over, no demodulator read before the end: every bank.feed overwrites the queues
    the demodulators were handed while up to five of their feeds may still be waiting.  WFM asks the bank for requiredBW(80000),
    the others for 48 kS/s."""
    fam = FAMILIES[family]
    req = fam.cm.required_bw(80000) if family == "wfm" else 48000
    fcs = [int(-24_000_000 + c * 13_000_000 + 1371 * c) for c in range(N_CH)]
    bank = sa.ChannelizerBank(FS, [req] * N_CH, fcs)
    cfgs, chains = [], []
    for c in range(N_CH):
        modes, rate, ofs = bank.info(c)
        assert rate >= req
        cfgs.append(bank_cfg(family, c, rate, ofs)); chains.append(orc.Chain(modes))
    demod = fam.Bank([fam.gcfg(k) for k in cfgs])
    x = synth.mix(sum(SEGMENTS), 78, 3000, 1500, 1)
    edges = np.concatenate(([0], np.cumsum(SEGMENTS))).tolist()
    segs = [x[2 * a: 2 * b] for a, b in zip(edges, edges[1:])]
    for seg in segs:
        bank.feed(seg)
        demod.feed_bank(bank)
        for c in range(N_CH):
            bank.skip(c)
    L = fam.cm.build_oracle()
    produced = 0
    for c in range(N_CH):
        case = {"cfg": cfgs[c], "segments": SEGMENTS}
        with naming(case, c, f"{family} feed_bank pipeline"):
            want = fam.run_spans(L, cfgs[c], [chains[c].feed(seg) for seg in segs])
            got = fam.read(demod, c)
            fam.check_feeds(case, [got], fam.last_feed(want), f"{family} feed_bank pipeline, channel {c}")
            fam.check_state(demod, c, want, f"{family} feed_bank pipeline, channel {c}")
            produced += got[0].shape[0]
    assert produced > 0
    demod.close(); bank.close()
