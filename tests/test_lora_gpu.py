"""GPU: the LoRa demodulator bank (sdrx_lora_*) against the reference's recording (tests/golden/lora_golden.npz, made by
tests/golden/make_golden_lora.py): for every case and every feed the Samples, the lines dumpRaw printed and the state (m_tune,
m_time, m_result, m_bin, m_count, lines so far), and the design products, all exact -- int16 out, and the float path is one
compiler's strict IEEE on both sides.  Channels of different configurations and feed lengths in one handle, device pointers, the
hand-over from a channelizer bank, reset, feeds queued without a sync between them, and a text buffer that is too small."""
import os

import numpy as np
import pytest

import sdrangel_amd as sa
from tests import lora_cases as lc

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
STATE = ("tune", "time", "result", "bin", "count", "lines")


@pytest.fixture(scope="module")
def gold():
    """the recording, loaded once and left unchanged; the inputs are checked against it where they are used"""
    g = np.load(os.path.join(GOLDEN, "lora_golden.npz"))
    return {k: g[k] for k in g.files}


def gcfg(cfg) -> sa.LoraCfg:
    return sa.LoraCfg(in_rate=int(cfg[0]), nco_freq=int(cfg[1]), bandwidth=int(cfg[2]))


def want_feeds(gold, name):
    """per feed: (Samples [n, 2], text)"""
    counts, nb = gold[name + "/counts"], gold[name + "/text_bytes"]
    samples = np.split(gold[name + "/samples"].reshape(-1, 2), np.cumsum(counts)[:-1])
    text = bytes(gold[name + "/text"]).decode("latin-1")
    ends = np.cumsum(nb)
    return [(s, text[int(e - b):int(e)]) for s, b, e in zip(samples, nb, ends)]


def state_of(bank, ch):
    st = bank.state(ch)
    return [getattr(st, k) for k in STATE]


def case_inputs(gold, case):
    x = lc.inputs(case)
    assert lc.sha(x) == str(gold[case["name"] + "/in_sha256"]), case["name"]
    return x


def check_feed(bank, ch, gold, name, i, want, what):
    got = bank.read(ch)
    assert got.shape == want[0].shape, (what, got.shape, want[0].shape)
    assert np.array_equal(got, want[0]), (what, int(np.count_nonzero((got != want[0]).any(axis=1))), int(np.flatnonzero((got != want[0]).any(axis=1))[0]))
    assert bank.read_text(ch) == want[1], (what, bank.read_text(ch), want[1])
    assert state_of(bank, ch) == [int(v) for v in gold[name + "/state"][i]], (what, state_of(bank, ch), gold[name + "/state"][i])


@pytest.mark.parametrize("case", lc.CASES, ids=[c["name"] for c in lc.CASES])
def test_case_bit_exact(gold, case):
    """Samples, lines and state after every feed of the case's own cuts"""
    x = case_inputs(gold, case)
    bank = sa.LoraDemodBank([gcfg(case["cfg"])])
    want = want_feeds(gold, case["name"])
    for i, part in enumerate(lc.cut(x, case["splits"])):
        bank.feed([part])
        check_feed(bank, 0, gold, case["name"], i, want[i], f"{case['name']} feed {i}")


def test_design_equals_the_recorder(gold):
    for case in lc.CASES[:5]:                       # the five bandwidths
        nt, taps, inc, vrot, k2, chirp, sample = sa.LoraDemodBank([gcfg(case["cfg"])]).design(0)
        assert nt == int(gold[case["name"] + "/ntaps"])
        for got, want in ((taps, gold[case["name"] + "/taps"]), (vrot, gold["design/vrot"]), (np.float32([k2]), gold["design/k2"]), (chirp, gold["design/chirp"])):
            assert got.size == want.size and np.array_equal(got.view(np.uint32), want.view(np.uint32)), case["name"]
        assert np.array_equal(sample, gold["design/sample"])


def test_the_cutoff_reaches_the_design_as_a_double(gold):
    """float(7813) / 1.9 has no float representation: taps designed from the rounded value differ from the recorder's, so this
    fails if the cutoff passes through a float anywhere.  The back-end's own float field shows what that would give."""
    case = lc.BY["bw7813_step1"]
    _, taps, _, _, _, _, _ = sa.LoraDemodBank([gcfg(case["cfg"])]).design(0)
    want = gold[case["name"] + "/taps"]
    assert np.array_equal(taps.view(np.uint32), want.view(np.uint32))
    through_float = float(np.float32(float(np.float32(7813)) / 1.9))
    be = sa.BackendBank([sa.BackendCfg(in_rate=7813, out_rate=7813, nco_freq=0, interp_cutoff=through_float, taps_per_phase=4.5)])
    rounded = be.design(0)[1]
    assert rounded.size == want.size and not np.array_equal(rounded.view(np.uint32), want.view(np.uint32))


def test_channels_of_different_configurations_and_lengths_in_one_handle(gold):
    """four channels, four bandwidths, feeds of different lengths in the same call, one of them always empty; a fifth gets nothing
    in the first call and its whole stream in the second"""
    names = ["bw7813_step1", "bw31250_frac", "bw20833_nco", "silence", "short_close"]
    cases = [lc.BY[n] for n in names]
    xs = [case_inputs(gold, c) for c in cases]
    bank = sa.LoraDemodBank([gcfg(c["cfg"]) for c in cases])
    cuts = [[4000, c["n"] - 4000] if i != 3 else [0, c["n"]] for i, c in enumerate(cases)]
    got = [[] for _ in cases]
    texts = ["" for _ in cases]
    for k in range(2):
        bank.feed([lc.cut(x, s)[k] for x, s in zip(xs, cuts)])
        for i in range(len(cases)):
            got[i].append(bank.read(i))
            texts[i] += bank.read_text(i)
    assert bank.read(3).shape[0] > 0 and got[3][0].shape[0] == 0
    for i, c in enumerate(cases):
        name = c["name"]
        assert np.array_equal(np.concatenate(got[i]), gold[name + "/samples"].reshape(-1, 2)), name
        assert texts[i] == bytes(gold[name + "/text"]).decode("latin-1"), name
        assert state_of(bank, i) == [int(v) for v in gold[name + "/state"][-1]], name


def test_feed_dev_and_queued_feeds_without_a_sync(gold):
    """device pointers; two feeds queued back to back with no sync between them: the second feed's Samples, its line and the state
    behind both equal the recording"""
    torch = pytest.importorskip("torch")
    case = lc.BY["feed_edges"]
    x = case_inputs(gold, case)
    half = 2 * 5000
    a = torch.from_numpy(x[:half].copy()).cuda()
    b = torch.from_numpy(x[half:].copy()).cuda()
    torch.cuda.synchronize()
    bank = sa.LoraDemodBank([gcfg(case["cfg"])])
    bank.feed_dev([a.data_ptr()], [a.numel() // 2])
    bank.feed_dev([b.data_ptr()], [b.numel() // 2])
    bank.sync()
    second = bank.read(0)
    want = gold[case["name"] + "/samples"].reshape(-1, 2)
    assert np.array_equal(second, want[want.shape[0] - second.shape[0]:])
    assert state_of(bank, 0) == [int(v) for v in gold[case["name"] + "/state"][-1]]
    assert bank.read_text(0) == bytes(gold[case["name"] + "/text"]).decode("latin-1")      # the line ends in the second half


def test_feed_bank_behind_a_channelizer_bank(gold):
    """the hand-over on the device equals feeding what the channelizer bank's read() returns"""
    rng = np.random.default_rng(5)
    rate = 4 * 62500
    x = rng.integers(-3000, 3000, 2 * 40000).astype(np.int16)
    chan = sa.ChannelizerBank(rate, [62500, 62500], [0, 31250])
    cfgs = [sa.LoraCfg(in_rate=62500, nco_freq=0, bandwidth=62500), sa.LoraCfg(in_rate=62500, nco_freq=-1000, bandwidth=31250)]
    on_dev, on_host = sa.LoraDemodBank(cfgs), sa.LoraDemodBank(cfgs)
    for part in (x[:30000], x[30000:]):
        chan.feed(part)
        on_dev.feed_bank(chan)
        on_host.feed([chan.read(0), chan.read(1)])
        for c in range(2):
            assert on_dev.read(c).shape[0] > 1000 and np.array_equal(on_dev.read(c), on_host.read(c))
            assert state_of(on_dev, c) == state_of(on_host, c)


def test_reset_gives_a_fresh_stream(gold):
    case = lc.BY["trace"]
    x = case_inputs(gold, case)
    bank = sa.LoraDemodBank([gcfg(case["cfg"])])
    bank.feed([x[: 2 * 3001]])
    bank.reset()
    assert state_of(bank, 0) == [0, 0, 0, 0, 0, 0]
    bank.feed([x])
    assert np.array_equal(bank.read(0), gold["trace/samples"].reshape(-1, 2))
    assert bank.read_text(0) == bytes(gold["trace/text"]).decode("latin-1") != ""
    assert state_of(bank, 0) == [int(v) for v in gold["trace/state"][-1]]


def test_read_text_with_a_buffer_that_is_too_small(gold):
    case = lc.BY["trace"]
    bank = sa.LoraDemodBank([gcfg(case["cfg"])])
    bank.feed([case_inputs(gold, case)])
    text = bytes(gold["trace/text"]).decode("latin-1")
    assert len(text) > 2
    with pytest.raises(sa.SdrxError, match="too small"):
        bank.read_text(0, cap=len(text) - 1)
    assert bank.read_text(0, cap=len(text)) == text
    with pytest.raises(sa.SdrxError):
        bank.read_text(1)
