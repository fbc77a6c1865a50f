"""GPU: the ATV demodulator bank (sdrx_atv_*) against tests/atv_oracle.cpp, the scalar restatement of ATVDemod::feed that
tests/test_atv_oracle.py ties to the recording: for every case of tests/atv_cases.py and every feed the render events, the stored
frames, the screen, the scope stream and the state's words, all exact -- bytes, int16, counts, indices and bit patterns; there is
no tolerance.  The same stream in one feed and cut at awkward places; feeds with no event, exactly frames_cap and more; banks of
1, 3 and 65 channels of mixed configurations and lengths; arena growth; reset; feeds queued without a sync; device pointers; the
hand-over from a channelizer bank."""
import numpy as np
import pytest
import torch

import sdrangel_amd as sa
from tests import atv_cases as ac

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def oracle():
    return ac.build_oracle()


@pytest.fixture(scope="module")
def gold():
    g = np.load(ac.GOLDEN)
    return {k: g[k] for k in g.files}


@pytest.fixture(scope="module")
def runs(oracle):
    """every case through the oracle with its own cuts, once, and left unchanged"""
    return {c["name"]: ac.run_oracle(oracle, c) for c in ac.CASES}


def gcfg(k: dict) -> sa.AtvCfg:
    return ac.as_struct(k, sa.AtvCfg)


def got_feed(bank, ch: int) -> dict:
    stored, ne = bank.frames(ch)
    return {"events": bank.events(ch), "frames": [bank.frame(ch, i) for i in range(stored)], "screen": bank.screen(ch), "scope": bank.read(ch),
            "state": ac.state_words(bank.state(ch)), "n_events": ne}


def assert_feed(got: dict, want: dict, what, frames_cap: int):
    assert got["n_events"] == want["events"].size, (what, got["n_events"], want["events"].size)
    assert np.array_equal(got["events"], want["events"]), (what, got["events"][:8], want["events"][:8])
    assert len(got["frames"]) == len(want["frames"]) == min(want["events"].size, frames_cap), what
    for i, (g, w) in enumerate(zip(got["frames"], want["frames"])):
        assert g.shape == w.shape and np.array_equal(g, w), (what, "frame", i, int(np.count_nonzero(g != w)))
    assert np.array_equal(got["screen"], want["screen"]), (what, "screen", int(np.count_nonzero(got["screen"] != want["screen"])))
    assert got["scope"].shape == want["scope"].shape and np.array_equal(got["scope"], want["scope"]), (
        what, "scope", int(np.flatnonzero(got["scope"] != want["scope"])[0]) if got["scope"].shape == want["scope"].shape else got["scope"].shape)
    assert got["state"] == want["state"], (what, "state", got["state"], want["state"])


@pytest.mark.parametrize("case", ac.CASES, ids=[c["name"] for c in ac.CASES])
def test_case_bit_exact(runs, gold, case):
    """events, frames, screen, scope and state after every feed of the case's own cuts; the design integers against the recording"""
    bank = sa.ATVBank([gcfg(case["cfg"])])
    assert ac.design_words(bank.design(0)) == runs[case["name"]]["design"] == gold[case["name"] + "/design"].tolist()
    for i, part in enumerate(ac.cut(ac.inputs(case), case["splits"])):
        bank.feed([part])
        assert_feed(got_feed(bank, 0), runs[case["name"]]["feeds"][i], f"{case['name']} feed {i}", case["cfg"]["frames_cap"])


@pytest.mark.parametrize("name", ["decim_fm1", "decim_am_hskip", "fft_am", "fft_fm1", "decim_fft_fm3", "fm1_classic"])
def test_taps_and_filter_spectra_equal_the_oracles_as_bits(oracle, name):
    """the decimator's phase-0 row (72 taps) and create_asym_filter's two spectra; nothing where the stage is off"""
    k = ac.BY_NAME[name]["cfg"]
    o = ac.OracleAtv(oracle, k)
    want = o.filters()
    o.close()
    got = sa.ATVBank([gcfg(k)]).filters(0)
    assert want[0].size == (72 if k["decimator_enable"] else 0) and want[1].size == (4096 if k["fft_filtering"] else 0)
    for g, w in zip(got, want):
        assert g.size == w.size and np.array_equal(g.view(np.uint32), w.view(np.uint32)), name


def test_the_cases_reach_every_branch(runs):
    ac.assert_coverage([r["hits"] for r in runs.values()])


SPLIT_CASES = ("fm2_classic", "am_classic", "fm1_hskip", "short_interleaved")


@pytest.mark.parametrize("name", SPLIT_CASES)
def test_one_feed_equals_the_same_stream_cut(oracle, name):
    """cut at 1, N - 1, N and N + 1 samples of a line, mid-frame, and with the whole stream at 64k +- 1 behind a first sample:
    events re-based, scope, screen and state as the oracle fed whole"""
    case = ac.BY_NAME[name]
    n, spl = case["n"], ac.SMALL_SPL
    x = ac.inputs(case)
    whole = ac.run_oracle(oracle, case, splits=[n])["feeds"][0]
    for splits in ([1, spl - 2, 1, 1, 1, n - spl - 2], [n // 2 + 17, n - n // 2 - 17], [n - 1, 1]):
        bank = sa.ATVBank([gcfg(dict(case["cfg"], frames_cap=64))])
        feeds = []
        for part in ac.cut(x, splits):
            bank.feed([part])
            feeds.append(got_feed(bank, 0))
        m = ac.merged(feeds, splits)
        assert np.array_equal(m["events"], whole["events"]), (name, splits)
        assert np.array_equal(m["scope"], whole["scope"]) and np.array_equal(m["screen"], whole["screen"]) and m["state"] == whole["state"], (name, splits)


@pytest.mark.parametrize("first", [65535, 65536, 65537])
def test_cuts_at_64k(oracle, first):
    """a stream of 64k + 700 samples cut at 64k - 1, 64k and 64k + 1"""
    case = dict(ac.BY_NAME["fm1_classic"], n=65536 + 700)
    x = ac.inputs(case)
    splits = [first, case["n"] - first]
    want = ac.run_oracle(oracle, case, splits=splits)["feeds"]
    bank = sa.ATVBank([gcfg(case["cfg"])])
    for i, part in enumerate(ac.cut(x, splits)):
        bank.feed([part])
        assert_feed(got_feed(bank, 0), want[i], f"cut at {first} feed {i}", case["cfg"]["frames_cap"])


def test_feeds_with_no_event_with_frames_cap_and_with_more(oracle):
    """the stream cut so that a feed renders nothing, exactly frames_cap times and more often; frames beyond the cap are counted
    and listed but not stored, and asking for one is an error"""
    case = ac.BY_NAME["one_feed"]
    x = ac.inputs(case)
    ev = ac.run_oracle(oracle, case)["feeds"][0]["events"]
    assert ev.size >= 5
    cap = 2
    splits = [int(ev[0]), int(ev[1]) + 1 - int(ev[0]), case["n"] - int(ev[1]) - 1]       # none, two, the rest (three or more)
    k = dict(case["cfg"], frames_cap=cap)
    want = ac.run_spans(oracle, k, ac.cut(x, splits))["feeds"]
    assert [w["events"].size for w in want][:2] == [0, cap] and want[2]["events"].size > cap
    bank = sa.ATVBank([gcfg(k)])
    for i, part in enumerate(ac.cut(x, splits)):
        bank.feed([part])
        assert_feed(got_feed(bank, 0), want[i], f"feed {i}", cap)
    assert bank.frames(0) == (cap, want[2]["events"].size)
    with pytest.raises(sa.SdrxError, match="no such stored frame"):
        bank.frame(0, cap)


@pytest.mark.parametrize("n_ch", [1, 3, 65])
def test_banks_of_mixed_configurations_and_lengths(runs, oracle, n_ch):
    """channel i runs case i (cycled) cut in two at a place of its own; one channel gets nothing in the first call"""
    cases = [ac.CASES[(7 * i) % len(ac.CASES)] for i in range(n_ch)]
    cuts = [[0, c["n"]] if i == 1 else [(c["n"] * (3 + i % 5)) // 9, c["n"] - (c["n"] * (3 + i % 5)) // 9] for i, c in enumerate(cases)]
    xs = [ac.inputs(c) for c in cases]
    want = {}
    for c, s in zip(cases, cuts):
        if (c["name"], tuple(s)) not in want:
            want[(c["name"], tuple(s))] = ac.run_oracle(oracle, c, splits=s)["feeds"]
    bank = sa.ATVBank([gcfg(c["cfg"]) for c in cases])
    for k in range(2):
        bank.feed([ac.cut(x, s)[k] for x, s in zip(xs, cuts)])
        for i, c in enumerate(cases):
            assert_feed(got_feed(bank, i), want[(c["name"], tuple(cuts[i]))][k], f"channel {i} {c['name']} feed {k}", c["cfg"]["frames_cap"])


def test_arena_growth_short_feed_then_one_16_times_longer(oracle):
    case = dict(ac.BY_NAME["am_classic"], n=17 * 4000)
    splits = [4000, 16 * 4000]
    want = ac.run_oracle(oracle, case, splits=splits)["feeds"]
    bank = sa.ATVBank([gcfg(case["cfg"])])
    for i, part in enumerate(ac.cut(ac.inputs(case), splits)):
        bank.feed([part])
        assert_feed(got_feed(bank, 0), want[i], f"feed {i}", case["cfg"]["frames_cap"])


def test_reset_gives_a_fresh_stream(runs, oracle):
    case = ac.BY_NAME["fm2_classic"]
    x = ac.inputs(case)
    bank = sa.ATVBank([gcfg(case["cfg"])])
    fresh = ac.state_words(bank.state(0))
    bank.feed([x[: 2 * 7001]])
    assert bank.screen(0).any()
    bank.reset()
    assert ac.state_words(bank.state(0)) == fresh and not bank.screen(0).any()
    want = ac.run_oracle(oracle, case, splits=[case["n"]])["feeds"][0]
    bank.feed([x])
    assert_feed(got_feed(bank, 0), want, "after reset", case["cfg"]["frames_cap"])


def test_feed_dev_and_queued_feeds_without_a_sync(oracle):
    """device pointers; two feeds queued back to back with no sync between them: the second feed's outputs and the state behind both"""
    case = ac.BY_NAME["am_hskip"]
    x = ac.inputs(case)
    half = case["n"] // 2 + 31
    want = ac.run_oracle(oracle, case, splits=[half, case["n"] - half])["feeds"][1]
    a = torch.from_numpy(x[: 2 * half].copy()).cuda()
    b = torch.from_numpy(x[2 * half:].copy()).cuda()
    torch.cuda.synchronize()
    bank = sa.ATVBank([gcfg(case["cfg"])])
    bank.feed_dev([a.data_ptr()], [a.numel() // 2])
    bank.feed_dev([b.data_ptr()], [b.numel() // 2])
    bank.sync()
    assert_feed(got_feed(bank, 0), want, "second queued feed", case["cfg"]["frames_cap"])
    p, n = bank.last_dev(0)
    assert p and n == case["n"] - half
    p, stored, pitch = bank.frames_last_dev(0)
    d = bank.design(0)
    assert p and stored == len(want["frames"]) and pitch >= d.rows * d.cols
    assert bank.screen_last_dev(0)[1:] == (d.rows, d.cols)


def test_feed_bank_behind_a_channelizer_bank():
    """the hand-over on the device equals feeding what the channelizer bank's read() returns"""
    rng = np.random.default_rng(11)
    rate = 4 * ac.SMALL_RATE
    x = rng.integers(-9000, 9000, 2 * 60000).astype(np.int16)
    chan = sa.ChannelizerBank(rate, [ac.SMALL_RATE, ac.SMALL_RATE], [0, 80000])
    cfgs = [gcfg(ac.cfg(modulation=ac.FM1, vsync=0)), gcfg(ac.cfg(modulation=ac.AM, nco_freq=-7000, standard=ac.HSKIP))]
    on_dev, on_host = sa.ATVBank(cfgs), sa.ATVBank(cfgs)
    for part in (x[:50000], x[50000:]):
        chan.feed(part)
        on_dev.feed_bank(chan)
        on_host.feed([chan.read(0), chan.read(1)])
        for c in range(2):
            a, b = got_feed(on_dev, c), got_feed(on_host, c)
            assert a["scope"].size > 1000
            assert_feed(a, b, f"channel {c}", 4)
