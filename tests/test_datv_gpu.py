"""GPU: the DATV receiver bank (sdrx_datv_*) against tests/datv_oracle.cpp, the scalar restatement of DATVDemod::feed down to
p_symbols that tests/test_datv_oracle.py ties to the recording: for every case of tests/datv_cases.py and every feed the soft
symbols, the constellation points, the measurements (mer included: both sides take logf from this process's libm) and the
state's words, all exact -- int16, bytes, counts and bit patterns; there is no tolerance.  The oracle runs on the very tables and
coefficients the handle built, so a libm difference on this machine shows in the design test and nowhere else.  One stream whole,
in feeds of awkward lengths and in every length from 1 to 130; banks of 1, 3, 65 and 257 channels of mixed configurations; two
constellations in one handle; reset; arena growth; feeds queued without a sync; device pointers; the hand-over from a channelizer
bank."""
import numpy as np
import pytest
import torch

import sdrangel_amd as sa
from tests import datv_cases as dc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def oracle():
    return dc.build_oracle()


@pytest.fixture(scope="module")
def gold():
    g = np.load(dc.GOLDEN)
    return {k: g[k] for k in g.files}


def gcfg(k: dict) -> sa.DatvCfg:
    return dc.as_struct(k, sa.DatvCfg)


def got_feed(bank, ch: int) -> dict:
    cost, symbol = bank.read(ch)
    return {"cost": cost, "symbol": symbol, "points": bank.points(ch).reshape(-1).view(np.uint32), "meas": bank.meas(ch).view(dc.MEAS_DTYPE),
            "state": dc.state_words(bank.state(ch))}


_TABLES = {}


def tables_of(k: dict):
    """the tables a handle builds for this configuration, fetched once per distinct design"""
    key = (k["modulation"], k["fec"], k["hard_metric"], k["sampler"], k["sample_rate"], k["symbol_rate"], k["rolloff"], k["excursion"])
    if key not in _TABLES:
        _TABLES[key] = sa.DatvBank([gcfg(k)]).tables(0)
    return _TABLES[key]


_RUNS = {}


def want_of(oracle, case: dict, splits=None) -> dict:
    """the case through the oracle on the bank's tables, once per (case, cuts), and left unchanged"""
    key = (case["name"], tuple(splits or case["splits"]))
    if key not in _RUNS:
        _RUNS[key] = dc.run_oracle(oracle, case, splits=splits, tables=tables_of(case["cfg"]))
    return _RUNS[key]


@pytest.mark.parametrize("case", dc.CASES, ids=[c["name"] for c in dc.CASES])
def test_case_bit_exact(oracle, gold, case):
    """symbols, points, measurements and state after every feed of the case's own cuts; the design words against the recording"""
    bank = sa.DatvBank([gcfg(case["cfg"])])
    want = want_of(oracle, case)
    assert dc.design_words(bank.design(0)) == want["design"]
    assert want["design"][:11] == gold[case["name"] + "/design"].tolist()
    for i, part in enumerate(dc.cut(dc.inputs(case), case["splits"])):
        bank.feed([part])
        dc.assert_same_feed(got_feed(bank, 0), want["feeds"][i], f"{case['name']} feed {i}")
    assert sum(f["cost"].size for f in want["feeds"]) > 0


DESIGN_CASES = ("rrc", "linear", "mod_bpsk", "mod_psk8", "mod_apsk16", "mod_apsk32", "mod_apsk64e", "mod_qam16", "mod_qam64", "mod_qam256",
                "hard_metric", "ratio_1p2_taps3", "ratio_8_taps63", "ratio_8_taps64", "ratio_2_taps55", "apsk16_fec910")


@pytest.mark.parametrize("name", DESIGN_CASES)
def test_tables_equal_the_recordings_and_the_oracles(oracle, gold, name):
    """the RRC coefficients, trig16, the constellation table and symbols[] as the handle built them (restated sinf, cosf and atan2f)
    against the oracle's, built with this machine's libm, and against the digests recorded from the reference's own classes"""
    k = dc.BY_NAME[name]["cfg"]
    o = dc.OracleDatv(oracle, k)
    want = o.tables()
    o.close()
    got = tables_of(k)
    for g, w, what in zip(got, want, ("coefficients", "trig16", "constellation table", "symbols")):
        assert g.size == w.size and np.array_equal(g.view(np.uint8), w.view(np.uint8)), (name, what)
    assert dc.table_digests(got) == gold[name + "/tables_sha256"].tolist()
    assert sa.DatvBank([gcfg(k)]).table_digests(0) == dc.table_digests(got)


def test_the_cases_reach_every_branch(oracle):
    dc.assert_coverage([want_of(oracle, c)["hits"] for c in dc.CASES])


def test_one_stream_whole_and_in_awkward_feeds(oracle):
    """feeds of 1, 127, 128, 129, 511, 512, 513 and 640 + readahead +- 1 (and the rest in one): one concatenated output, one state"""
    case = dc.BY_NAME["rrc"]
    x = dc.inputs(case)
    whole = dc.merged(want_of(oracle, case, splits=[case["n"]])["feeds"])
    ra = sa.DatvBank([gcfg(case["cfg"])]).design(0).readahead
    assert ra > 100
    for first in dc.cut_lengths(ra):
        for splits in ([first, case["n"] - first], dc.even_cut(case["n"], first) if first >= 127 else [first] * 5 + [case["n"] - 5 * first]):
            bank = sa.DatvBank([gcfg(case["cfg"])])
            feeds = []
            for part in dc.cut(x, splits):
                bank.feed([part])
                feeds.append(got_feed(bank, 0))
            dc.assert_same_feed(dc.merged(feeds), whole, f"feeds of {first}")


@pytest.mark.parametrize("sampler", [dc.NEAREST, dc.LINEAR, dc.RRC])
def test_every_feed_length_from_1_to_130(oracle, sampler):
    """a bank of 130 channels on one stream: channel i is fed i + 1 samples at a time"""
    case = dict(dc.CUT_STREAM, cfg=dict(dc.CUT_STREAM["cfg"], sampler=sampler), name=f"cut_stream_{sampler}")
    x = dc.inputs(case)
    n = case["n"]
    whole = dc.merged(want_of(oracle, case, splits=[n])["feeds"])
    assert whole["cost"].size > 100 and whole["meas"].size > 5
    bank = sa.DatvBank([gcfg(case["cfg"])] * dc.CUT_CHANNELS)
    parts = [dc.cut(x, dc.even_cut(n, i + 1)) for i in range(dc.CUT_CHANNELS)]
    feeds = [[] for _ in range(dc.CUT_CHANNELS)]
    quiet = np.zeros(dc.CUT_CHANNELS, np.int64)
    for r in range(n):
        live = [i for i in range(dc.CUT_CHANNELS) if r < len(parts[i])]
        if not live:
            break
        bank.feed([parts[i][r] if r < len(parts[i]) else x[:0] for i in range(dc.CUT_CHANNELS)])
        for i in live:
            # the front hands a block over when the channel's samples pass a multiple of 512, and only then can a chunk run: the
            # outputs are read after every such feed and after the last one.  A feed in between that stored something all the
            # same would show in the state's running symbol count at the next read, and in the merged output
            before, after = r * (i + 1), min((r + 1) * (i + 1), n)
            if after // 512 > before // 512 or r == len(parts[i]) - 1:
                feeds[i].append(got_feed(bank, i))
            else:
                quiet[i] += 1
    assert quiet[0] > 1200 and quiet[129] >= 6
    for i in range(dc.CUT_CHANNELS):
        dc.assert_same_feed(dc.merged(feeds[i]), whole, f"feeds of {i + 1}")
        assert sum(f["cost"].size for f in feeds[i]) == feeds[i][-1]["state"][-1], f"feeds of {i + 1}: symbols stored in a feed that was not read"


def test_feeds_of_1_to_21_samples_are_read_after_every_feed(oracle):
    """the shortest feeds, which mostly return nothing, hold samples back and rebuild shifted_coeffs from the carried freqw: 21 channels,
    channel i fed i + 1 samples at a time, every output read after every feed"""
    case = dict(dc.CUT_STREAM, n=700, name="cut_stream_short", splits=[700])
    x = dc.inputs(case)
    n = case["n"]
    whole = dc.merged(want_of(oracle, case, splits=[n])["feeds"])
    assert whole["cost"].size > 30 and whole["meas"].size >= 2
    bank = sa.DatvBank([gcfg(case["cfg"])] * 21)
    parts = [dc.cut(x, dc.even_cut(n, i + 1)) for i in range(21)]
    feeds = [[] for _ in range(21)]
    for r in range(n):
        bank.feed([parts[i][r] if r < len(parts[i]) else x[:0] for i in range(21)])
        for i in range(21):
            if r < len(parts[i]):
                feeds[i].append(got_feed(bank, i))
    for i in range(21):
        assert sum(1 for f in feeds[i] if f["cost"].size) == 1 and len(feeds[i]) == len(parts[i])
        dc.assert_same_feed(dc.merged(feeds[i]), whole, f"feeds of {i + 1}")


@pytest.mark.parametrize("n_ch", [1, 3, 65, 257])
def test_banks_of_mixed_configurations_and_lengths(oracle, n_ch):
    """channel i runs case i (cycled, the short ones) cut in two at a place of its own; one channel gets nothing in the first call"""
    short = [c for c in dc.CASES if c["n"] <= 9000]
    cases = [short[(7 * i) % len(short)] for i in range(n_ch)]
    cuts = [[0, c["n"]] if i == 1 else [(c["n"] * (3 + i % 5)) // 9, c["n"] - (c["n"] * (3 + i % 5)) // 9] for i, c in enumerate(cases)]
    xs = {c["name"]: dc.inputs(c) for c in cases}
    bank = sa.DatvBank([gcfg(c["cfg"]) for c in cases])
    if n_ch >= 65:
        assert len({(c["cfg"]["modulation"], c["cfg"]["hard_metric"]) for c in cases}) >= 3
    for k in range(2):
        bank.feed([dc.cut(xs[c["name"]], s)[k] for c, s in zip(cases, cuts)])
        for i, c in enumerate(cases):
            dc.assert_same_feed(got_feed(bank, i), want_of(oracle, c, splits=cuts[i])["feeds"][k], f"channel {i} {c['name']} feed {k}")


def test_two_constellations_in_one_handle_share_nothing(oracle):
    a, b = dc.BY_NAME["mod_qam64"], dc.BY_NAME["hard_metric"]
    bank = sa.DatvBank([gcfg(a["cfg"]), gcfg(b["cfg"]), gcfg(a["cfg"])])
    assert bank.table_digests(0)[2] != bank.table_digests(1)[2] and bank.table_digests(0) == bank.table_digests(2)
    bank.feed([dc.inputs(a), dc.inputs(b), dc.inputs(a)])
    for i, c in enumerate((a, b, a)):
        dc.assert_same_feed(got_feed(bank, i), dc.merged(want_of(oracle, c, splits=[c["n"]])["feeds"]), f"channel {i}")


def test_arena_growth_short_feed_then_one_16_times_longer(oracle):
    case = dict(dc.BY_NAME["meas_100"], n=17 * 3000, name="meas_100_long")
    splits = [3000, 16 * 3000]
    want = want_of(oracle, case, splits=splits)["feeds"]
    bank = sa.DatvBank([gcfg(case["cfg"])])
    for i, part in enumerate(dc.cut(dc.inputs(case), splits)):
        bank.feed([part])
        dc.assert_same_feed(got_feed(bank, 0), want[i], f"feed {i}")


def test_reset_gives_a_fresh_stream(oracle):
    case = dc.BY_NAME["rrc"]
    x = dc.inputs(case)
    bank = sa.DatvBank([gcfg(case["cfg"])])
    fresh = dc.state_words(bank.state(0))
    bank.feed([x[: 2 * 5001]])
    assert dc.state_words(bank.state(0)) != fresh and bank.read(0)[0].size > 0
    bank.reset()
    assert dc.state_words(bank.state(0)) == fresh
    bank.feed([x])
    dc.assert_same_feed(got_feed(bank, 0), dc.merged(want_of(oracle, case, splits=[case["n"]])["feeds"]), "after reset")


def test_feed_dev_and_queued_feeds_without_a_sync(oracle):
    """device pointers; two feeds queued back to back with no sync between them: the second feed's outputs and the state behind both"""
    case = dc.BY_NAME["drift_reset_down"]
    x = dc.inputs(case)
    half = case["n"] // 2 + 31
    want = want_of(oracle, case, splits=[half, case["n"] - half])["feeds"][1]
    a = torch.from_numpy(x[: 2 * half].copy()).cuda()
    b = torch.from_numpy(x[2 * half:].copy()).cuda()
    torch.cuda.synchronize()
    bank = sa.DatvBank([gcfg(case["cfg"])])
    bank.feed_dev([a.data_ptr()], [a.numel() // 2])
    bank.feed_dev([b.data_ptr()], [b.numel() // 2])
    bank.sync()
    dc.assert_same_feed(got_feed(bank, 0), want, "second queued feed")
    pc, ps, n = bank.last_dev(0)
    assert pc and ps and n == want["cost"].size


def test_a_feed_of_one_sample_returns_nothing(oracle):
    case = dc.BY_NAME["linear"]
    bank = sa.DatvBank([gcfg(case["cfg"])])
    bank.feed([dc.inputs(case)[:2]])
    g = got_feed(bank, 0)
    assert g["cost"].size == 0 and g["points"].size == 0 and g["meas"].size == 0 and bank.last_dev(0)[2] == 0


def test_feed_bank_behind_a_channelizer_bank():
    """the hand-over on the device equals feeding what the channelizer bank's read() returns"""
    rng = np.random.default_rng(11)
    rate = 1000000
    x = rng.integers(-9000, 9000, 2 * 60000).astype(np.int16)
    chan = sa.ChannelizerBank(4 * rate, [rate, rate], [0, 500000])
    cfgs = [gcfg(dc.cfg()), gcfg(dc.cfg(sampler=dc.LINEAR, modulation=dc.QAM16, centre_frequency=-7000))]
    on_dev, on_host = sa.DatvBank(cfgs), sa.DatvBank(cfgs)
    total = 0
    for part in (x[:50000], x[50000:]):
        chan.feed(part)
        on_dev.feed_bank(chan)
        on_host.feed([chan.read(0), chan.read(1)])
        for c in range(2):
            a, b = got_feed(on_dev, c), got_feed(on_host, c)
            total += a["cost"].size
            dc.assert_same_feed(a, b, f"channel {c}")
    assert total > 1000
