"""GPU: the stretch walk of the ATV bank (atv_fast_stretch in sdrangel_amd/csrc/atv_kernels.hpp) at the line shapes the cases of
tests/test_atv_gpu.py do not have, against tests/atv_oracle.cpp, which tests/test_atv_oracle.py ties to the reference at these very
cases (tests/golden/atv_random_golden.npz).  Everything is exact, as there: events, stored frames, screen, scope stream and the
state's 28 words after every feed.

The shape cases (atv_cases.SHAPE_CASES): lines of 9 to 1000 samples against the 64-sample window, tops of 0 to 130 samples (from 64
on a detection needs the count carried over two or more stretches), the tie of the running sum with the vsync level, lost sync that
puts the column under 0 or past the line, NaN sums, noise under tops of 1 and 2, and 700 lines of PAL-625 at 10 MS/s.

Every cut: the 64-sample windows start at a feed's first sample, so a stream cut elsewhere is walked in other stretches.  For four
short streams a bank of 131 channels of one configuration, channel i fed the first i samples and then the rest; then every channel
pieces of 1, 7, 8, 9, 63, 64 and 65 samples, on both sides of the span of 8 from which the stretch is tried.  Each channel's feeds
equal the oracle fed the same spans, and merged they equal the oracle fed whole.

One shape case each through arena growth, reset, two feed_dev calls queued without a sync, and feed_bank behind a ChannelizerBank."""
import functools

import numpy as np
import pytest
import torch

import sdrangel_amd as sa
from tests import atv_cases as ac
from tests.test_atv_gpu import assert_feed, gcfg, got_feed

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def oracle():
    return ac.build_oracle()


@functools.lru_cache(maxsize=None)
def expected() -> dict:
    """every shape case through the oracle with its own cuts, once, and left unchanged"""
    return {c["name"]: ac.run_oracle(oracle(), c) for c in ac.SHAPE_CASES}


@functools.lru_cache(maxsize=None)
def gold() -> dict:
    return ac.load_random_golden()


@pytest.mark.parametrize("case", ac.SHAPE_CASES, ids=[c["name"] for c in ac.SHAPE_CASES])
def test_shape_case_bit_exact(case):
    """events, frames, screen, scope and state after every feed of the case's own cuts; the design integers against the recording"""
    want = expected()[case["name"]]
    bank = sa.ATVBank([gcfg(case["cfg"])])
    assert ac.design_words(bank.design(0)) == want["design"] == gold()[case["name"]]["design"].tolist()
    for i, part in enumerate(ac.cut(ac.inputs(case), case["splits"])):
        bank.feed([part])
        assert_feed(got_feed(bank, 0), want["feeds"][i], f"{case['name']} feed {i}", case["cfg"]["frames_cap"])


def test_the_shape_cases_reach_the_geometry():
    ac.assert_geo_coverage([expected()[c["name"]]["geo"] for c in ac.SHAPE_CASES if ac.is_fm_classic(c["cfg"])])


@pytest.mark.parametrize("case", ac.CUT_STREAMS, ids=[c["name"] for c in ac.CUT_STREAMS])
def test_every_cut(case):
    x = ac.inputs(case)
    cap = case["cfg"]["frames_cap"]
    whole = ac.run_oracle(oracle(), case, splits=[case["n"]])["feeds"][0]
    spans = [ac.cut_spans(case, i) for i in range(ac.CUT_CHANNELS)]
    wants = [ac.run_spans(oracle(), case["cfg"], ac.cut(x, s))["feeds"] for s in spans]
    parts = [ac.cut(x, s) for s in spans]
    bank = sa.ATVBank([gcfg(case["cfg"])] * ac.CUT_CHANNELS)
    got = [[] for _ in spans]
    for r in range(len(spans[0])):
        bank.feed([p[r] for p in parts])
        for i in range(ac.CUT_CHANNELS):
            got[i].append(got_feed(bank, i))
            assert_feed(got[i][r], wants[i][r], f"{case['name']} cut at {i} feed {r}", cap)
    for i, s in enumerate(spans):
        m = ac.merged(got[i], s)
        assert np.array_equal(m["events"], whole["events"]) and np.array_equal(m["scope"], whole["scope"]), (case["name"], i)
        assert np.array_equal(m["screen"], whole["screen"]) and m["state"] == whole["state"], (case["name"], i)


# ---------------------------------------------------------------- the bank's other ways in, one shape case each
def test_arena_growth_at_a_long_line():
    """1000 samples per line and 130 per top: a feed of 700 samples, then one 60 times longer"""
    case = ac.SHAPE_BY_NAME["shape_1000_130_fm2"]
    splits = [700, 42000, case["n"] - 42700]
    want = ac.run_oracle(oracle(), case, splits=splits)["feeds"]
    assert sum(w["events"].size for w in want) >= 3
    bank = sa.ATVBank([gcfg(case["cfg"])])
    for i, part in enumerate(ac.cut(ac.inputs(case), splits)):
        bank.feed([part])
        assert_feed(got_feed(bank, 0), want[i], f"feed {i}", case["cfg"]["frames_cap"])


def test_reset_gives_a_fresh_stream_at_a_carried_count():
    """reset in the middle of a top of 64 samples, the count carried: the stream fed again is as from a new bank"""
    case = ac.SHAPE_BY_NAME["shape_192_64_fm3"]
    x = ac.inputs(case)
    bank = sa.ATVBank([gcfg(case["cfg"])])
    fresh = ac.state_words(bank.state(0))
    bank.feed([x[: 2 * (192 * 20 + 40)]])
    assert bank.state(0).synchro_points > 0 and bank.screen(0).any()
    bank.reset()
    assert ac.state_words(bank.state(0)) == fresh and not bank.screen(0).any()
    want = ac.run_oracle(oracle(), case, splits=[case["n"]])["feeds"][0]
    bank.feed([x])
    assert_feed(got_feed(bank, 0), want, "after reset", case["cfg"]["frames_cap"])


def test_queued_feed_dev_calls_across_a_long_top():
    """192 / 70: two feed_dev calls with no sync between them, cut 30 samples into a top: the second feed's outputs and the state"""
    case = ac.SHAPE_BY_NAME["shape_192_70_fm3"]
    x = ac.inputs(case)
    first = 192 * 18 + 30
    want = ac.run_oracle(oracle(), case, splits=[first, case["n"] - first])
    assert want["geo"]["points_from_far"] >= 1 and want["feeds"][1]["events"].size >= 1
    a = torch.from_numpy(x[: 2 * first].copy()).cuda()
    b = torch.from_numpy(x[2 * first:].copy()).cuda()
    torch.cuda.synchronize()
    bank = sa.ATVBank([gcfg(case["cfg"])])
    bank.feed_dev([a.data_ptr()], [a.numel() // 2])
    bank.feed_dev([b.data_ptr()], [b.numel() // 2])
    bank.sync()
    assert_feed(got_feed(bank, 0), want["feeds"][1], "second queued feed", case["cfg"]["frames_cap"])


def test_feed_bank_behind_a_channelizer_bank_at_65_2():
    """the configuration of shape_noise_65_2 behind a ChannelizerBank that takes noise down by four: the hand-over on the device,
    feeding what read() returns, and the oracle fed the same, feed by feed"""
    rate = 160000
    k = dict(ac.SHAPE_BY_NAME["shape_noise_65_2"]["cfg"], in_rate=rate, line_duration=65.25 / rate, top_duration=2.25 / rate)
    x = np.random.default_rng(12).integers(-9000, 9000, 2 * 48000).astype(np.int16)
    chan = sa.ChannelizerBank(4 * rate, [rate], [0])
    on_dev, on_host = sa.ATVBank([gcfg(k)]), sa.ATVBank([gcfg(k)])
    o = ac.OracleAtv(oracle(), k)
    assert ac.design_words(on_dev.design(0)) == ac.design_words(o.design) and o.design.samples_per_line == 65 and o.design.samples_per_top == 2
    events = 0
    for i, part in enumerate((x[:50002], x[50002:])):
        chan.feed(part)
        on_dev.feed_bank(chan)
        given = chan.read(0)
        on_host.feed([given])
        want = o.feed(given)
        events += want["events"].size
        assert_feed(got_feed(on_dev, 0), want, f"device path feed {i}", k["frames_cap"])
        assert_feed(got_feed(on_host, 0), want, f"host path feed {i}", k["frames_cap"])
    assert events >= 2 and o.geo()["detect_twice_near"] >= 1 and o.hits()["hcorr_classic"] >= 1
    o.close()
