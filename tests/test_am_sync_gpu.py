"""GPU: the synchronous-AM channels of the AM demodulator bank (sdrx_am_create_ex) against the reference's recording
(tests/golden/am_sync_golden.npz, made by tests/golden/make_golden_am_sync.py): every audio sample of every feed, m_magsq, peak,
count, squelch state, getPllLocked() and getPllFrequency() after every feed bit for bit, the level sum within the bound sdrx.h
states; the design products; the once-designed SSBFilter; random splits; sixteen mixed channels in one handle, the envelope ones
against tests/golden/am_golden.npz; reset, device pointers and the hand-over from the channelizer bank."""
import hashlib
import os

import numpy as np
import pytest

import sdrangel_amd as sa
from tests import am_cases as ac
from tests import am_sync_cases as sc

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def gold():
    """the recording, loaded once and left unchanged; the inputs are checked against it where they are used"""
    g = np.load(os.path.join(GOLDEN, "am_sync_golden.npz"))
    return {k: g[k] for k in g.files}


def gcfg(cfg) -> sa.AmCfg:
    return sa.AmCfg(in_rate=int(cfg[0]), nco_freq=int(cfg[1]), audio_rate=int(cfg[2]), rf_bandwidth=float(cfg[3]), volume=float(cfg[4]),
                    squelch_db=float(cfg[5]), audio_mute=int(cfg[6]), bandpass_enable=int(cfg[7]))


def gsync(sync) -> sa.AmSyncCfg:
    return sa.AmSyncCfg(pll=int(sync[0]), sync_op=int(sync[1]), ssb_design_rate=int(sync[2]), ssb_design_bw=float(sync[3]))


def make_bank(case):
    return sa.AmDemodBank([gcfg(case["cfg"])], sync=[gsync(case["sync"])])


def want_feeds(gold, case):
    counts = gold[case["name"] + "/counts"]
    return np.split(gold[case["name"] + "/audio"], np.cumsum(counts)[:-1])


def pll_bits(bank, ch):
    locked, freq = bank.pll(ch)
    return int(locked), int(np.float32(freq).view(np.uint32))


def check_state(bank, ch, gold, case, feed, what):
    """levels, squelch and loop state after feed number `feed` of the case"""
    lv, st = gold[case["name"] + "/levels"][feed], gold[case["name"] + "/state"][feed]
    m, s, p, n = bank.levels(ch)
    assert n == int(st[0]), what
    assert m == lv[0], (what, m, lv[0])
    assert p == lv[2], what
    assert bank.squelch_open(ch) == bool(st[1]), what
    # reordering n non-negative double terms moves the sum by at most n * 2^-53 relative, on either side
    assert abs(s - lv[1]) <= 2 * max(n, 1) * 2.0 ** -53 * lv[1], (what, s, lv[1])
    assert pll_bits(bank, ch) == (int(st[3]), int(st[4])), (what, bank.pll(ch), st[3:5])


def run_gpu(gold, case, splits=None, bank=None, check_each=False):
    x = sc.inputs(case)
    assert sc.sha(x) == str(gold[case["name"] + "/in_sha256"]), case["name"]
    bank = bank or make_bank(case)
    feeds = []
    for i, part in enumerate(sc.cut(x, splits or case["splits"])):
        bank.feed([part])
        feeds.append(bank.read(0))
        if check_each:
            check_state(bank, 0, gold, case, i, f"{case['name']} feed {i}")
    return bank, feeds


def assert_feeds_equal(got, want, what):
    assert [g.size for g in got] == [w.size for w in want], what
    for i, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), (what, i, int(np.count_nonzero(g != w)), int(np.flatnonzero(g != w)[0]))


@pytest.mark.parametrize("case", sc.CASES, ids=[c["name"] for c in sc.CASES])
def test_case_bit_exact(gold, case):
    """audio of every feed, and after every feed the levels, the squelch and getPllLocked / getPllFrequency"""
    bank, got = run_gpu(gold, case, check_each=True)
    assert_feeds_equal(got, want_feeds(gold, case), case["name"])
    if case["expect"].get("never_open"):
        assert not np.concatenate(got).any() and bank.pll(0) == (False, 0.0)


def test_sync_design_equals_the_recorder(gold):
    for name in ("dsb_0", "usb_0_bp", "lsb_0", "dsb_m170", "usb_design_default", "usb_design_own", "lsb_p30_bp"):
        case = sc.BY[name]
        taps, filt, coef = make_bank(case).sync_design(0)
        assert filt.size == 2 * 2 * sc.block(case["sync"][1]), name
        for got, key in ((taps, "taps"), (filt, "filter"), (coef, "coef")):
            want = gold[f"{name}/{key}"]
            assert got.size == want.size and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (name, key)


def test_ssb_filter_is_designed_once(gold):
    """USB through the filter of the constructor's defaults and through one designed from the channel's own rate and bandwidth: both
    equal their recordings (test_case_bit_exact) and differ from each other, in the filter and in the audio"""
    a, b = sc.BY["usb_design_default"], sc.BY["usb_design_own"]
    assert a["cfg"] == b["cfg"] and a["sig"] == b["sig"] and a["sync"] != b["sync"]
    (bank_a, got_a), (bank_b, got_b) = run_gpu(gold, a, splits=[a["n"]]), run_gpu(gold, b, splits=[b["n"]])
    assert not np.array_equal(bank_a.sync_design(0)[1], bank_b.sync_design(0)[1])
    assert got_a[0].size == got_b[0].size and not np.array_equal(got_a[0], got_b[0])
    assert np.array_equal(got_b[0], gold["usb_design_own/audio"])


@pytest.mark.parametrize("name", ["usb_reopen", "dsb_reopen_bp", "lsb_m170", "dsb_p30_bp"])
def test_random_splits_equal_one_feed(gold, name):
    case = sc.BY[name]
    one = gold[name + "/audio"]
    B = sc.block(case["sync"][1])
    rng = np.random.default_rng(len(name) + 7)
    for trial in range(2):
        splits, left = [], case["n"]
        while left > 0:
            m = min(left, int(rng.choice([0, 1, 2, B - 1, B, B + 1, int(rng.integers(1, 300)), int(rng.integers(1, 3000)), int(rng.integers(1, 3000))])))
            splits.append(m); left -= m
        # with the squelch open nearly throughout, cuts that are no multiple of the block land inside one
        assert sum(1 for m in np.cumsum(splits) if m % B) >= 3
        bank, got = run_gpu(gold, case, splits)
        got = np.concatenate(got)
        assert got.size == one.size and np.array_equal(got, one), (name, trial, int(np.flatnonzero(got != one)[0]) if got.size == one.size else -1)
        check_state(bank, 0, gold, case, -1, f"{name} trial {trial}")


ENVELOPE = ("step1_48k", "burst_bandpass", "audio_mute", "earliest_open")


def test_sixteen_mixed_channels_in_one_handle(gold):
    """twelve sync channels (the three operations, three audio rates, Bandpass on and off) and four envelope channels in one handle:
    every new kernel runs with more than one channel row; a sync channel equals its recording, an envelope channel the envelope
    recording of tests/golden/am_golden.npz for the same configuration"""
    env_gold = np.load(os.path.join(GOLDEN, "am_golden.npz"))
    sync_names = ["dsb_0", "usb_0_bp", "lsb_0", "dsb_p30_bp", "usb_p30", "lsb_p30_bp", "dsb_m170", "usb_m170_bp", "lsb_m170", "usb_design_own",
                  "usb_reopen", "dsb_reopen_bp"]
    chans = []                                              # (case, cuts, is sync)
    for i, name in enumerate(sync_names):
        chans.append((sc.BY[name], sc.cut(sc.inputs(sc.BY[name]), sc.BY[name]["splits"]), True))
        if i % 3 == 2:
            e = {c["name"]: c for c in ac.CASES}[ENVELOPE[i // 3]]
            chans.append((e, ac.cut(ac.inputs(e), e["splits"]), False))
    assert len(chans) == 16
    bank = sa.AmDemodBank([gcfg(c["cfg"]) for c, _, _ in chans], sync=[gsync(c["sync"]) if s else sa.AmSyncCfg() for c, _, s in chans])
    rounds = max(len(x) for _, x, _ in chans)
    empty = np.zeros(0, np.int16)
    got = [[] for _ in chans]
    for r in range(rounds):
        bank.feed([x[r] if r < len(x) else empty for _, x, _ in chans])
        for c, (_, x, _) in enumerate(chans):
            a = bank.read(c)
            if r < len(x):
                got[c].append(a)
            else:
                assert a.size == 0, (c, r)                  # an empty feed: no audio, state untouched
    for c, (case, _, is_sync) in enumerate(chans):
        name = case["name"]
        if is_sync:
            assert_feeds_equal(got[c], want_feeds(gold, case), name)
            check_state(bank, c, gold, case, -1, name)
            continue
        audio = np.concatenate(got[c])
        assert [g.size for g in got[c]] == list(env_gold[name + "/counts"]), name
        if name + "/audio" in env_gold.files:
            assert np.array_equal(audio, env_gold[name + "/audio"]), name
        else:
            assert hashlib.sha256(audio.tobytes()).hexdigest() == str(env_gold[name + "/sha256"]), name
        m, s, p, n = bank.levels(c)
        lv, st = env_gold[name + "/levels"], env_gold[name + "/state"]
        assert (m, p, n, bank.squelch_open(c)) == (lv[0], lv[2], int(st[0]), bool(st[1])), name
        assert bank.pll(c) == (False, 0.0), name


def test_reset_restores_a_fresh_handle(gold):
    for name in ("dsb_reopen_bp", "usb_m170_bp"):
        case = sc.BY[name]
        bank, first = run_gpu(gold, case)
        assert_feeds_equal(first, want_feeds(gold, case), name)
        # leave the loop turning, a block half full and the AGC history part full
        bank.feed([sc.inputs(sc.BY["usb_p30"])[: 2 * 2777]])
        bank.reset()
        assert bank.levels(0) == (0.0, 0.0, 0.0, 0) and not bank.squelch_open(0) and bank.pll(0) == (False, 0.0)
        _, again = run_gpu(gold, case, bank=bank, check_each=True)
        assert_feeds_equal(again, want_feeds(gold, case), name + " after reset")


def test_feed_dev_and_last_dev_match_feed(gold):
    import torch
    case = sc.BY["lsb_0"]
    bank = make_bank(case)
    for i, (x, w) in enumerate(zip(sc.cut(sc.inputs(case), case["splits"]), want_feeds(gold, case))):
        t = torch.from_numpy(x.copy()).cuda() if x.size else torch.zeros(2, dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        bank.feed_dev([t.data_ptr()], [x.size // 2])
        ptr, n = bank.last_dev(0)
        assert n == w.size
        assert np.array_equal(bank.read(0), w)
        assert (ptr != 0) or n == 0
        bank.sync()
        check_state(bank, 0, gold, case, i, f"feed_dev {i}")


def test_feed_bank_device_handover():
    """a 1.024 MS/s stream, 3 channels at req_rate 8000 (DSB, USB and envelope), 600 000 samples in three uneven feeds: the audio and
    the loop state of feed_bank equal feed() of what the channelizer bank's read returned; the next bank.feed queued right behind does
    not disturb it"""
    from tests import synth
    fs, n_ch = 1_024_000, 3
    fcs = [-300_000, 1371, 225_000]
    bank_dev = sa.ChannelizerBank(fs, [8000] * n_ch, fcs)
    bank_host = sa.ChannelizerBank(fs, [8000] * n_ch, fcs)
    cfgs, syncs = [], []
    for c in range(n_ch):
        _, out_rate, ofs = bank_dev.info(c)
        assert out_rate >= 8000
        cfgs.append(gcfg((out_rate, -ofs, 8000, 3000.0, 1.0, -90.0, 0, c % 2)))
        syncs.append(sa.AmSyncCfg(pll=int(c < 2), sync_op=c % 2))
    am, am_host = sa.AmDemodBank(cfgs, sync=syncs), sa.AmDemodBank(cfgs, sync=syncs)
    x = synth.mix(600_000, 78, 3000, 1500, 1)
    cuts = ((0, 200_001), (200_001, 430_000), (430_000, 600_000))
    segs = [x[2 * a: 2 * b] for a, b in cuts]
    heard = [False] * n_ch

    def check(seg):
        bank_host.feed(seg)
        am_host.feed([bank_host.read(c) for c in range(n_ch)])
        for c in range(n_ch):
            got, want = am.read(c), am_host.read(c)
            assert got.size == want.size and got.size > 0 and np.array_equal(got, want), c
            assert am.pll(c) == am_host.pll(c) and am.levels(c) == am_host.levels(c), c
            heard[c] = heard[c] or bool(got.any())

    for i, seg in enumerate(segs):
        bank_dev.feed(seg)                   # from the second round on this overwrites the queues the demodulators were handed
        if i:
            check(segs[i - 1])               # ... before their results for the previous feed are looked at
        am.feed_bank(bank_dev)
        for c in range(n_ch):
            bank_dev.skip(c)
    check(segs[-1])
    assert all(am.squelch_open(c) for c in range(n_ch)) and all(heard)


def test_twenty_channels_reach_a_second_prefix_sum_group(gold):
    """am_sync_psum_kernel takes sixteen channels per workgroup: twenty sync channels in one handle, the three operations in turn on
    short cases, put its second workgroup to work; every channel equals its recording"""
    names = ["trace_usb_m170", "lsb_muted", "dsb_never_open", "usb_block_edges"]
    chans = [sc.BY[names[c % len(names)]] for c in range(20)]
    cuts = [sc.cut(sc.inputs(c), c["splits"]) for c in chans]
    bank = sa.AmDemodBank([gcfg(c["cfg"]) for c in chans], sync=[gsync(c["sync"]) for c in chans])
    empty = np.zeros(0, np.int16)
    got = [[] for _ in chans]
    for r in range(max(len(x) for x in cuts)):
        bank.feed([x[r] if r < len(x) else empty for x in cuts])
        for c, x in enumerate(cuts):
            if r < len(x):
                got[c].append(bank.read(c))
    for c, case in enumerate(chans):
        assert_feeds_equal(got[c], want_feeds(gold, case), f"{case['name']} as channel {c}")
        check_state(bank, c, gold, case, -1, f"{case['name']} as channel {c}")
