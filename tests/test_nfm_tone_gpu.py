"""GPU: the NFM demodulator bank with CTCSS and the AF squelch (sdrx_nfm_create_ex) against the oracle (tests/nfm_tone_oracle.c):
every audio sample, every change of m_ctcssIndex with its position, the detector's powers as bit patterns, its block count and
flags, m_afSquelchOpen, the AF squelch's sums as uint64 patterns and its counter, the levels and the squelch state -- the named cases of tests/nfm_tone_cases.py, 16 mixed channels in one handle against 16 handles of one
channel, random cuts, feeds queued without a sync, reset, the hand-over from a channelizer bank, 20 random configurations; and,
independent of that oracle, a handle with CTCSS on and no tone selected, or with every option off, against the plain bank."""
import numpy as np
import pytest

import sdrangel_amd as sa
from tests import nfm_cases as nc
from tests import nfm_tone_cases as tc
from tests import oracle_py as orc
from tests.test_nfm_gpu import assert_feeds_equal, check_levels, gcfg

pytestmark = pytest.mark.gpu
BY = {c["name"]: c for c in tc.CASES}


@pytest.fixture(scope="module")
def oracle():
    return tc.build_oracle()


@pytest.fixture(scope="module")
def wants(oracle):
    """every named case through the oracle once, shared (and left unchanged) by the tests below"""
    return {c["name"]: tc.run_oracle(oracle, c) for c in tc.CASES}


def tcfg(cfg) -> sa.NfmToneCfg:
    return sa.NfmToneCfg(delta_squelch=int(cfg[12]) if len(cfg) > 12 else 0, ctcss_on=int(cfg[10]), ctcss_index=int(cfg[11]), reserved=0)


def make_bank(cfgs) -> sa.NfmDemodBank:
    return sa.NfmDemodBank([gcfg(c) for c in cfgs], tone=[tcfg(c) for c in cfgs])


def run_gpu(case, splits=None, bank=None):
    bank = bank or make_bank([case["cfg"]])
    feeds, events = [], []
    for x in tc.cut(tc.inputs(case), splits or case["splits"]):
        bank.feed([x])
        feeds.append(bank.read(0))
        events.append(bank.ctcss_events(0))
    return bank, feeds, events


def stream_events(feeds, events):
    return tc.all_events({"feeds": feeds, "events": events})


def check_tone_state(bank, ch, want, what):
    index, hz, changes = bank.ctcss(ch)
    power, detected, max_index, blocks = bank.ctcss_powers(ch)
    print(f"{what}: index {index} ({hz} Hz), changes {changes}, blocks {blocks}, detected {detected}, max {max_index}, max power {power.max()!r}")
    assert (index, changes, blocks, detected, max_index) == (want["index"], want["changes"], want["blocks"], want["detected"], want["max_index"]), what
    assert hz == (np.float32(tc.TONES[index - 1]) if index else 0.0), what
    assert np.array_equal(power.view(np.uint32), want["power"].view(np.uint32)), what
    af_open, af_sums, af_count = bank.af_squelch(ch)
    print(f"{what}: AF open {af_open}, counter {af_count}, sums {af_sums[0]!r} {af_sums[1]!r}")
    assert (af_open, af_count) == (want["af_open"], want["af_count"]), what
    assert np.array_equal(af_sums.view(np.uint64), want["af_sums"].view(np.uint64)), what
    check_levels(bank, ch, want, what)


def check_events(got, want, what):
    assert len(got) == len(want), what
    for i, ((ga, gi), (wa, wi)) in enumerate(zip(got, want)):
        assert np.array_equal(ga, wa) and np.array_equal(gi, wi), (what, i, ga, gi, wa, wi)


@pytest.mark.parametrize("case", tc.CASES, ids=[c["name"] for c in tc.CASES])
def test_case_bit_exact(wants, case):
    want = wants[case["name"]]
    bank, got, events = run_gpu(case)
    assert_feeds_equal(got, want["feeds"], case["name"])
    check_events(events, want["events"], case["name"])
    check_tone_state(bank, 0, want, case["name"])


def test_design_products_equal_the_oracle(oracle):
    for name in ("tone_selected", "cuts_block_ends", "rate48k_tone32", "af_1k_opens", "af_threshold_straddled", "af_and_ctcss"):
        case = BY[name]
        N, rate, coef, lp = tc.OracleNfmTone(oracle, case["cfg"]).design()
        bank = make_bank([case["cfg"]])
        g = bank.tone_design(0)
        an, tones, acoef, th = tc.OracleNfmTone(oracle, case["cfg"]).af_design()
        assert g[4] == an and g[7] == th and (th != 0.0) == bool(case["cfg"][12]), name
        assert bank.af_squelch(0)[0] is False and bank.af_squelch(0)[2] == 0 and not bank.af_squelch(0)[1].any(), name      # nothing fed yet
        assert np.array_equal(g[5].view(np.uint64), tones.view(np.uint64)) and np.array_equal(g[6].view(np.uint64), acoef.view(np.uint64)), name
        assert g[:2] == (N, rate) == (case["cfg"][2] // 16, case["cfg"][2] // 8), name
        assert np.array_equal(g[2].view(np.uint32), coef.view(np.uint32)), name
        assert np.array_equal(g[3].view(np.uint32), lp.view(np.uint32)), name
        # the plain design is untouched
        nt, taps, bp, inc, lvl, gate = nc.OracleNfm(nc.build_oracle(), case["cfg"][:10]).design()
        d = bank.design(0)
        # m_squelchLevel as the mode defines it: pow(10, squelch / 100), or -squelch / 1000 with the AF squelch
        lvl = tc.OracleNfmTone(oracle, case["cfg"]).level() if case["cfg"][12] else lvl
        assert np.array_equal(d[2].view(np.uint32), bp.view(np.uint32)) and np.float32(d[4]) == np.float32(lvl) and d[5] == gate, name


@pytest.mark.parametrize("name", ["tone_any", "carrier_gap", "rate48k_tone32"])
def test_no_tone_selected_and_options_off_equal_the_plain_bank(name):
    """independent of tests/nfm_tone_oracle.c: the same input through sdrx_nfm_create, through create_ex with every option off,
    and through create_ex with CTCSS on and no tone selected gives the same audio, feed by feed"""
    case = BY[name]
    base = case["cfg"][:10]
    plain = sa.NfmDemodBank([gcfg(base)])
    off = make_bank([base + (0, 0)])
    off_null = sa.NfmDemodBank([gcfg(base)], tone=[sa.NfmToneCfg()])
    on_any = make_bank([base + (1, 0)])
    heard = 0
    for x in tc.cut(tc.inputs(case), case["splits"]):
        outs = []
        for b in (plain, off, off_null, on_any):
            b.feed([x])
            outs.append(b.read(0))
        for o in outs[1:]:
            assert o.size == outs[0].size and np.array_equal(o, outs[0]), name
        heard += int(np.count_nonzero(outs[0]))
    assert heard > 10000, heard
    assert plain.levels(0) == off.levels(0) == on_any.levels(0)
    assert off.ctcss(0) == (0, 0.0, 0) and off.ctcss_powers(0)[3] == 0
    assert on_any.ctcss_powers(0)[3] > 0 and on_any.ctcss(0)[0] > 0


def test_sixteen_mixed_channels_in_one_handle(wants):
    """twelve named cases, plus four with other options: every combination of AF squelch and CTCSS, a tone selected or not, rates
    8000 and 48000, muted and unmuted, all in one handle, against sixteen handles of one channel"""
    cases = list(tc.CASES)
    cases = [c for c in cases if c["name"] not in ("af_noise_closed", "af_all_zero", "af_gate_24000", "tone_any", "no_tone", "tone_removed",
                                                   "neighbour_tones", "cuts_one_feed", "rate48k_tone1_other")]
    for name, on, index, delta in (("tone_selected", 0, 12, 0), ("carrier_gap", 0, 0, 0), ("rate48k_tone32", 1, 0, 1), ("tone_muted", 0, 0, 1)):
        cases.append(dict(BY[name], cfg=BY[name]["cfg"][:10] + (on, index, delta)))
    assert {(c["cfg"][12], c["cfg"][10]) for c in cases} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert len(cases) == 16 and {c["cfg"][2] for c in cases} == {8000, 48000} and {c["cfg"][9] for c in cases} == {0, 1}
    assert {(c["cfg"][10], c["cfg"][11] != 0) for c in cases} == {(0, False), (0, True), (1, False), (1, True)}
    bank = make_bank([c["cfg"] for c in cases])
    cuts = [tc.cut(tc.inputs(c), c["splits"]) for c in cases]
    rounds = max(len(x) for x in cuts)
    empty = np.zeros(0, np.int16)
    got, events = [[] for _ in cases], [[] for _ in cases]
    for r in range(rounds):
        bank.feed([x[r] if r < len(x) else empty for x in cuts])
        for c, x in enumerate(cuts):
            a = bank.read(c)
            if r < len(x):
                got[c].append(a); events[c].append(bank.ctcss_events(c))
            else:
                assert a.size == 0 and bank.ctcss_events(c)[0].size == 0, (c, r)    # an empty feed: no audio, state untouched
    for c, case in enumerate(cases):
        single, feeds, ev = run_gpu(case)
        what = f"channel {c} ({case['name']} {case['cfg'][10:]})"
        assert_feeds_equal(got[c], feeds, what)
        check_events(events[c], ev, what)
        assert bank.ctcss(c) == single.ctcss(0), what
        gp, sp = bank.ctcss_powers(c), single.ctcss_powers(0)
        assert np.array_equal(gp[0].view(np.uint32), sp[0].view(np.uint32)) and gp[1:] == sp[1:], what
        assert bank.levels(c) == single.levels(0) and bank.squelch_open(c) == single.squelch_open(0), what
        ga, sa_ = bank.af_squelch(c), single.af_squelch(0)
        assert ga[0] == sa_[0] and ga[2] == sa_[2] and np.array_equal(ga[1].view(np.uint64), sa_[1].view(np.uint64)), what
        if case is BY.get(case["name"]):
            check_tone_state(bank, c, wants[case["name"]], what)


@pytest.mark.parametrize("name", ["carrier_gap", "neighbour_tones", "af_lap", "af_and_ctcss"])
def test_random_splits_equal_one_feed(oracle, name):
    case = BY[name]
    want = tc.run_oracle(oracle, case, splits=[case["n"]])
    one = np.concatenate(want["feeds"])
    rng = np.random.default_rng(len(name))
    for trial in range(2):
        splits, left = [], case["n"]
        while left > 0:
            m = min(left, int(rng.choice([0, 1, 5, 7, 8, 9, int(rng.integers(1, 2000)), int(rng.integers(1, 12000)), int(rng.integers(1, 12000))])))
            splits.append(m); left -= m
        bank, got, events = run_gpu(case, splits)
        assert np.array_equal(np.concatenate(got), one), (name, trial)
        assert stream_events(got, events) == tc.all_events(want), (name, trial)
        check_tone_state(bank, 0, want, f"{name} trial {trial}")


def test_feeds_queued_without_a_sync(wants):
    """feed_dev after feed_dev on device-resident pieces, nothing read in between: the carry of one feed is the next one's input
    on the device alone.  The last feed's audio and everything that accumulates equal the oracle's"""
    import torch
    for name in ("cuts_block_ends", "carrier_gap", "af_sig_noise_sig_gate_gt_z"):
        case = BY[name]
        want = wants[name]
        pieces = tc.cut(tc.inputs(case), case["splits"])
        dev = [torch.from_numpy(x.copy()).cuda() if x.size else torch.zeros(2, dtype=torch.int16, device="cuda") for x in pieces]
        torch.cuda.synchronize()
        bank = make_bank([case["cfg"]])
        for t, x in zip(dev, pieces):
            bank.feed_dev([t.data_ptr()], [x.size // 2])
        assert np.array_equal(bank.read(0), want["feeds"][-1]), name
        check_events([bank.ctcss_events(0)], [want["events"][-1]], name)
        check_tone_state(bank, 0, want, name + " queued")


def test_reset_restores_a_fresh_handle(wants):
    for name in ("tone_removed", "carrier_gap", "af_and_ctcss"):
        case = BY[name]
        want = wants[name]
        bank, first, ev = run_gpu(case)
        assert_feeds_equal(first, want["feeds"], name)
        # leave a detected tone, a partial block and half-full rings behind
        bank.feed([tc.inputs(BY["tone_selected"])[: 2 * 9000]])
        bank.reset()
        assert bank.ctcss(0) == (0, 0.0, 0) and bank.ctcss_powers(0)[1:] == (False, 0, 0) and not bank.ctcss_powers(0)[0].any()
        assert bank.levels(0) == (0.0, 0.0, 0.0, 0) and not bank.squelch_open(0)
        _, again, ev2 = run_gpu(case, bank=bank)
        assert_feeds_equal(again, want["feeds"], name + " after reset")
        check_events(ev2, want["events"], name + " after reset")
        check_tone_state(bank, 0, want, name + " after reset")


def test_feed_bank_device_handover(oracle):
    """a 1.024 MS/s stream, two channels at req_rate 8000, each with a carrier that has a sub-audible tone, in three uneven
    feeds: the audio and the tone state of feed_bank equal the oracle on the bank oracle's output"""
    fs, n_ch, n = 1_024_000, 2, 1_900_000
    fcs = [-200_000, 150_000]
    hz = [100.0, 103.5]
    bank_dev = sa.ChannelizerBank(fs, [8000] * n_ch, fcs)
    x = np.zeros(2 * n, np.int64)
    for c in range(n_ch):
        sig = {"kind": "tone", "tones": [(n, hz[c])], "f0": float(fcs[c]), "tdev": 400.0, "dev": 1500.0, "fa": 1000.0, "amp": 6000.0, "noise": 10.0}
        x += tc.signal(sig, n, fs, 300 + c)
    x = x.astype(np.int16)
    cfgs, oras, chains = [], [], []
    for c in range(n_ch):
        modes, out_rate, ofs = bank_dev.info(c)
        assert out_rate >= 8000
        cfg = (out_rate, -ofs, 8000, 8330.0, 3000.0, 2000, 2.0, -600.0, 1, 0, 1, 12)      # tone 12 selected in both
        cfgs.append(cfg); oras.append(tc.OracleNfmTone(oracle, cfg)); chains.append(orc.Chain(modes))
    nfm = make_bank(cfgs)
    cuts = ((0, 700_001), (700_001, 1_250_000), (1_250_000, n))
    heard = [0] * n_ch
    for a, b in cuts:
        seg = x[2 * a: 2 * b]
        bank_dev.feed(seg)
        nfm.feed_bank(bank_dev)
        for c in range(n_ch):
            bank_dev.skip(c)
            want = oras[c].feed(chains[c].feed(seg))
            got = nfm.read(c)
            assert got.size == want.size and got.size > 0 and np.array_equal(got, want), c
            wa, wi = oras[c].events()
            ga, gi = nfm.ctcss_events(c)
            assert np.array_equal(ga, wa) and np.array_equal(gi, wi), c
            heard[c] += int(np.count_nonzero(got))
    # channel 0 hears its tone; what channel 1 detects next to a second carrier is the oracle's word, and never tone 12
    assert nfm.ctcss(0)[0] == 12 and heard[0] > 3000 and nfm.ctcss(1)[0] != 12 and heard[1] == 0, (nfm.ctcss(0), nfm.ctcss(1), heard)
    for c in range(n_ch):
        assert nfm.ctcss(c)[::2] == oras[c].ctcss() and nfm.ctcss_powers(c)[3] == oras[c].powers()[3] >= 2, c
        assert np.array_equal(nfm.ctcss_powers(c)[0].view(np.uint32), oras[c].powers()[0].view(np.uint32)), c


def test_random_configurations_in_one_handle(oracle):
    """the first 20 random configurations of tests/nfm_tone_cases.py, one channel each of one handle"""
    cases = tc.random_cases(20)
    wants = [tc.run_oracle(oracle, c) for c in cases]
    bank = make_bank([c["cfg"] for c in cases])
    cuts = [tc.cut(tc.inputs(c), c["splits"]) for c in cases]
    empty = np.zeros(0, np.int16)
    got, events = [[] for _ in cases], [[] for _ in cases]
    for r in range(max(len(x) for x in cuts)):
        bank.feed([x[r] if r < len(x) else empty for x in cuts])
        for c, x in enumerate(cuts):
            if r < len(x):
                got[c].append(bank.read(c)); events[c].append(bank.ctcss_events(c))
    for c, case in enumerate(cases):
        assert_feeds_equal(got[c], wants[c]["feeds"], case["name"])
        check_events(events[c], wants[c]["events"], case["name"])
        check_tone_state(bank, c, wants[c], case["name"])
    assert sum(w["blocks"] > 0 for w in wants) >= 10 and sum(w["probe"]["mismatch"] > 0 for w in wants) >= 5


def test_seventy_channels_reach_the_walk_kernels_second_workgroup(oracle):
    """nfm_af_walk_kernel takes one lane per channel, 64 to a workgroup: 70 channels, the AF squelch in four of five, the first
    9000 inputs of five cases in two feeds, every channel against the oracle"""
    names = ("af_sig_noise_sig_gate_lt_z", "af_threshold_straddled", "tone_selected", "af_and_ctcss", "af_noise_closed")
    cases = [BY[names[c % 5]] for c in range(70)]
    bank = make_bank([c["cfg"] for c in cases])
    xs = {n: tc.inputs(BY[n])[: 2 * 9000] for n in names}
    want = {}
    for n in names:
        o = tc.OracleNfmTone(oracle, BY[n]["cfg"])
        want[n] = ([o.feed(xs[n][: 2 * 4001]), o.feed(xs[n][2 * 4001:])], o.af(), o.ctcss())
    got = [[] for _ in cases]
    for lo, hi in ((0, 4001), (4001, 9000)):
        bank.feed([xs[c["name"]][2 * lo: 2 * hi] for c in cases])
        for k in range(70):
            got[k].append(bank.read(k))
    for k, c in enumerate(cases):
        feeds, (af_open, af_sums, af_count), (index, changes) = want[c["name"]]
        assert_feeds_equal(got[k], feeds, f"channel {k} {c['name']}")
        ga = bank.af_squelch(k)
        assert (ga[0], ga[2]) == (af_open, af_count) and np.array_equal(ga[1].view(np.uint64), af_sums.view(np.uint64)), k
        assert bank.ctcss(k)[::2] == (index, changes), k
