"""GPU: RDS in the broadcast-FM bank (sdrx_bfmrds_*) against the recording of the reference's own RDSDemod, RDSDecoder, Interpolator
and RDSPhaseLock (tests/golden/bfm_rds_golden.npz): the bits and groups of every feed, subcarr_bb of every RDS sample, the
report, the whole carried state after every feed, and no unsure sample in any case.  Then one handle of 11 channels with RDS on
and off, mono and stereo interleaved; reset; queued device feeds; the hand-over from the channelizer bank; and that RDS disturbs
neither the audio nor the sink stream, nor a handle created without it."""
import numpy as np
import pytest

import sdrangel_amd as sa
from tests import bfm_cases as bc
from tests import bfm_rds_cases as rc
from tests.test_bfm_gpu import gcfg

pytestmark = pytest.mark.gpu
BY_NAME = {c["name"]: c for c in rc.CASES}


@pytest.fixture(scope="module")
def gold():
    return rc.golden()


def snapshot(bank, ch) -> dict:
    """what the interface gives about the last feed of an RDS channel"""
    a, q, f, dq, synced = bank.rds_report(ch)
    rep = np.array([np.float32(v).view(np.uint32) for v in (a, q, f, dq)] + [int(synced)], np.uint32)
    return {"bits": bank.rds_bits(ch), "groups": bank.rds_groups(ch), "bb": bank.rds_bb(ch), "report": rep, "state": rc.state_words(bank.rds_state(ch))}


def run_gpu(case, bank=None, iq=None):
    bank = bank or sa.BfmBank([gcfg(case["cfg"])], rds=[case["rds"]])
    feeds = []
    for x in bc.cut(rc.inputs(case) if iq is None else iq, case["splits"]):
        bank.feed([x])
        feeds.append(snapshot(bank, 0))
    return bank, feeds


def assert_feed_equals(got: dict, want: dict, i: int, what: str):
    assert np.array_equal(got["bits"], want["bits"][i]), (what, "bits of feed", i, got["bits"].size, want["bits"][i].size)
    assert np.array_equal(got["groups"], want["groups"][i]), (what, "groups of feed", i)
    assert got["bb"].size == want["n_rds"][i], (what, "RDS samples of feed", i, got["bb"].size, want["n_rds"][i])
    if want["bb"] is not None:
        bad = np.flatnonzero(got["bb"].view(np.uint32) != want["bb"][i].view(np.uint32))
        assert bad.size == 0, (what, "subcarr_bb of feed", i, "first at", int(bad[0]), "of", bad.size)
    else:
        if got["bb"].size:
            e = min(rc.BB_EDGE, got["bb"].size)
            assert np.array_equal(got["bb"][:e].view(np.uint32), want["bb_head"][i][:e].view(np.uint32)), (what, "head of subcarr_bb of feed", i)
            assert np.array_equal(got["bb"][-e:].view(np.uint32), want["bb_tail"][i][-e:].view(np.uint32)), (what, "tail of subcarr_bb of feed", i)
        assert rc.sha_f32(got["bb"]) == want["bb_sha"][i], (what, "subcarr_bb of feed", i)
    for k in range(4):
        assert rc.same_float_bits(int(got["report"][k]), int(want["report"][i][k])), (what, "report", k, "feed", i, got["report"], want["report"][i])
    assert got["report"][4] == want["report"][i][4], (what, "synced() after feed", i)
    diff = [(f, int(g), int(w)) for f, g, w in zip(rc.STATE_FIELDS, got["state"], want["state"][i]) if g != w]
    assert not diff, (what, "state after feed", i, diff)


def assert_equals_recording(feeds, want, what):
    assert len(feeds) == len(want["n_rds"])
    for i, f in enumerate(feeds):
        assert_feed_equals(f, want, i, what)


@pytest.mark.parametrize("case", rc.CASES, ids=[c["name"] for c in rc.CASES])
def test_case_equals_the_recording(gold, case):
    x = rc.inputs(case)
    want = rc.golden_case(gold, case)
    assert bc.sha(x) == want["in_sha"], "the generator gave other samples than the recorder was fed"
    bank, feeds = run_gpu(case, iq=x)
    assert_equals_recording(feeds, want, case["name"])
    assert bank.rds_unsure(0) == 0, "a sample whose mixer product the enclosure does not pin"


def test_the_long_case_decodes_in_the_recording_and_here(gold):
    """the reference's own chain left SYNC after the 50-block count, found presync and sync again and completed groups; two of
    the cuts put a bit, and a bit that completes a group, on the last RDS sample of a feed"""
    want = rc.golden_case(gold, BY_NAME["long_288k"])
    sync = [int(s[rc.STATE_FIELDS.index("sync")]) for s in want["state"]]
    assert sync == [1, 1, 0, 1, 1] and sum(g.shape[0] for g in want["groups"][3:]) >= 3
    assert (np.concatenate(want["groups"])[:, 0] == 0xD314).all()                # the PI code that was sent
    # bits and groups come out at RDS samples whose index is a multiple of 8: numsamples after feeds 0 and 3 is one past one
    ns = [int(s[rc.STATE_FIELDS.index("numsamples")]) for s in want["state"]]
    assert ns[0] % 8 == 1 and ns[3] % 8 == 1 and want["groups"][3].shape[0] >= 1


def test_rds_leaves_audio_and_sink_stream_alone(gold):
    case = BY_NAME[rc.AUDIO_CASE]
    ac, sc = gold[f"{case['name']}/audio_counts"], gold[f"{case['name']}/sink_counts"]
    audio, sink = np.split(gold[f"{case['name']}/audio"], np.cumsum(ac)[:-1]), np.split(gold[f"{case['name']}/sink"], np.cumsum(sc)[:-1])
    on, off = sa.BfmBank([gcfg(case["cfg"])], rds=[1]), sa.BfmBank([gcfg(case["cfg"])])
    for i, x in enumerate(bc.cut(rc.inputs(case), case["splits"])):
        on.feed([x]); off.feed([x])
        a, k = on.read(0), on.read_sink(0)
        assert np.array_equal(a, audio[i]) and np.array_equal(k[:, 0], sink[i]) and not np.any(k[:, 1]), i
        assert np.array_equal(a, off.read(0)) and np.array_equal(k, off.read_sink(0)), i
        assert on.pilot(0) == off.pilot(0) and on.levels(0) == off.levels(0)


def test_null_and_zero_rds_are_create(gold):
    """same outputs, the same walk named by last_launch, and the RDS calls refuse the channel"""
    case = bc.CASES[0]
    banks = [sa.BfmBank([gcfg(case["cfg"])]), sa.BfmBank([gcfg(case["cfg"])], rds=[0])]
    for x in bc.cut(bc.inputs(case), case["splits"]):
        outs = []
        for b in banks:
            b.feed([x])
            outs.append((b.read(0), b.read_sink(0), b.pilot(0), b.levels(0), b.last_launch()))
        assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1]) and outs[0][2:] == outs[1][2:]
    assert banks[1].last_launch()["kernel"] == "bfm_walk_kernel"
    on = sa.BfmBank([gcfg(case["cfg"])], rds=[1])                     # an RDS-on stereo handle runs, and reports, the other walk
    on.feed([bc.inputs(case)[: 2 * 2048]])
    assert on.last_launch()["kernel"] == "bfm_walk_rds_kernel"
    mono = sa.BfmBank([gcfg(dict(case["cfg"], stereo=0))], rds=[1])   # a mono one has no walk at all
    mono.feed([bc.inputs(case)[: 2 * 2048]])
    assert mono.last_launch()["kernel"] == "bfm_fft_kernel"
    for call in (banks[1].rds_bits, banks[1].rds_groups, banks[1].rds_report, banks[1].rds_state, banks[1].rds_unsure):
        with pytest.raises(sa.SdrxError, match="without RDS"):
            call(0)


def _mixed():
    """11 channels: RDS on and off, mono and stereo interleaved, each with its own feed lengths: three workgroups of each walk"""
    names = [("stereo_250k", 1), ("mono_250k", 1), ("stereo_240k", 0), ("lsb_384k", 1), ("mono_240k_one_feed", 0), ("squelch_bursts", 1),
             ("mono_384k", 1), ("pilot_stops", 0), ("stereo_240k", 1), ("noise", 1), ("mono_240k_one_feed", 1)]
    return [(BY_NAME[n], on) for n, on in names]


def test_rds_on_and_off_mono_and_stereo_interleaved_in_one_handle(gold):
    chans = _mixed()
    assert len(chans) == 11 and {(c["cfg"]["stereo"], on) for c, on in chans} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    bank = sa.BfmBank([gcfg(c["cfg"]) for c, _ in chans], rds=[on for _, on in chans])
    plain = [None if on else sa.BfmBank([gcfg(c["cfg"])]) for c, on in chans]
    cuts = [bc.cut(rc.inputs(c), c["splits"]) for c, _ in chans]
    empty = np.zeros(0, np.int16)
    feeds = [[] for _ in chans]
    for r in range(max(len(x) for x in cuts)):
        bank.feed([x[r] if r < len(x) else empty for x in cuts])
        for i, ((c, on), x) in enumerate(zip(chans, cuts)):
            if r >= len(x):
                if on:
                    assert bank.rds_bits(i).size == 0 and bank.rds_bb(i).size == 0, (i, r)     # an empty feed: nothing out
                continue
            if on:
                feeds[i].append(snapshot(bank, i))
            else:
                plain[i].feed([x[r]])
                assert np.array_equal(bank.read(i), plain[i].read(0)) and np.array_equal(bank.read_sink(i), plain[i].read_sink(0)), (i, r)
                with pytest.raises(sa.SdrxError, match="without RDS"):
                    bank.rds_bits(i)
    for i, (c, on) in enumerate(chans):
        if on:
            assert_equals_recording(feeds[i], rc.golden_case(gold, c), f"channel {i} {c['name']}")
            assert bank.rds_unsure(i) == 0


def test_reset_restores_a_fresh_handle(gold):
    for name in ("stereo_250k", "bits_250k"):
        case = BY_NAME[name]
        want = rc.golden_case(gold, case)
        bank, first = run_gpu(case)
        assert_equals_recording(first, want, name)
        bank.feed([rc.inputs(case)[: 2 * 777]])            # leave pending samples and a half-way state behind
        bank.reset()
        st = bank.rds_state(0)
        assert st.numsamples == 0 and st.bit_counter == 0 and st.sync == 1 and st.mix_phase == 0 and st.subcarr_phi == 0
        assert st.distance_remain == np.float32(np.float64(np.float32(case["cfg"]["in_rate"])) / 250000.0).view(np.uint32)
        _, again = run_gpu(case, bank=bank)
        assert_equals_recording(again, want, name + " after reset")


def test_queued_device_feeds_equal_synced_feeds(gold):
    """feed_dev after feed_dev on device-resident pieces, nothing read in between: the last feed's bits, groups and subcarr_bb and
    the state behind all of them equal the recording's"""
    import torch
    for name in ("stereo_250k", "lsb_384k", "bits_250k"):
        case = BY_NAME[name]
        want = rc.golden_case(gold, case)
        pieces = bc.cut(rc.inputs(case), case["splits"])
        dev = [torch.from_numpy(x.copy()).cuda() if x.size else torch.zeros(2, dtype=torch.int16, device="cuda") for x in pieces]
        torch.cuda.synchronize()
        bank = sa.BfmBank([gcfg(case["cfg"])], rds=[1])
        for t, x in zip(dev, pieces):
            bank.feed_dev([t.data_ptr()], [x.size // 2])
        assert_feed_equals(snapshot(bank, 0), want, len(pieces) - 1, name + " queued")
        p, n = bank.rds_bits_last_dev(0)
        assert n == want["bits"][-1].size and (p != 0 or n == 0)


def test_feed_bank_equals_feed_of_the_banks_output():
    """a small channelizer bank, 4 channels at 240 kS/s (the clamped schedule): feed_bank on the device equals feed() of what
    bank.read returned"""
    fs, n_ch = 3_840_000, 4
    fcs = [-900_000 + 600_000 * c + 1371 * c for c in range(n_ch)]
    bank_dev = sa.ChannelizerBank(fs, [240000] * n_ch, fcs)
    bank_host = sa.ChannelizerBank(fs, [240000] * n_ch, fcs)
    cfgs = []
    for c in range(n_ch):
        _modes, out_rate, ofs = bank_dev.info(c)
        cfgs.append(gcfg(bc._cfg(out_rate, nco_freq=-ofs, rf=12500.0, sq=-80.0, stereo=c % 2, lsb=(c // 2) % 2)))
    rds = [1, 1, 0, 1]
    bfm, bfm_host = sa.BfmBank(cfgs, rds=rds), sa.BfmBank(cfgs, rds=rds)
    from tests import synth
    x = synth.mix(400_000, 78, 3000, 1500, 1)
    for a, b in ((0, 150_001), (150_001, 400_000)):
        seg = x[2 * a: 2 * b]
        bank_dev.feed(seg); bank_host.feed(seg)
        bfm.feed_bank(bank_dev)
        chans = [bank_host.read(c) for c in range(n_ch)]
        for c in range(n_ch):
            bank_dev.skip(c)
        bfm_host.feed(chans)
        for c in range(n_ch):
            assert np.array_equal(bfm.read(c), bfm_host.read(c)), c
            if not rds[c]:
                continue
            g, w = snapshot(bfm, c), snapshot(bfm_host, c)
            assert g["bb"].size > 1000 and g["bits"].size > 4
            assert np.array_equal(g["bits"], w["bits"]) and np.array_equal(g["bb"].view(np.uint32), w["bb"].view(np.uint32)), c
            assert np.array_equal(g["state"], w["state"]) and np.array_equal(g["groups"], w["groups"]), c
