"""GPU: the broadcast-FM stereo demodulator bank (sdrx_bfm_*) against the recording of the reference's own classes
(tests/golden/bfm_golden.npz): every l, r pair, every Sample of the sink stream and the state after every feed of every case;
mono and stereo channels interleaved in one handle, reset, queued device feeds, the hand-over from the channelizer bank.

Of the state the fixture keeps, the interface gives locked(), get_pilot_level() (2 * m_pilot_level, exact) and the bits of m_freq and
m_phase, the squelch flag and the levels; m_lock_cnt, m_squelchState and both m_y1 are checked on the oracle (tests/test_bfm_oracle.py)
and show here in what follows from them."""
import numpy as np
import pytest

import sdrangel_amd as sa
from tests import bfm_cases as bc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def oracle():
    return bc.build_oracle()


@pytest.fixture(scope="module")
def gold():
    return bc.golden()


def gcfg(cfg) -> sa.BfmCfg:
    return sa.BfmCfg(in_rate=int(cfg["in_rate"]), nco_freq=int(cfg["nco_freq"]), audio_rate=int(cfg["audio_rate"]), rf_bandwidth=float(cfg["rf"]),
                     af_bandwidth=float(cfg["af"]), volume=float(cfg["vol"]), squelch_db=float(cfg["sq"]), audio_stereo=int(cfg["stereo"]),
                     lsb_stereo=int(cfg["lsb"]), show_pilot=int(cfg["pilot"]))


def state(bank, ch, cfg) -> dict:
    s, p, n = bank.levels(ch)
    locked, level, fbits, pbits = bank.pilot(ch)
    # get_pilot_level() = 2 * m_pilot_level: the doubling is exact, halved again it is m_pilot_level's bits (0, subnormals aside)
    lv = np.float32(level) / np.float32(2)
    return {"sum": s, "peak": p, "count": n, "locked": int(locked), "open": bank.squelch_open(ch),
            "bits": np.array([lv.view(np.uint32), fbits, pbits], np.uint32)}


def run_gpu(case, splits=None, bank=None, iq=None):
    bank = bank or sa.BfmBank([gcfg(case["cfg"])])
    audio, sink, states = [], [], []
    for x in bc.cut(bc.inputs(case) if iq is None else iq, splits or case["splits"]):
        bank.feed([x])
        audio.append(bank.read(0))
        k = bank.read_sink(0)
        assert not np.any(k[:, 1])
        sink.append(k[:, 0].copy())
        states.append(state(bank, 0, case["cfg"]))
    return bank, {"audio": audio, "sink": sink, "states": states}


def check_open(got, want, cfg, what):
    for i, (g, w) in enumerate(zip(got["states"], want["states"])):
        assert g["open"] == (np.float32(w["sq_state"]) > np.float32(cfg["rf"]) / np.float32(20)), (what, i)


@pytest.mark.parametrize("case", bc.CASES, ids=[c["name"] for c in bc.CASES])
def test_case_equals_the_recording(gold, case):
    want = bc.golden_case(gold, case)
    _, got = run_gpu(case)
    bc.assert_equals_recording(got, want, case["name"], state_keys=("count", "locked", "peak"))
    check_open(got, want, case["cfg"], case["name"])


def test_design_products_equal_the_oracle(oracle):
    for case in bc.CASES[:4] + bc.CASES[-1:]:
        o = bc.OracleBfm(oracle, case["cfg"]).design()
        g = sa.BfmBank([gcfg(case["cfg"])]).design(0)
        assert g[0] == o[0] == 72 and g[3] == o[3] and g[6] == o[6], case["name"]
        for i in (1, 2, 5, 7):
            assert np.array_equal(g[i].view(np.uint32), o[i].view(np.uint32)), (case["name"], i)
        assert np.float32(g[4]) == np.float32(o[4])
    assert sa.BfmBank([gcfg(bc.CASES[-1]["cfg"])]).design(0)[6] == 38399


def _mixed():
    """11 channels, mono and stereo interleaved, each with its own feed lengths: three workgroups of the walk, waves that return at
    once next to waves that walk"""
    by = {c["name"]: c for c in bc.CASES}
    names = ["stereo_240k", "mono_250k", "lsb_384k", "show_pilot_mono", "squelch_bursts", "mono_240k_one_feed", "pilot_stops", "mono_250k",
             "pilot_19k045_48k", "show_pilot_stereo", "volume_clips"]
    return [by[n] for n in names]


def test_mono_and_stereo_channels_interleaved_in_one_handle(gold):
    cases = _mixed()
    assert len(cases) >= 9 and len({c["cfg"]["stereo"] for c in cases}) == 2
    bank = sa.BfmBank([gcfg(c["cfg"]) for c in cases])
    cuts = [bc.cut(bc.inputs(c), c["splits"]) for c in cases]
    rounds = max(len(x) for x in cuts)
    empty = np.zeros(0, np.int16)
    got = [{"audio": [], "sink": [], "states": []} for _ in cases]
    for r in range(rounds):
        bank.feed([x[r] if r < len(x) else empty for x in cuts])
        for c, x in enumerate(cuts):
            a, k = bank.read(c), bank.read_sink(c)
            if r < len(x):
                got[c]["audio"].append(a); got[c]["sink"].append(k[:, 0].copy()); got[c]["states"].append(state(bank, c, cases[c]["cfg"]))
            else:
                assert a.shape[0] == 0 and k.shape[0] == 0, (c, r)          # an empty feed: nothing out, state untouched
    ll = bank.last_launch()
    assert ll["kernel"] == "bfm_walk_kernel" and ll["grid"] == 3 and ll["block"] == 256 and ll["lds_bytes"] == 0, ll
    for c, case in enumerate(cases):
        bc.assert_equals_recording(got[c], bc.golden_case(gold, case), f"channel {c} {case['name']}", state_keys=("count", "locked", "peak"))


def test_reset_restores_a_fresh_handle(gold):
    for name in ("squelch_bursts", "stereo_250k"):
        case = {c["name"]: c for c in bc.CASES}[name]
        want = bc.golden_case(gold, case)
        bank, first = run_gpu(case)
        bc.assert_equals_recording(first, want, name, state_keys=("count", "locked", "peak"))
        bank.feed([bc.inputs(case)[: 2 * 777]])            # leave pending samples and a half-way state behind
        bank.reset()
        assert bank.levels(0) == (0.0, 0.0, 0) and not bank.squelch_open(0) and bank.pilot(0)[0] is False
        _, again = run_gpu(case, bank=bank)
        bc.assert_equals_recording(again, want, name + " after reset", state_keys=("count", "locked", "peak"))


def test_queued_device_feeds_equal_synced_feeds(gold):
    """feed_dev after feed_dev on device-resident pieces, nothing read in between: the carry of one feed is the next one's input on
    the device alone.  The last feed's audio and sink stream and the state behind all of them equal the recording's"""
    import torch
    for name in ("stereo_240k", "squelch_bursts", "lock_96k"):
        case = {c["name"]: c for c in bc.CASES}[name]
        want = bc.golden_case(gold, case)
        pieces = bc.cut(bc.inputs(case), case["splits"])
        dev = [torch.from_numpy(x.copy()).cuda() if x.size else torch.zeros(2, dtype=torch.int16, device="cuda") for x in pieces]
        torch.cuda.synchronize()
        bank = sa.BfmBank([gcfg(case["cfg"])])
        for t, x in zip(dev, pieces):
            bank.feed_dev([t.data_ptr()], [x.size // 2])
        got = {"audio": [bank.read(0)], "sink": [bank.read_sink(0)[:, 0].copy()], "states": [state(bank, 0, case["cfg"])]}
        last = {"audio": want["audio"][-1:], "sink": None, "sink_counts": want["sink_counts"][-1:], "sink_sha": want["sink_sha"][-1:],
                "states": want["states"][-1:]}
        bc.assert_equals_recording(got, last, name + " queued", state_keys=("count", "locked", "peak"))


def test_feed_bank_equals_feed_of_the_banks_output(oracle):
    """a small channelizer bank, 4 channels at 240 kS/s: feed_bank on the device equals feed() of what bank.read returned, and the
    oracle on the same samples"""
    fs, n_ch = 3_840_000, 4
    fcs = [-900_000 + 600_000 * c + 1371 * c for c in range(n_ch)]
    bank_dev = sa.ChannelizerBank(fs, [240000] * n_ch, fcs)
    bank_host = sa.ChannelizerBank(fs, [240000] * n_ch, fcs)
    cfgs, raws = [], []
    for c in range(n_ch):
        _modes, out_rate, ofs = bank_dev.info(c)
        cfg = bc._cfg(out_rate, nco_freq=-ofs, rf=12500.0, sq=-80.0, stereo=c % 2, lsb=(c // 2) % 2)
        raws.append(cfg); cfgs.append(gcfg(cfg))
    bfm, bfm_host = sa.BfmBank(cfgs), sa.BfmBank(cfgs)
    oras = [bc.OracleBfm(oracle, r) for r in raws]
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
            got, want = bfm.read(c), bfm_host.read(c)
            wa, ws = oras[c].feed(chans[c])
            assert got.shape[0] > 1000 and np.array_equal(got, want) and np.array_equal(got, wa), c
            assert np.array_equal(bfm.read_sink(c)[:, 0], ws), c
            assert bfm.pilot(c) == bfm_host.pilot(c)
