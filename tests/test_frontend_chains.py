"""CPU: what the chains of tests/frontend_chains.py must reach, asserted on the oracle alone, so that a chain of
tests/test_frontend_queued_gpu.py cannot pass for the wrong reason: the state carried into the last span matters, the last
span is long enough, the hand-over after load_stages spans several calls, a bank queue grows while it holds samples, and the
spectrum sink has frames queued when its queue grows."""
import numpy as np
import pytest

from tests import frontend_chains as fc
from tests import oracle_py as orc
from tests import spectrum_cases as sc

CHAINS = fc.all_chains()
IDS = [c.name for c in CHAINS]


def n_outputs(chain, s, y):
    """outputs in y, the result of stream / channel s of a round: complex samples, except mono audio samples (audio tail),
    reals (the back-end's discriminator) and, for the spectrum sink, the bins of its frames"""
    if chain.name == "audiotail" or chain.name.startswith("spectrum") or (chain.name == "pipeline" and s >= 1):
        return y.size
    return y.size // 2


def stateless(chain, s):
    """a pass-through channel carries nothing, decimate1 is a shift per sample, and an SSB tail without the AGC threshold never
    leaves step value 0: its audio is silence whatever it carries"""
    if chain.name.startswith("decim_log0"):
        return True
    if chain.name == "audiotail":
        return chain.cfgs[s]["kind"] == 1 and not chain.cfgs[s]["agc_threshold_enable"]
    if chain.name.startswith("bank"):
        return len(bank_modes(chain, s)) == 0
    return False


def bank_modes(chain, s):
    return chain.modes[s] if chain.name.startswith("bank24") else fc.bank_model(chain).ch[s]["modes"]


def test_shape_of_a_chain():
    for unit in (1, 2, 8, 16):
        s = fc.SPANS(unit, 77)
        assert len(s) == 10 and s[:9] == [m if m <= 1 else unit * m for m in fc.HEAD] and s[9] == 77
        assert 0 in s and 1 in s and s[fc.BIG] >= 4.5 * max(s[:fc.BIG])
    assert fc.HEAD == __import__("tests.test_demod_queued_gpu", fromlist=["HEAD"]).HEAD
    for c in CHAINS:
        assert c.rounds == (6 if c.name == "pipeline" else 10), c
        for spans in c.spans:
            assert all(m % c.per == 0 for m in spans), c


@pytest.mark.parametrize("chain", CHAINS, ids=IDS)
def test_carried_state_matters_and_last_span_is_long_enough(chain):
    last = chain.want[-1]
    fresh = chain.run(first=chain.rounds - 1)[0]
    assert len(last) == len(fresh)
    streams = len(chain.spans)
    for s, (a, b) in enumerate(zip(last, fresh)):
        if streams > 1 and chain.spans[s][-1] == 0:        # the batch's empty stream of the last round
            assert a.size == 0 and chain.name == "decim_batch"
            continue
        # 512 outputs; 64 for the deepest channel of the bank (11 stages) and for what is deeper still in the 24-bit bank (12, 13)
        need = fc.DEEP_OUT if chain.name.startswith("bank") and len(bank_modes(chain, s)) >= max(fc.BANK_STAGES) else fc.LAST_OUT
        assert n_outputs(chain, s, a) >= need, (chain.name, s, n_outputs(chain, s, a))
        if stateless(chain, s):
            continue
        assert a.shape != b.shape or not np.array_equal(a.view(np.uint8), b.view(np.uint8)), (chain.name, s)


def test_transition_after_load_stages_spans_three_calls():
    c = fc.chain_decim_after_load()
    group = orc.lib().sdro_decim_group_int16(c.cfg[0], c.cfg[1])
    consumed = [(m // group) * (group // 2) for m in c.spans[0]]
    before, calls = 0, 0
    for r, n in enumerate(consumed):
        if before >= fc.HANDOVER:
            break
        calls += n > 0
        before += n
    assert calls >= 3, (calls, consumed)
    assert sum(consumed[:r - 1]) < fc.HANDOVER <= sum(consumed[:r]) and r < c.rounds, consumed    # it ends inside a call, more follow
    assert consumed[r - 1] > fc.HANDOVER                   # ... and the parallel kernels take over within that call
    # the stage states the other variant left matter to the chain's first outputs
    plain = orc.Decim(*c.cfg)
    first = np.concatenate([y[0] for y in c.want[:fc.BIG + 1]])
    assert not np.array_equal(first, np.concatenate([plain.process(c.segs(r)[0]) for r in range(fc.BIG + 1)]))


def test_a_bank_queue_grows_while_it_holds_samples():
    c = fc.chain_bank()
    m = fc.bank_model(c)
    assert [len(ch["modes"]) for ch in m.ch] == list(fc.BANK_STAGES)
    assert list(m.ch[5]["modes"][:7]) == list(m.ch[4]["modes"][:7]) and list(m.ch[3]["modes"][:3]) == list(m.ch[2]["modes"])
    held = [sum(c.want[r][ch].size // 2 for r in range(c.rounds - 1)) for ch in range(len(m.ch))]
    assert max(held) > fc.QUEUE0, held
    # it also grows in the middle: the big span alone overflows what the spans before it left room for
    before_big = [sum(c.want[r][ch].size // 2 for r in range(fc.BIG)) for ch in range(len(m.ch))]
    assert any(0 < b < fc.QUEUE0 < b + c.want[fc.BIG][ch].size // 2 for ch, b in enumerate(before_big)), before_big


def test_bank_chains_with_operations():
    c = fc.chain_bank_reconf()
    m = fc.bank_model(c)
    assert len(m.ch) == 4 and all(len(ch["modes"]) for ch in m.ch)
    feeds = [r for r in range(c.rounds) if r >= 2 and c.spans[0][r] > 0]
    assert len(feeds) == 7 and c.spans[0][2] == 0          # HEAD's empty span is feed 3: seven of the eight feeds launch
    # three groups per feed, a ring of four tables: it wraps at least five times
    assert 3 * len(feeds) // 4 >= 5
    assert list(m.ch[1]["modes"]) == [1, 2, 0]             # the reconfigured channel
    s = fc.chain_bank_skip()
    (r1, _, _, c1, n1), (r2, _, _, c2) = s.ops
    have1 = sum(s.want[r][c1].size // 2 for r in range(r1 + 1))
    assert (r1, r2) == (3, 5) and c1 != c2 and 0 < n1 < have1
    left = fc.bank_model(s)
    assert left.ch[c1]["q"].size // 2 == sum(y[c1].size // 2 for y in s.want) - n1
    assert left.ch[c2]["q"].size // 2 == sum(s.want[r][c2].size // 2 for r in range(r2 + 1, s.rounds))


@pytest.mark.parametrize("cfg", fc.SPECTRUM_CASES)
def test_spectrum_has_frames_queued_before_its_largest_span(cfg):
    c = fc.chain_spectrum(cfg)
    frames = [y[0].shape[0] for y in c.want]
    big = int(np.argmax(c.spans[0]))
    assert big == c.rounds - 1
    queued = sum(frames[:big])
    assert queued >= 1 and frames[big] > queued, frames
    if cfg[3] != sc.FIXED:                                 # the queue's initial room overflows with those frames in it
        assert (queued + frames[big]) * cfg[0] > fc.SPECTRUM_QUEUE0


def test_pipeline_produces_on_every_leg():
    c = fc.chain_pipeline()
    assert all(len(p[0]) == 5 and p[1] == 75000 for p in c.plans)
    frames = sum(y[1].shape[0] for y in c.want)
    assert frames >= 100 and all(c.want[-1][2 + k].size >= fc.LAST_OUT for k in range(4))
