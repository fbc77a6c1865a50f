"""CPU: tests/datv_oracle.cpp, the scalar restatement of DATVDemod::feed down to p_symbols that the GPU tests compare the bank with.

Without the reference: the oracle equals the recordings tests/golden/datv_golden.npz and datv_random_golden.npz (made by
tests/golden/make_golden_datv.py from the reference's own NCO, fftfilt and leansdr classes) for every case and every feed -- the
design words, the digests of the coefficients and the three tables, the soft symbols, the constellation points, (freq, ss, mer)
of every measurement and the state's words, as they are for the short cases and as sha256 for the long ones; fed whole it equals
itself fed by a case's cuts; the cases reach every branch of the issue's list and the draw keeps its shares, asserted on the
oracle's counters.  The tables and the recorded mer come from the recording machine's libm: a different libm here shows in these
tests, not on the GPU.

With the reference (`ref`): the recorder is built and run, the oracle equals it feed by feed, and the recorder stepped by
DATVDemod::feed's own rule equals itself stepped every 37 samples."""
import os
import sys

import numpy as np
import pytest

from tests import datv_cases as dc

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_golden_datv as mk  # noqa: E402

REF = "/root/reference"
RANDOM = [dc.CUT_STREAM] + dc.random_cases()


@pytest.fixture(scope="module")
def oracle():
    return dc.build_oracle()


@pytest.fixture(scope="module")
def gold():
    out = {}
    for path in (dc.GOLDEN, dc.RANDOM_GOLDEN):
        g = np.load(path)
        out.update({k: g[k] for k in g.files})
    return out


@pytest.fixture(scope="module")
def runs(oracle):
    """every case through the oracle with its own cuts and its own tables, once"""
    out = {}
    for c in dc.CASES + RANDOM:
        o = dc.OracleDatv(oracle, c["cfg"])
        tables = o.tables()
        o.close()
        out[c["name"]] = dict(dc.run_oracle(oracle, c), tables=tables)
    return out


def assert_equals_recording(got: dict, gold: dict, case: dict, full: bool):
    name = case["name"]
    assert dc.sha(dc.inputs(case)) == str(gold[name + "/in_sha256"])
    assert got["design"][:11] == gold[name + "/design"].tolist()
    assert dc.table_digests(got["tables"]) == gold[name + "/tables_sha256"].tolist()
    feeds = got["feeds"]
    assert [[f["cost"].size, f["points"].size // 2, f["meas"].size] for f in feeds] == gold[name + "/counts"].tolist()
    for i, f in enumerate(feeds):
        assert f["state"] == gold[name + "/state"][i].tolist(), (name, "feed", i)
    if full:
        m = dc.merged(feeds)
        assert np.array_equal(m["cost"], gold[name + "/cost"]) and np.array_equal(m["symbol"], gold[name + "/symbol"])
        assert np.array_equal(m["points"], gold[name + "/points"])
        assert np.array_equal(mk.meas3(m["meas"]).view(np.uint32), gold[name + "/meas"])
    else:
        want = gold[name + "/feeds_sha256"].tolist()
        assert [[dc.sha(f["cost"]), dc.sha(f["symbol"]), dc.sha(f["points"]), dc.sha(mk.meas3(f["meas"]))] for f in feeds] == want


@pytest.mark.parametrize("case", dc.CASES, ids=[c["name"] for c in dc.CASES])
def test_oracle_equals_the_recording(runs, gold, case):
    assert_equals_recording(runs[case["name"]], gold, case, full=case["n"] <= dc.FULL)


@pytest.mark.parametrize("case", RANDOM, ids=[c["name"] for c in RANDOM])
def test_oracle_equals_the_random_recording(runs, gold, case):
    assert_equals_recording(runs[case["name"]], gold, case, full=False)


def test_the_recordings_have_every_case(gold):
    assert {k.split("/")[0] for k in gold} == {c["name"] for c in dc.CASES + RANDOM}


@pytest.mark.parametrize("case", dc.CASES, ids=[c["name"] for c in dc.CASES])
def test_fed_whole_equals_fed_by_the_cuts(oracle, runs, case):
    whole = dc.run_oracle(oracle, case, splits=[case["n"]])["feeds"][0]
    dc.assert_same_feed(dc.merged(runs[case["name"]]["feeds"]), whole, case["name"])


def test_the_cases_reach_every_branch(runs):
    dc.assert_coverage([runs[c["name"]]["hits"] for c in dc.CASES])


def test_named_cases_reach_what_they_are_named_for(runs):
    assert runs["drift_reset_down"]["hits"]["drift_reset"] > 0 and runs["drift_reset_up"]["hits"]["drift_reset"] > 0
    assert runs["offset_past_limit"]["hits"]["drift_reset"] == 0 and runs["allow_drift"]["hits"]["drift_reset"] == 0
    assert runs["timing_fast"]["hits"]["clamp_high"] > 100 and runs["timing_slow"]["hits"]["clamp_low"] > 100
    assert runs["meas_100"]["hits"]["two_meas"] > 0 and runs["meas_128"]["hits"]["two_meas"] == 0
    assert sum(f["meas"].size for f in runs["meas_never"]["feeds"]) == 0
    assert runs["silence_then_full"]["hits"]["max_halvings"] >= 12
    assert runs["ratio_1p05_mu_negative"]["hits"]["fewer_taps"] > 0 and runs["ratio_1p05_linear"]["hits"]["mu_negative"] > 0
    assert runs["silence"]["hits"]["symbols"] > 0 and runs["silence"]["hits"]["halved"] == 0
    assert runs["ratio_8_taps64"]["hits"]["max_taps"] == 64 and runs["ratio_8_taps63"]["hits"]["max_taps"] == 63
    for name in ("omega_300_no_symbol", "omega_300_linear"):            # chunks without a symbol: no point for them, measurements all the same
        r = runs[name]
        assert r["hits"]["no_symbol"] > 30 and sum(f["points"].size // 2 for f in r["feeds"]) == r["feeds"][-1]["state"][22] - r["hits"]["no_symbol"]
    assert sum(f["meas"].size for f in runs["omega_300_no_symbol"]["feeds"]) > 60 and runs["omega_300_no_symbol"]["hits"]["two_meas"] > 0
    assert sum(h["hits"]["no_symbol"] for n, h in runs.items() if not n.startswith("omega_300")) == 0


def test_the_design_spans_the_issues_ranges(runs):
    """rrc_steps from 53 down to 8, taps per symbol from 3 to the limit of 64, meas_decimation 100, 128, 300 and more than the stream"""
    d = {n: dict(zip(dc.DESIGN_FLOATS + dc.DESIGN_INTS, runs[n]["design"])) for n in dc.BY_NAME}
    taps = lambda n: -(-d[n]["ncoeffs"] // d[n]["rrc_steps"])
    assert d["ratio_1p2_taps3"]["rrc_steps"] == 53 and taps("ratio_1p2_taps3") == 3
    assert d["ratio_8_taps63"]["rrc_steps"] == 8 and taps("ratio_8_taps63") == 63
    assert d["ratio_8_taps64"]["rrc_steps"] == 8 and d["ratio_8_taps64"]["ncoeffs"] == 507 and taps("ratio_8_taps64") == 64      # the limit create admits
    assert taps("ratio_2_taps55") == 55 and d["ratio_2"]["rrc_steps"] == 32
    assert [d[n]["meas_decimation"] for n in ("meas_100", "meas_128", "rrc", "meas_never")] == [100, 128, 300, 200000]
    assert {d["mod_" + m]["nsymbols"] for m in dc.MOD_NAMES} == {2, 4, 8, 16, 32, 64, 256}
    assert d["linear"]["readahead"] == 1 and d["nearest"]["readahead"] == 0 and d["rrc"]["readahead"] == d["rrc"]["ncoeffs"] - 1


def test_the_draw_keeps_its_shares(runs):
    cases = dc.random_cases()
    dc.assert_random_shares(cases, [runs[c["name"]]["hits"] for c in cases])


def test_configurations_the_bank_refuses_are_refused_by_the_oracle(oracle):
    for kw in (dict(notch_filters=1), dict(modulation=dc.APSK16, fec=dc.FEC12), dict(modulation=dc.APSK32, fec=dc.FEC23), dict(rolloff=0.0),
               dict(rolloff=0.01, excursion=40), dict(symbol_rate=125000, excursion=40), dict(symbol_rate=125000, excursion=30, rolloff=0.339), dict(finfo=50000.0), dict(symbol_rate=2000000)):
        s = dc.as_struct(dc.cfg(**kw))
        assert not oracle.dto_create(dc.C.byref(s), None, None, None, None), kw


ref = pytest.mark.skipif(not mk.available(REF), reason="needs the reference tree and the Qt headers")


@pytest.fixture(scope="module")
def recorder():
    return mk.build_recorder(REF)


@ref
@pytest.mark.parametrize("case", dc.CASES[::4] + RANDOM[::10], ids=[c["name"] for c in dc.CASES[::4] + RANDOM[::10]])
def test_oracle_vs_rebuilt_recorder(recorder, runs, case):
    x = dc.inputs(case)
    r = mk.record(recorder, case, x)
    got = runs[case["name"]]
    assert got["design"][:11] == r["design"]
    for g, w in zip(got["tables"], r["tables"]):
        assert g.size == w.size and np.array_equal(g.view(np.uint8), w.view(np.uint8))
    for i, (fo, fr) in enumerate(zip(got["feeds"], r["feeds"])):
        assert np.array_equal(fo["cost"], fr["cost"]) and np.array_equal(fo["symbol"], fr["symbol"]), (case["name"], i)
        assert np.array_equal(fo["points"], fr["points"]) and np.array_equal(mk.meas3(fo["meas"]), fr["meas"]), (case["name"], i)
        assert fo["state"] == fr["state"], (case["name"], i)


@ref
@pytest.mark.parametrize("name", ["rrc", "linear", "meas_100", "ratio_1p2", "drift_reset_down"])
def test_the_symbols_do_not_depend_on_when_the_scheduler_steps(recorder, name):
    """DATVDemod::feed's rule, (m_lngReadIQ + 1) >= writable(), against a step every 37 samples: one stream of everything"""
    case = dc.BY_NAME[name]
    x = dc.inputs(case)
    a = mk.record(recorder, case, x, splits=[case["n"]])["feeds"][0]
    b = mk.record(recorder, case, x, splits=[case["n"]], step_every=37)["feeds"][0]
    assert a["cost"].size > 1000
    for key in ("cost", "symbol", "points", "meas"):
        assert np.array_equal(a[key], b[key]), (name, key)
    assert a["state"] == b["state"]
