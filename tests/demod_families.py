"""One face for the five demodulator-bank families (wfm, am, nfm, ssb, udpsrc), for the GPU tests that run all of them the same
way (tests/test_demod_random_gpu.py, tests/test_demod_queued_gpu.py).  Nothing is decided here: the cases and the oracle come from
tests/<family>_cases.py, the comparison rules (bit for bit; for udpsrc formats 2 and 3 the ruling of assert_streams) from
tests/test_<family>_gpu.py."""
from __future__ import annotations

import contextlib

import sdrangel_amd as sa
from tests import am_cases, nfm_cases, ssb_cases, udpsrc_cases, wfm_cases
from tests import test_am_gpu, test_nfm_gpu, test_ssb_gpu, test_udpsrc_gpu, test_wfm_gpu


class Family:
    """name: the family; cm: its cases module; gm: its GPU test module; spectrum: whether it has a second output stream"""

    def __init__(self, name, cm, gm, bank, oracle, spectrum, level_keys, flag):
        self.name, self.cm, self.gm, self.Bank, self.Oracle, self.spectrum = name, cm, gm, bank, oracle, spectrum
        self._level_keys, self._flag = level_keys, flag

    def gcfg(self, cfg):
        return self.gm.gcfg(cfg)

    def read(self, bank, ch) -> tuple:
        """the last feed's output streams of one channel"""
        return (bank.read(ch), bank.read_spectrum(ch)) if self.spectrum else (bank.read(ch),)

    def run_spans(self, L, cfg, spans) -> dict:
        """the oracle over a list of feeds, in the layout of <family>_cases.run_oracle (per-feed lists, then the final state)"""
        o = self.Oracle(L, cfg)
        if self.name == "udpsrc":
            res = {"feeds": [], "specs": [], "masks": []}
            for x in spans:
                p, s = o.feed(x)
                res["feeds"].append(p); res["specs"].append(s); res["masks"].append(o.last_open())
            res.update(o.state())
        elif self.name == "ssb":
            feeds = [o.feed(x) for x in spans]
            res = {"audio": [f[0] for f in feeds], "spec": [f[1] for f in feeds]}
        else:
            res = {"feeds": [o.feed(x) for x in spans]}
        if self.name != "udpsrc":
            res.update(zip(self._level_keys, o.levels()))
            res[self._flag[0]] = getattr(o, self._flag[1])()
        o.close()
        return res

    @staticmethod
    def last_feed(want: dict) -> dict:
        """the same result with every per-feed list cut down to its last entry"""
        return {k: (v[-1:] if isinstance(v, list) else v) for k, v in want.items()}

    def check_feeds(self, case, got, want, what):
        """got: what read() returned after each feed"""
        if self.name == "udpsrc":
            self.gm.assert_streams(case, [g[0] for g in got], [g[1] for g in got], want, what)
        elif self.name == "ssb":
            self.gm.assert_feeds_equal([g[0] for g in got], want["audio"], what + " audio")
            self.gm.assert_feeds_equal([g[1] for g in got], want["spec"], what + " spectrum")
        else:
            self.gm.assert_feeds_equal([g[0] for g in got], want["feeds"], what)

    def check_state(self, bank, ch, want, what):
        (self.gm.check_state if self.name == "udpsrc" else self.gm.check_levels)(bank, ch, want, what)


_LEVELS4 = ("magsq", "sum", "peak", "count")
FAMILIES = {f.name: f for f in (
    Family("wfm", wfm_cases, test_wfm_gpu, sa.WfmDemodBank, wfm_cases.OracleWfm, False, ("sum", "peak", "count"), ("open", "squelch_open")),
    Family("am", am_cases, test_am_gpu, sa.AmDemodBank, am_cases.OracleAm, False, _LEVELS4, ("open", "squelch_open")),
    Family("nfm", nfm_cases, test_nfm_gpu, sa.NfmDemodBank, nfm_cases.OracleNfm, False, _LEVELS4, ("open", "squelch_open")),
    Family("ssb", ssb_cases, test_ssb_gpu, sa.SsbDemodBank, ssb_cases.OracleSsb, True, _LEVELS4, ("active", "audio_active")),
    Family("udpsrc", udpsrc_cases, test_udpsrc_gpu, sa.UdpSrcBank, udpsrc_cases.OracleUdp, True, (), None),
)}


@contextlib.contextmanager
def naming(case: dict, ch: int, where: str = ""):
    """a failing assertion inside names the channel and prints the whole case (cfg, sig, n, seed, splits), so that it can be
    run again alone in a one-channel handle"""
    try:
        yield
    except AssertionError as e:
        raise AssertionError(f"{where} channel {ch}, case {case!r}:\n{e}") from e
