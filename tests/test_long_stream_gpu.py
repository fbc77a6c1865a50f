"""GPU: the channel banks (sdrx_chan_bank_*, sdrx_chan24_bank_*, sdrx_decim24_*) at stream positions past 2^30, 2^31, 2^32 and 2^33,
bit-exact against the oracle chains.  Both banks address their work by absolute stream position (Group::T in sdrx_chan.hip,
WEngine::T in sdrx_wide.hip) and the kernels do 64-bit arithmetic on it by hand; a receiver at 61.44 MS/s passes 2^32 in 70 s.

The stream is P | B | B | ... (tests/long_stream_cases.py): from repetition 2 on every chain repeats its output (W2, proved by
tests/test_long_stream.py), so the banks are fed the device-resident block over and over -- 16 repetitions per travel feed -- and
compared with W2 wherever they are.  Each bank makes the journey twice: once with a single feed that holds the threshold strictly
inside, once with the ragged cuts over the repetitions around it, where the cut N - len(P) ends one feed exactly on the threshold.

Every repetition writes the same samples to the same places of the output buffers, so what a feed left there would pass for the
next one's output: every region a feed has written is overwritten with POISON before the next feed."""
import time
from collections import defaultdict

import numpy as np
import pytest

import sdrangel_amd as sa
from tests import bank_path_cases as B
from tests import long_stream_cases as L
from tests import oracle_py as orc
from tests.test_chan_gpu import assert_engine

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

POISON = 0x5A


class _Raw:
    """device memory of the library as torch sees it"""

    def __init__(self, ptr, nbytes):
        self.__cuda_array_interface__ = dict(shape=(nbytes,), typestr="|u1", data=(ptr, False), version=2)


class Buffers:
    """P, B and Brep (B tiled R times) on the device"""

    def __init__(self, case):
        self.t = {"p": torch.from_numpy(case["p"]).cuda(), "b": torch.from_numpy(case["b"]).cuda()}
        self.t["brep"] = self.t["b"].repeat(L.R)
        self.sample_bytes = 2 * case["b"].itemsize
        # the libraries run on streams of their own, not ordered against torch's: the data is complete before they are pointed at it
        torch.cuda.synchronize()

    def ptr(self, which, a=0):
        return self.t[which].data_ptr() + self.sample_bytes * a


class Dut:
    """What a journey needs of a handle: feed device samples; per channel count, take or drop what the feeds produced; poison
    every output region written since the last poison (all channels taken or dropped: their regions start at the buffer's base)."""
    accumulates = False                                    # outputs queue up over feeds until taken

    def __init__(self):
        self.dirty = defaultdict(int)

    def take(self, c):
        n = self.count(c)
        self.dirty[c] = max(self.dirty[c], n)
        return self._read(c, n)

    def drop(self):
        for c in range(self.n_ch):
            self.dirty[c] = max(self.dirty[c], self.count(c))
            self._skip(c)

    def poison(self):
        self.h.sync()
        for c, n in self.dirty.items():
            if n:
                torch.as_tensor(_Raw(self._base(c), n * self.out_bytes), device="cuda").fill_(POISON)
        self.dirty.clear()
        torch.cuda.synchronize()

    def _skip(self, c):
        pass


class Bank16(Dut):
    accumulates, out_bytes = True, 4

    def __init__(self, case):
        super().__init__()
        ch = case["case"]["channels"]
        self.h = sa.ChannelizerBank(case["case"]["in_rate"], [r for r, _ in ch], [f for _, f in ch])
        for c, (modes, out_rate, ofs) in enumerate(case["plans"]):
            m, r, o = self.h.info(c)
            assert np.array_equal(m, modes) and (r, o) == (out_rate, ofs), c

    n_ch = property(lambda self: self.h.n_ch)

    def feed(self, ptr, n):
        self.h.feed_dev(ptr, n)

    def count(self, c):
        return self.h.available(c)

    def _read(self, c, n):
        return self.h.read(c)

    def _skip(self, c):
        self.h.skip(c)

    def _base(self, c):
        return self.h.last_dev(c)[0]                       # the queue is empty: the last feed's offset in it is 0


class Bank24(Dut):
    out_bytes = 8

    def __init__(self, case):
        super().__init__()
        self.h = sa.ChannelizerBank24(L.IN_RATE24, [r for r, _ in case["channels"]], [f for _, f in case["channels"]])
        self.n_ch = len(case["channels"])
        for c, (modes, out_rate, ofs) in enumerate(case["plans"]):
            m, r, o = self.h.info(c)
            assert np.array_equal(m, modes) and (r, o) == (out_rate, ofs), c

    def feed(self, ptr, n):
        self.h.feed_dev(ptr, n)

    def count(self, c):
        return self.h.out_dev(c)[1]

    def _read(self, c, n):
        out = np.empty(2 * n, np.int32)
        assert sa.lib().sdrx_chan24_bank_read(self.h._h, c, out.ctypes.data, n) == n
        return out

    def _base(self, c):
        return self.h.out_dev(c)[0]


class Decim24(Dut):
    n_ch, out_bytes = 1, 8

    def __init__(self, case, log2, fcpos, bits):
        super().__init__()
        self.h = sa.Decimators24(log2, fcpos, bits)
        self.out = torch.empty(2 * ((L.R * case["n"] >> log2) + 1), dtype=torch.int32, device="cuda")
        self.k = 0
        torch.cuda.synchronize()

    def feed(self, ptr, n):
        self.k = self.h.decimate_dev(ptr, n, self.out.data_ptr())

    def count(self, c):
        return self.k

    def _read(self, c, n):
        self.h.sync()
        return self.out[: 2 * n].cpu().numpy()

    def _base(self, c):
        return self.out.data_ptr()


def _pow2(x):
    return f"2^{x.bit_length() - 1}"


class Journey:
    """one handle on its way along P | B | B | ...; `pos` = samples fed = the absolute position of the next one"""

    def __init__(self, dut, case, buf, label, pos=0):
        self.dut, self.case, self.buf, self.label, self.pos = dut, case, buf, label, pos
        self.n, self.p_len, self.cuts = case["n"], case["p"].size // 2, case["cuts"]
        self.depths = dict(enumerate(case["depths"]))

    @property
    def reps(self):
        return (self.pos - self.p_len) // self.n

    def W(self, w):
        return {c: W[w] for c, W in enumerate(self.case["W"])}

    def _feed(self, which, a, n):
        self.dut.feed(self.buf.ptr(which, a), n)
        self.pos += n

    def check(self, what, c, got, want, start, k=None, sizes=None):
        """got == want, or a message that says which position was hit: `start` = absolute input position of the first feed compared"""
        if got.size == want.size and np.array_equal(got, want):
            return
        d = self.depths[c]
        m = min(got.size, want.size)
        bad = np.nonzero(got[:m] != want[:m])[0]
        i = int(bad[0]) // 2 if bad.size else m // 2
        if k is None:
            k = int(np.searchsorted(np.cumsum(sizes), i, side="right"))
        o = (start >> d) + i
        pytest.fail(f"{self.label}: {what}, feed {k}, channel {c} (depth {d}): {got.size // 2} outputs for {want.size // 2} expected, "
                    f"{bad.size} of {m} values differ, the first at output {i} of the comparison = absolute output {o} ({o:#x}) "
                    f"<-> absolute input position {o << d} ({o << d:#x}); the comparison starts at input {start} ({start:#x}), "
                    f"got {got[2 * i: 2 * i + 2].tolist()} for {want[2 * i: 2 * i + 2].tolist()}")

    def prefix(self):
        self._feed("p", 0, self.p_len)
        for c, W in enumerate(self.case["W"]):
            self.check("prefix", c, self.dut.take(c), W[0][0], 0, k=0)
        self.dut.poison()

    def rep(self, what, want=None, accumulate=False):
        """one repetition cut at the ragged boundaries; want = per channel the expected output of every feed (default W2)"""
        want = want or self.W(2)
        start0, have = self.pos, dict.fromkeys(want, 0)
        for k, (a, e) in enumerate(zip(self.cuts, self.cuts[1:])):
            start = self.pos
            self._feed("b", a, e - a)
            for c, segs in want.items():
                have[c] = have[c] * accumulate + segs[k].size // 2
                n = self.dut.count(c)
                assert n == have[c], (f"{self.label}: {what}, feed {k} (input {start:#x}..{self.pos:#x}), channel {c} "
                                      f"(depth {self.depths[c]}): {n} outputs available, {have[c]} expected")
            if not accumulate:
                for c, segs in want.items():
                    self.check(what, c, self.dut.take(c), segs[k], start, k=k)
                self.dut.poison()
        if accumulate:
            for c, segs in want.items():
                self.check(what, c, self.dut.take(c), np.concatenate(segs), start0, sizes=[s.size // 2 for s in segs])
            self.dut.poison()

    def travel_to(self, reps):
        """whole-Brep feeds, then whole-B feeds, until `reps` repetitions are fed; nothing is read"""
        assert (self.pos - self.p_len) % self.n == 0 and self.reps <= reps
        while self.reps + L.R <= reps:
            self._feed("brep", 0, L.R * self.n)
            self.dut.drop()
        while self.reps < reps:
            self._feed("b", 0, self.n)
            self.dut.drop()
        self.dut.poison()

    def straddle(self, x):
        """one Brep feed with x strictly inside it"""
        self.travel_to(x // self.n - L.R // 2)
        start = self.pos
        self._feed("brep", 0, L.R * self.n)
        assert start < x < self.pos
        what = f"one feed over {_pow2(x)} (input {start:#x}..{self.pos:#x})"
        for c, W in enumerate(self.case["W"]):
            one = np.concatenate(W[2])
            n = self.dut.count(c)
            assert n == L.R * one.size // 2, f"{self.label}: {what}, channel {c} (depth {self.depths[c]}): {n} outputs available"
            got = self.dut.take(c)
            if not (got.reshape(L.R, -1) == one).all():
                self.check(what, c, got, np.tile(one, L.R), start, k=0)
        self.dut.poison()

    def edge(self, x):
        """the ragged cuts over the repetitions before x, around x (a feed ends on x, the next begins there) and after x"""
        self.travel_to(x // self.n - 2)
        self.rep(f"repetition before {_pow2(x)}")
        assert self.pos + self.n - self.p_len == x and self.n - self.p_len in self.cuts
        self.rep(f"repetition with a feed boundary on {_pow2(x)}", accumulate=self.dut.accumulates)
        self.rep(f"repetition after {_pow2(x)}")


def begin(dut, case, buf, label):
    """prefix and two repetitions: plain oracle parity, and the baseline W2 at a small position"""
    j = Journey(dut, case, buf, label)
    j.prefix()
    j.rep("repetition 1", want=j.W(1))
    j.rep("repetition 2 (baseline)")
    return j


def checkpoint(j):
    """The state carries T as 64 bits, and a fresh bank that is given it goes on as the first one does.  (What the two produce
    cannot tell: T modulo 2^32 has the same phase at every depth.  The state's own words can: [magic, n_groups], then per group
    [T, n_streams] and the histories, sdrx_chan.hip.)"""
    lib, h = sa.lib(), j.dut.h
    st = np.zeros(lib.sdrx_chan_bank_state_bytes(h._h), np.uint8)
    assert lib.sdrx_chan_bank_get_state(h._h, st.ctypes.data) == 0
    assert st[8:16].view(np.int64)[0] == 1 and st[16:24].view(np.int64)[0] == j.pos > 1 << 32, (j.label, st[:24].view(np.int64), j.pos)
    fresh = Bank16(j.case)
    assert lib.sdrx_chan_bank_set_state(fresh.h._h, st.ctypes.data) == 0
    back = np.zeros_like(st)
    assert lib.sdrx_chan_bank_get_state(fresh.h._h, back.ctypes.data) == 0 and np.array_equal(back, st), j.label
    j2 = Journey(fresh, j.case, j.buf, j.label + "/restored", pos=j.pos)
    j.rep("repetition after the checkpoint")
    j2.rep("repetition after the checkpoint")
    fresh.h.close()


def dynamic(j):
    """add_channel and reconfigure past 2^32: their groups start an epoch at T = 0 beside the old group at T > 2^32"""
    h, case = j.dut.h, j.case
    assert j.pos > 1 << 32 and h.group_count == 1
    moved, plans = 3, {}
    new = h.add_channel(48000, 7_654_321)
    plans[new] = orc.chan_plan(case["case"]["in_rate"], 48000, 7_654_321)
    h.reconfigure(moved, 48000, 2_000_000)
    plans[moved] = orc.chan_plan(case["case"]["in_rate"], 48000, 2_000_000)
    assert new == len(case["W"]) and h.group_count == 3
    chains = {}
    for c, (modes, out_rate, ofs) in plans.items():
        m, r, o = h.info(c)
        assert np.array_equal(m, modes) and (r, o) == (out_rate, ofs), c
        chains[c], j.depths[c] = orc.Chain(modes), len(modes)

    def segs(c):                                            # a fresh chain from zero state, fed what the bank is fed
        return [chains[c].feed(case["b"][2 * a: 2 * e]) for a, e in zip(j.cuts, j.cuts[1:])]

    j.rep("repetition after add_channel and reconfigure", want={**j.W(2), new: segs(new), moved: segs(moved)})
    h.remove_channel(new)
    assert h.group_count == 2
    j.rep("repetition after remove_channel", want={**j.W(2), moved: segs(moved)})
    assert h.available(new) == 0


@pytest.mark.parametrize("engine", B.ENGINES)
@pytest.mark.parametrize("name", list(L.BANKS16))
def test_bank16_past_2_33(name, engine, monkeypatch):
    monkeypatch.setenv("SDRX_CHAN_ENGINE", engine)
    options = B.OPTIONS[L.BANKS16[name]["options"]]
    if options:
        monkeypatch.setenv("SDRX_CHAN_MAX_LEVELS", str(options[0]))
        monkeypatch.setenv("SDRX_CHAN_LDS_KB", str(options[1]))
    else:
        monkeypatch.delenv("SDRX_CHAN_MAX_LEVELS", raising=False)
        monkeypatch.delenv("SDRX_CHAN_LDS_KB", raising=False)
    case = L.bank16(name)
    buf = Buffers(case)
    for kind in ("straddle", "edge"):
        t0 = time.perf_counter()
        dut = Bank16(case)
        j = begin(dut, case, buf, f"{name}/{engine}/{kind}")
        assert_engine(dut.h, engine)
        for x in L.THRESHOLDS16:
            getattr(j, kind)(x)
            if kind == "edge" and x == 1 << 32:
                checkpoint(j)
        assert j.pos > 1 << 33
        if kind == "edge" and name == "cfg3":
            dynamic(j)
        dut.h.close()
        print(f"{j.label}: {j.pos} samples, {time.perf_counter() - t0:.2f} s")


def run24(make, case, label):
    buf = Buffers(case)
    for kind in ("straddle", "edge"):
        t0 = time.perf_counter()
        dut = make()
        j = begin(dut, case, buf, f"{label}/{kind}")
        t1 = time.perf_counter()
        j.travel_to(j.reps + L.R)
        print(f"{j.label}: one travel feed of {L.R * j.n} samples, {1e3 * (time.perf_counter() - t1):.2f} ms")
        for x in L.THRESHOLDS24:
            getattr(j, kind)(x)
        assert j.pos > 1 << 32
        dut.h.close()
        print(f"{j.label}: {j.pos} samples, {time.perf_counter() - t0:.2f} s")


def test_bank24_past_2_32():
    """ChannelizerBank24.feed_dev on {int32, int32} input: pass-through, 1, 6, 7, 12 and 13 stages (one to three passes)"""
    case = L.bank24()
    run24(lambda: Bank24(case), case, "bank24")


@pytest.mark.parametrize("log2,fcpos,bits", L.DECIM24)
def test_decim24_past_2_32(log2, fcpos, bits):
    """Decimators24.decimate_dev on int16 input (n_out derived from T), whole groups per feed"""
    case = L.decim24(log2, fcpos, bits)
    run24(lambda: Decim24(case, log2, fcpos, bits), case, case["name"])
