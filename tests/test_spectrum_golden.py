"""The C restatement of SpectrumVis (tests/spectrum_oracle.c, the checker of the GPU sink) against the reference's own
SpectrumVis: every case of tests/spectrum_cases.py recorded by tests/golden/make_golden_spectrum.py into
tests/golden/spectrum_golden.npz (frame counts of every feed, frames bit for bit or their sha256).  Where the reference tree
and Qt are present, a `ref` test rebuilds the recorder and compares 200 random configurations and feed splits."""
import hashlib
import os

import numpy as np
import pytest

from tests import spectrum_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "spectrum_golden.npz")
REF = "/root/reference"


@pytest.fixture(scope="module")
def oracle():
    return sc.build_oracle()


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def _feeds(res):
    return [fr for kind, fr in res if kind == "frames"]


def test_golden_covers_every_case(golden):
    names = {k.split("/")[0] for k in golden.files}
    assert names == {c["name"] for c in sc.CASES}


@pytest.mark.parametrize("case", sc.CASES, ids=[c["name"] for c in sc.CASES])
def test_oracle_matches_reference_recording(oracle, golden, case):
    feeds = _feeds(sc.run_oracle(oracle, case))
    name = case["name"]
    assert [f.shape[0] for f in feeds] == golden[f"{name}/counts"].tolist()
    if f"{name}/frames" in golden.files:
        got = np.concatenate([f.reshape(-1) for f in feeds]).astype(np.float32)
        assert np.array_equal(got.view(np.int32), golden[f"{name}/frames"].view(np.int32))
    else:
        want = golden[f"{name}/sha256"].tolist()
        got = [hashlib.sha256(np.ascontiguousarray(f, np.float32).tobytes()).hexdigest() for f in feeds]
        assert got == want


def _random_case(rng):
    sizes = [64, 128, 256, 512, 1024, 2048, 4096]
    def cfg():
        return (int(rng.choice(sizes)), int(rng.integers(0, 50)), int(rng.choice([0, 1, 2, 3, 5, 10])),
                int(rng.integers(0, 3)), int(rng.integers(0, 6)), int(rng.integers(0, 2)))
    steps = []
    c0 = cfg()
    n_fft = c0[0]
    for _ in range(int(rng.integers(3, 10))):
        if rng.random() < 0.15:
            c = cfg(); n_fft = c[0]
            steps.append(("configure", c))
        else:
            n = int(rng.choice([1, n_fft - 1, n_fft + 1, int(rng.integers(1, 3 * n_fft)), int(rng.integers(1, 8 * n_fft))]))
            steps.append(("feed", max(n, 1), bool(rng.random() < 0.3), str(rng.choice(["noise", "tone", "min", "zero"]))))
    return {"name": "random", "cfg": c0, "steps": steps}


@pytest.mark.ref
@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "sdrgui", "dsp")), reason="no reference tree here")
def test_oracle_vs_rebuilt_recorder_random(oracle):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_golden_spectrum as mg
    if not mg.available(REF):
        pytest.skip("moc / Qt5Core not available")
    exe = mg.build_recorder(REF)
    rng = np.random.default_rng(20261016)
    for i in range(200):
        case = _random_case(rng)
        ins = sc.inputs(case, seed=i)
        want = mg.record(exe, case["cfg"], case["steps"], ins)
        o = sc.OracleSpectrum(oracle, case["cfg"])
        k = 0
        for s, iq in zip(case["steps"], ins):
            if s[0] == "configure":
                o.configure(s[1])
                continue
            got = o.feed(iq, s[2])
            w = want[k]; k += 1
            assert got.shape[0] == w.shape[0], (i, case)
            if got.shape[0]:
                assert np.array_equal(got.view(np.int32), w.view(np.int32)), (i, case)
        o.close()
