"""CPU: bench.py --dump-outputs.  The writer keeps small arrays whole, converts int16 samples to float32 exactly, stays under
64 MB in all however much the step computed, and samples the same rows on every run; the launcher self-test workload
writes its step result through the same path."""
import json
import os
import subprocess
import sys

import numpy as np

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_budget_exact_values_and_fixed_sample(tmp_path):
    rng = np.random.default_rng(3)
    arrays = {f"ch{c}": rng.integers(-32768, 32768, (1 << 22, 2)).astype(np.int16) for c in range(4)}
    arrays["small"] = np.arange(-5, 5, dtype=np.int16).reshape(5, 2)
    arrays["demod"] = rng.standard_normal(1000).astype(np.float32)
    w1 = bench.dump_outputs(str(tmp_path / "a"), arrays)
    w2 = bench.dump_outputs(str(tmp_path / "b"), arrays)
    assert w1 == w2
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted(k + ".npy" for k in arrays)
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) < 64 * 1000 * 1000
    for k, a in arrays.items():
        got = np.load(tmp_path / "a" / (k + ".npy"))
        assert got.dtype == np.float32 and got.shape[1:] == a.shape[1:]
        assert np.array_equal(got, np.load(tmp_path / "b" / (k + ".npy")))
        kept, rows = w1[k]
        assert rows == a.shape[0] and kept == got.shape[0]
        if k in ("small", "demod"):
            assert kept == rows and np.array_equal(got, a.astype(np.float32))
        else:
            assert 0 < kept < rows
            # every kept row is one of the array's rows, I and Q together
            key = lambda v: v[:, 0].astype(np.int64) * 65536 + v[:, 1].astype(np.int64)
            assert np.isin(key(got), key(a)).all()


def test_launchcheck_dumps_its_last_step(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "launchcheck", "--steps", "4", "--warmup", "1",
                        "--dump-outputs", str(tmp_path)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == 4 and line["ms_per_step"] > 0
    got = np.load(tmp_path / "launchcheck_sum.npy")
    assert got.dtype == np.float64 and got.tolist() == [float(np.arange(1 << 16, dtype=np.int64).sum())]
