"""CPU: the 57 kHz mixer's cosine (sdrangel_amd/csrc/rds_mix.hpp, built for the host by tests/rds_mix_check.cpp).  Over 10^7 phases
the host libm's cos(3.0 * phase) lies inside rds_cos's enclosure; with mpmath, on 10^5 phases that include the neighbours of every
multiple of pi / 2 up to 32, rds_cos is within its stated bound RDS_COS_E = 1 ulp of the true value."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("rds_mix") / "rds_mix_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-I" + os.path.join(ROOT, "sdrangel_amd", "csrc"),
                           os.path.join(ROOT, "tests", "rds_mix_check.cpp"), "-o", out])
    return out


def test_the_host_cosine_lies_inside_the_enclosure(exe):
    outside, differ, maxdiff, unsure = subprocess.check_output([exe, "enclose", "10000000", "1"], text=True).split()
    print(f"outside {outside}, differing from rds_cos {differ}, largest difference {maxdiff} ulp, unsure samples {unsure} of 10^7")
    assert int(outside) == 0 and float(maxdiff) <= 1.0
    # with +-1 ulp of a double in front of a float rounding the expected rate is about 2^-28 per sample: a handful at most here
    assert int(unsure) <= 8


def _phases():
    rng = np.random.default_rng(57000)
    ph = list(rng.uniform(0.0, 2 * np.pi + 0.5, 100000 - 21 * 41).astype(np.float32))
    for k in range(0, 21):                       # 3 * phase next to k * pi / 2 <= 32: the floats around k * pi / 6, 20 either side
        f = np.float32(k * np.pi / 6)
        lo = f
        for _ in range(20):
            lo = np.nextafter(lo, np.float32(-1))
        for _ in range(41):
            ph.append(lo)
            lo = np.nextafter(lo, np.float32(100))
    return np.array(ph, np.float32)


def test_rds_cos_is_within_its_bound_of_the_true_cosine(exe):
    mp = pytest.importorskip("mpmath")
    mp.mp.prec = 200
    ph = _phases()
    assert ph.size == 100000
    out = subprocess.run([exe, "eval"], input="\n".join("%08x" % b for b in ph.view(np.uint32)) + "\n", text=True, capture_output=True, check=True).stdout.split()
    got = np.array([int(o, 16) for o in out], np.uint64).view(np.float64)
    worst, closest = 0.0, 1.0
    for f, g in zip(ph, got):
        t = 3 * mp.mpf(float(f))
        true = mp.cos(t)
        if true == 0:
            continue
        ulp = mp.mpf(2) ** (mp.floor(mp.log(abs(true), 2)) - 52)
        worst = max(worst, float(abs(mp.mpf(float(g)) - true) / ulp))
        closest = min(closest, float(abs(true)))
    print(f"largest error {worst:.4f} ulp; smallest |cos| among the arguments 2^{np.log2(closest):.1f}")
    assert worst < 1.0                            # RDS_COS_E
    assert closest < 2.0 ** -20                   # the zeros' neighbours were among them
