"""The DATV example (examples/filesource_to_datv.py: .sdriq -> FIFO -> channelizer bank -> feed_bank -> symbols and measurements as
.npy) runs on the GPU: each carrier yields about one soft symbol per symbol period, its files hold what the run returned, and the
receiver locks -- the first measurement's MER is under 3 dB, the last one's above 12 dB and the frequency estimate is small."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_example_locks_and_writes_its_files(tmp_path, capsys):
    spec = importlib.util.spec_from_file_location("filesource_to_datv", os.path.join(ROOT, "examples", "filesource_to_datv.py"))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    res = mod.main(str(tmp_path))
    assert "MER over time" in capsys.readouterr().out
    for c, fm in enumerate(mod.SYMBOL_RATES):
        want = fm * mod.SECONDS
        assert 0.9 * want < res["symbols"][c] < 1.02 * want, (c, res["symbols"][c], want)
        cost, symbol, meas = (np.load(p) for p in res["files"][c])
        assert cost.size == symbol.size == res["symbols"][c] and symbol.max() <= 3
        assert meas.size == res["meas"][c].size >= 15 and np.array_equal(meas["mer"], res["meas"][c]["mer"])
        # the estimates average over about 100 chunks and start from no signal power: MER climbs for tens of thousands of samples.
        # Locked, at more than 26 dB of signal to noise, the error vector ends under a quarter of the symbol's amplitude: 12 dB
        assert meas["mer"][0] < 3.0 and meas["mer"][-1] > 12.0 and np.all(np.diff(meas["mer"][-5:]) > -1.0), (c, meas["mer"])
        assert np.abs(meas["freq"][-5:]).max() < 0.002, (c, meas["freq"][-5:])
