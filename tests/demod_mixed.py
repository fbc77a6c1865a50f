"""The mixed-bank loop of the demodulator-bank GPU tests (tests/test_ssb_gpu.py, tests/test_udpsrc_gpu.py,
tests/test_demod_random_gpu.py): channels of different configurations and lengths in one handle, each cut by its own list."""
from __future__ import annotations

import numpy as np


def feed_rounds(bank, cuts, read, idle=None):
    """Round r feeds every channel its r-th span, or an empty array once its list has ended.  After each round read(bank, c)
    -- an array or a tuple of arrays -- is collected for every channel that was fed; a channel whose list has ended must
    report no samples (idle(bank, c) is its sample count, the rows of what read returns by default; its state is compared by
    the caller at the end, with an oracle that never saw the empty feeds).  Returns got[c][r]."""
    def rows(bank, c):
        out = read(bank, c)
        return sum(a.shape[0] for a in (out if isinstance(out, tuple) else (out,)))

    idle = idle or rows
    empty = np.zeros(0, np.int16)
    got = [[] for _ in cuts]
    for r in range(max(len(x) for x in cuts)):
        bank.feed([x[r] if r < len(x) else empty for x in cuts])
        for c, x in enumerate(cuts):
            if r < len(x):
                got[c].append(read(bank, c))
            else:
                assert idle(bank, c) == 0, (c, r)           # an empty feed: nothing out, state untouched
    return got
