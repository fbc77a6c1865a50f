#!/usr/bin/env python3
"""Record what the reference's own DecimatorsFI (compiled where it lies by oracle/Makefile -> oracle/_ref/libsdrref.so,
wrapper oracle/ref_shim_f.cpp; strict IEEE, x86-64) makes of the "wrap" and "overflow" inputs of
tests/float_edge_cases.py: products with 32768 whose low 16 bits wrap, and products that no int32 holds (+-7e4, +-1e6,
+-3e38, +-inf, NaN), for the (log2, fcpos) of FD_GOLDEN_CASES in the blocks of FD_BLOCKS.  The fixture keeps the int16
outputs only; the inputs are rebuilt from their seeds.  Build container only:

    python tests/golden/make_golden_fdecim_edges.py
"""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests import float_edge_cases as fe  # noqa: E402


def main():
    ref = C.CDLL(os.path.join(ROOT, "oracle", "_ref", "libsdrref.so"))
    vp = C.c_void_p
    ref.ref_fdecim_new.restype = vp; ref.ref_fdecim_new.argtypes = [C.c_int] * 3
    ref.ref_fdecim_free.argtypes = [vp]
    ref.ref_fdecim_process.restype = C.c_int; ref.ref_fdecim_process.argtypes = [vp, C.c_int, C.c_int, vp, C.c_int32, vp]
    g = {}
    for name in fe.FD_KIND_INPUTS["fi"]:
        x = fe.FD_INPUTS[name]()
        for L, fc in fe.FD_GOLDEN_CASES:
            h = ref.ref_fdecim_new(0, 0, 16)
            outs = []
            for blk in fe.fd_blocks(x):
                blk = np.ascontiguousarray(blk)
                o = np.zeros(blk.size + 8, np.int16)
                k = ref.ref_fdecim_process(h, L, fc, blk.ctypes.data, blk.size, o.ctypes.data)
                outs.append(o[: 2 * k].copy())
            ref.ref_fdecim_free(h)
            g[f"fi_{name}_L{L}_fc{fc}"] = np.concatenate(outs)
    path = os.path.join(HERE, "fdecim_edges_golden.npz")
    np.savez_compressed(path, **g)
    print("written:", path, os.path.getsize(path), "bytes,", len(g), "arrays")


if __name__ == "__main__":
    main()
