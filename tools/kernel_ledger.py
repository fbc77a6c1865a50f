#!/usr/bin/env python3
"""Which kernels of libsdrx.so has the GPU suite launched, and with what grid?

    python tools/kernel_ledger.py symbols sdrangel_amd/libsdrx.so
        the library's kernels, one per line, from its symbol table (the __device_stub__ host stubs); no GPU needed

    python tools/kernel_ledger.py fold [--lib sdrangel_amd/libsdrx.so] [--raw] DIR... > profiles/kernel_ledger.txt
        folds every *kernel_trace.csv under the DIRs -- what
            rocprofv3 --kernel-trace --output-format csv -d DIR -- python -m pytest -m gpu -q
        leaves, one file per traced process -- into one line per kernel of the library:
            <kernel> <TAB> <dispatches> <TAB> <X>x<Y>      the largest grid seen, in workgroups per dimension
            <kernel> <TAB> never                           not dispatched by any traced process
        --raw lists every kernel name of the trace as the profiler spelt it (other libraries' kernels included), for
        checking the normalisation.

Both sides are normalised to `name<template args>`: no return type, no namespace (anonymous ones included), no parameter
list, no blanks.  tests/test_kernel_ledger.py holds the committed ledger against the built library."""
from __future__ import annotations

import argparse
import csv
import os
import re
import shutil
import subprocess
import sys

STUB = "__device_stub__"


def _strip_params(s: str) -> str:
    """`f<a>(int, (anonymous namespace)::T*)` -> `f<a>`: drop the parenthesis group that ends the string"""
    if not s.endswith(")"):
        return s
    depth = 0
    for i in range(len(s) - 1, -1, -1):
        if s[i] == ")":
            depth += 1
        elif s[i] == "(":
            depth -= 1
            if depth == 0:
                return s[:i]
    return s


def _last_token(s: str) -> str:
    """drop a return type: what follows the last blank outside <> and ()"""
    depth, start = 0, 0
    for i, ch in enumerate(s):
        if ch in "<(":
            depth += 1
        elif ch in ">)":
            depth -= 1
        elif ch == " " and depth == 0:
            start = i + 1
    return s[start:]


def normalise(name: str) -> str:
    """a demangled kernel name, from the profiler or from nm -C, as `name<template args>`"""
    s = name.strip().strip('"')
    s = re.sub(r"\s*\[clone [^\]]*\]$", "", s)
    if s.endswith(".kd"):
        s = s[:-3]
    s = s.replace("(anonymous namespace)::", "").replace(STUB, "")
    s = _last_token(_strip_params(s).strip())
    s = re.sub(r"(?:[A-Za-z_]\w*::)+", "", s)                          # namespaces, of the name and inside the arguments
    s = re.sub(r"\([A-Za-z_][\w ]*\)(?=-?\d)", "", s)                   # `(int)3`, `(Mode)3` -> `3`
    s = re.sub(r"(?<=\d)(?:ull|ul|ll|u|l)(?=[,>])", "", s)              # `3u` -> `3`
    return s.replace(" ", "")


def _nm() -> str:
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    for cand in ("nm", "llvm-nm", os.path.join(rocm, "llvm", "bin", "llvm-nm")):
        path = shutil.which(cand)
        if path:
            return path
    raise RuntimeError("neither nm nor llvm-nm found")


def symbols(lib: str) -> list:
    """the kernels of a HIP shared library, normalised and sorted: every kernel has a host stub named __device_stub__<kernel>"""
    out = subprocess.run([_nm(), "-C", "--defined-only", lib], check=True, capture_output=True, text=True).stdout
    names = set()
    for line in out.splitlines():
        if STUB not in line:
            continue
        parts = line.split(None, 2)                                     # address, type, demangled name
        names.add(normalise(parts[2] if len(parts) == 3 else parts[-1]))
    return sorted(names)


def trace_files(dirs) -> list:
    found = []
    for d in dirs:
        if os.path.isfile(d):
            found.append(d)
            continue
        for root, _sub, files in os.walk(d):
            found += [os.path.join(root, f) for f in files if f.endswith("kernel_trace.csv")]
    return sorted(found)


def fold(files, norm=normalise) -> dict:
    """{kernel: [dispatches, largest grid x, largest grid y]}, grids in workgroups, over all the trace files"""
    seen = {}
    for path in files:
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                name = row.get("Kernel_Name")
                if not name:
                    continue
                gx, gy = int(row["Grid_Size_X"]), int(row["Grid_Size_Y"])
                wx, wy = max(int(row["Workgroup_Size_X"]), 1), max(int(row["Workgroup_Size_Y"]), 1)
                e = seen.setdefault(norm(name), [0, 0, 0])
                e[0] += 1
                e[1] = max(e[1], -(-gx // wx))
                e[2] = max(e[2], -(-gy // wy))
    return seen


def ledger_lines(kernels, seen) -> list:
    launched = sum(1 for k in kernels if k in seen)
    lines = [f"# kernels in the library: {len(kernels)}; launched: {launched}; never: {len(kernels) - launched}",
             "# kernel <TAB> dispatches <TAB> largest grid in workgroups (x by y), or `never`"]
    for k in kernels:
        lines.append(f"{k}\t{seen[k][0]}\t{seen[k][1]}x{seen[k][2]}" if k in seen else f"{k}\tnever")
    return lines


def read_ledger(path: str) -> dict:
    """{kernel: (dispatches, grid x, grid y)}; a kernel marked `never` has 0 dispatches"""
    out = {}
    with open(path) as f:
        for line in f:
            line = line.rstrip("\n")
            if not line or line.startswith("#"):
                continue
            cols = line.split("\t")
            if cols[1] == "never":
                out[cols[0]] = (0, 0, 0)
            else:
                x, y = cols[2].split("x")
                out[cols[0]] = (int(cols[1]), int(x), int(y))
    return out


def main(argv=None) -> int:
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    sub = ap.add_subparsers(dest="cmd", required=True)
    p = sub.add_parser("symbols")
    p.add_argument("lib")
    p = sub.add_parser("fold")
    p.add_argument("--lib", default=os.path.join(here, "sdrangel_amd", "libsdrx.so"))
    p.add_argument("--raw", action="store_true")
    p.add_argument("dirs", nargs="+")
    a = ap.parse_args(argv)
    if a.cmd == "symbols":
        print("\n".join(symbols(a.lib)))
        return 0
    files = trace_files(a.dirs)
    if not files:
        print("no *kernel_trace.csv under " + " ".join(a.dirs), file=sys.stderr)
        return 1
    if a.raw:
        for k, (n, x, y) in sorted(fold(files, norm=lambda s: s).items()):
            print(f"{k}\t{n}\t{x}x{y}")
        return 0
    print("\n".join(ledger_lines(symbols(a.lib), fold(files))))
    return 0


if __name__ == "__main__":
    sys.exit(main())
