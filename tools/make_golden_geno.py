#!/usr/bin/env python
"""Generate tests/golden/geno_edges.npz from the REAL reference (oracle/_ref/libref.so, built by oracle/Makefile.ref): for every
case of tests/geno_cases.py whose ranges all span less than 10^6 -- the reference's _median allocates one counter per unit of
span -- and every job of it, the reference's own _median and _interquartilerange of the body's values and of the flank's (NaN
for an empty range).  Recorded results only.

Usage: python tools/make_golden_geno.py   (needs oracle/_ref: make -f oracle/Makefile all)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import geno_cases as gc
    import oracle
    ref = oracle.Ref()
    out = {}
    for name, case in gc.cases().items():
        if gc.is_wide(case):
            print(name, "left out: a range spans 10^6 or more")
            continue
        vals = gc.golden_ranges(case)
        out[name + ".med"] = np.array([np.nan if v is None else ref.median(v) for v in vals], dtype=np.float64)
        out[name + ".iqr"] = np.array([np.nan if v is None else ref.iqr(v) for v in vals], dtype=np.float64)
        print(name, len(vals), "ranges")
    path = os.path.join(ROOT, "tests", "golden", "geno_edges.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
