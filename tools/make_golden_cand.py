#!/usr/bin/env python3
"""Generate tests/golden/cand_edges.npz from the REAL reference (oracle/_ref/libref.so, built by oracle/Makefile.ref): every tested
candidate as its isitcnvwrap + isitcnv judge it (rsi.cpp:101-287), for every case of tests/cand_cases.py but the groups without a
reference behaviour (cand_cases.NO_GOLDEN).  Data only, never reference source.

  python tools/make_golden_cand.py

The inputs are rebuilt from the seeds in tests/cand_cases.py and are not stored.  Before a record reaches the reference the restatement
(cand_cases.restate) proves that the reference's loops stay inside its arrays: a neighbourhood longer than the candidate, no value taken
past `capacity`, every index of the depth inside it.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from make_golden_per_base import write_npz  # noqa: E402  (same folder: the archive with fixed time stamps)

INTS = ("type", "status", "geno")
FLOATS = ("p1", "cnvmed", "cnvsd", "cnviqr", "refmed", "refsd", "refiqr")


def main():
    import oracle
    import cand_cases as cc
    R = oracle.Ref()
    names, counts, ints, floats = [], [], [], []
    for c in cc.all_cases():
        if not cc.in_golden(c):
            continue
        recs = cc.restated(c)
        p = oracle.make_params(**c.P)
        for ci in c.index:
            r = recs[ci]
            lo, hi = cc.reads(r)
            assert not r["empty"] and not r["past_capacity"], f"{c.name}[{ci}]: the reference would leave an array"
            assert (lo is None or lo >= 0) and (hi is None or hi < c.depth.size), f"{c.name}[{ci}]: a walk would leave the depth"
            g = R.isitcnvwrap(p, c.depth, c.span_all, c.RDmedian, c.cands, ci)
            ints.append([g[k] for k in INTS])
            floats.append([g[k] for k in FLOATS])
        names.append(c.name)
        counts.append(len(c.index))
        print(f"{c.name}: n {c.depth.size} candidates {len(c.cands)} tested {len(c.index)}", flush=True)
    out = dict(names=np.array(json.dumps(names)), off=np.cumsum([0] + counts).astype(np.int64), int_fields=np.array(json.dumps(INTS)),
               float_fields=np.array(json.dumps(FLOATS)), ints=np.array(ints, dtype=np.int32).reshape(-1, len(INTS)),
               floats=np.array(floats, dtype=np.float64).reshape(-1, len(FLOATS)))
    path = os.path.join(ROOT, "tests", "golden", "cand_edges.npz")
    write_npz(path, out)
    print(f"{path}: {os.path.getsize(path) / 1024:.0f} KB, {len(names)} cases, {len(ints)} records")


if __name__ == "__main__":
    main()
