#!/usr/bin/env python3
"""Generate tests/golden/scan_edges.npz from the REAL reference (oracle/_ref/libref.so, built by oracle/Makefile.ref): the status array
of its rsistatus (rsi.cpp:1191-1259) for every case of tests/scan_cases.py whose answer is the reference's.  Data only, never
reference source.

  python tools/make_golden_scan.py

The inputs are rebuilt from the seeds in tests/scan_cases.py and are not stored.  Before a case reaches the reference the bounded
restatement (tests/scan_restatement.py) proves that none of its trimming walks leaves the array: the reference reads past it there.
One concatenated status array with offsets, keyed by the list of names: an archive of a few hundred tiny members is mostly headers.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from make_golden_per_base import write_npz  # noqa: E402  (same folder: the archive with fixed time stamps)


def main():
    import oracle
    import scan_cases as sc
    R = oracle.Ref()
    names, parts = [], []
    for c in sc.all_cases():
        if not c.ref:
            continue
        assert sc.walks_inside(c, R.exact_median), f"{c.name}: a trimming walk leaves the array"
        st = R.rsistatus(c.T, c.medint, c.RDmedian, c.tmedian, c.tlamda, c.Lmax)
        names.append(c.name)
        parts.append(st)
        print(f"{c.name}: nb {c.T.size} Lmax {c.Lmax} DEL bins {np.count_nonzero(st < 0)} DUP bins {np.count_nonzero(st > 0)}", flush=True)
    out = dict(names=np.array(json.dumps(names)), status=np.concatenate(parts),
               off=np.cumsum([0] + [a.size for a in parts]).astype(np.int64))
    path = os.path.join(ROOT, "tests", "golden", "scan_edges.npz")
    write_npz(path, out)
    print(f"{path}: {os.path.getsize(path) / 1024:.0f} KB, {len(names)} cases")


if __name__ == "__main__":
    main()
