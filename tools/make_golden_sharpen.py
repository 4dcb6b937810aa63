#!/usr/bin/env python3
"""Generate tests/golden/sharpen_edges.npz from the REAL reference (oracle/_ref/libref.so, built by oracle/Makefile.ref): every job's
start and end after one and after two calls of its optimize_with_derivative (rsi.cpp:889-937), for every case of tests/sharpen_cases.py
but the group `crossed`.  Data only, never reference source.

  python tools/make_golden_sharpen.py

The inputs are rebuilt from the seeds in tests/sharpen_cases.py and are not stored.  Before a job reaches the reference the restatement
(sharpen_cases.refine) proves that no call's loops leave the vector dd: the reference indexes it out of range for a candidate whose
first call left end < start.
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
    import sharpen_cases as sh
    R = oracle.Ref()
    names, once, twice = [], [], []
    for c in sh.all_cases():
        if c.group == "crossed":
            continue
        rows = [[], []]
        for s, e, t in c.jobs:
            assert sh.stays_inside(sh.refine(c.depth, int(s), int(e), int(t))[2]), f"{c.name}: a call would leave dd"
            for k in (1, 2):
                rows[k - 1].append(R.optimize_with_derivative(c.depth, s, e, t, calls=k))
        names.append(c.name)
        once.append(np.array(rows[0], dtype=np.int32).reshape(-1, 2))
        twice.append(np.array(rows[1], dtype=np.int32).reshape(-1, 2))
        print(f"{c.name}: n {c.depth.size} jobs {len(c.jobs)}", flush=True)
    out = dict(names=np.array(json.dumps(names)), off=np.cumsum([0] + [a.shape[0] for a in once]).astype(np.int64),
               once=np.concatenate(once), twice=np.concatenate(twice))
    path = os.path.join(ROOT, "tests", "golden", "sharpen_edges.npz")
    write_npz(path, out)
    print(f"{path}: {os.path.getsize(path) / 1024:.0f} KB, {len(names)} cases")


if __name__ == "__main__":
    main()
