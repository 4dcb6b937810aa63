#!/usr/bin/env python3
"""Generate tests/golden/filter_edges.npz from the REAL reference (oracle/_ref/libref.so, built by oracle/Makefile.ref): the status array
its filterstatus (rsi.cpp:948-1047) leaves for every case of tests/filter_cases.py it can run.  Data only, never reference source.

  python tools/make_golden_filter.py

The inputs are rebuilt from the seeds in tests/filter_cases.py and are not stored.  The file holds names, offsets and answers: of every
case the positions whose status the reference changed (it only ever clears bins), so the million-bin cases cost a few bytes a run.
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
    import filter_cases as fc
    R = oracle.Ref()
    names, cleared = [], []
    for c in fc.golden_cases():
        assert c.status.min() <= 0 <= c.status.max() and (c.status == 0).any(), c.name    # the reference reads RDsum[-minlevel]
        got = R.filterstatus(c.T, c.status, c.dev)
        changed = np.nonzero(got != c.status)[0]
        assert (got[changed] == 0).all(), c.name
        names.append(c.name)
        cleared.append(changed.astype(np.int32))
        print(f"{c.name}: nb {c.T.size} cleared {changed.size}", flush=True)
    # positions as differences: runs of cleared bins become runs of ones
    out = dict(names=np.array(json.dumps(names)), off=np.cumsum([0] + [a.size for a in cleared]).astype(np.int64),
               cleared_diff=np.concatenate([np.diff(a, prepend=0) for a in cleared]).astype(np.int32))
    path = os.path.join(ROOT, "tests", "golden", "filter_edges.npz")
    write_npz(path, out)
    print(f"{path}: {os.path.getsize(path) / 1024:.0f} KB, {len(names)} cases")


if __name__ == "__main__":
    main()
