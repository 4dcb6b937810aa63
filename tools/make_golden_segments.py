#!/usr/bin/env python3
"""Generate tests/golden/segment_edges.npz from the REAL reference (oracle/_ref/libref.so, built by oracle/Makefile.ref): start, end,
type and score of its get_rsi_segments (rsi.cpp:1060-1117) for every case of tests/segment_cases.py.  Data only, never reference source.

  python tools/make_golden_segments.py

The inputs are rebuilt from the seeds in tests/segment_cases.py and are not stored: the file holds names, offsets and answers.
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
    import segment_cases as sg
    R = oracle.Ref()
    names, cols = [], [[], [], [], []]
    for c in sg.all_cases():
        assert sg.exact_condition(c), c.name
        got = R.get_rsi_segments(c.T, c.status, c.tmedian)
        assert got[0].size == len(c.runs), f"{c.name}: {got[0].size} segments for {len(c.runs)} runs"
        names.append(c.name)
        for col, a in zip(cols, got):
            col.append(a)
        print(f"{c.name}: nb {c.T.size} runs {len(c.runs)}", flush=True)
    out = dict(names=np.array(json.dumps(names)), off=np.cumsum([0] + [a.size for a in cols[0]]).astype(np.int64),
               start=np.concatenate(cols[0]).astype(np.int32), end=np.concatenate(cols[1]).astype(np.int32),
               type=np.concatenate(cols[2]).astype(np.int8), score=np.concatenate(cols[3]).astype(np.float64))
    path = os.path.join(ROOT, "tests", "golden", "segment_edges.npz")
    write_npz(path, out)
    print(f"{path}: {os.path.getsize(path) / 1024:.0f} KB, {len(names)} cases")


if __name__ == "__main__":
    main()
