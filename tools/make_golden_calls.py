#!/usr/bin/env python3
"""Generate tests/golden/calls_edges.npz from the REAL reference (oracle/_ref/libref.so, built by oracle/Makefile.ref): the answers of
areblockscnv, mergesegments, isitcnvwrap over one list in order, expand_coordinate and sd_filters for every case of tests/calls_cases.py.
Data only, never reference source.

  python tools/make_golden_calls.py

The inputs are rebuilt from the seeds in tests/calls_cases.py and are not stored.  Before a case reaches the reference the restatement
(calls_cases.restated) proves that every neighbourhood test its loops run stays inside the reference's arrays, and every edge refinement
inside its vector.  A block or merge case is one call of the reference's function.  detectcnv's own body is not a function that can be
called on a list, so a calls case asks the reference stage by stage, each stage on the list the restatement hands the one before:

  merged  mergesegments on the refined, ordered list            tested  isitcnvwrap for every index in order on the merged, ordered list
  expand  expand_coordinate at every junction and call edge     kept    sd_filters on the restatement's calls
  refined optimize_with_derivative, twice, per candidate (left out where its first call leaves end < start: the second then has no
          defined behaviour in the reference)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from make_golden_per_base import write_npz  # noqa: E402  (same folder: the archive with fixed time stamps)


def expand_positions(case, rec):
    import calls_cases as K
    pos = K.junction_positions([tuple(int(x) for x in r) for r in case.noncode], case.depth.size)
    pos += [c[k] for c in rec["tested"] for k in ("start", "end")]
    return sorted(set(pos))


def main():
    import oracle
    import calls_cases as K
    R = oracle.Ref()
    out = {}

    def put(name, part, L):
        out[f"{name}/{part}/i"], out[f"{name}/{part}/f"] = K.pack(L)

    for c in K.all_cases():
        n = c.depth.size
        r = K.restated(c)
        assert all(K.inside(t, n) for t in r[-1]["tests"]), f"{c.name}: a test would leave the reference's arrays"
        p = oracle.make_params(**c.P)
        if c.stage == "block":
            put(c.name, "out", R.areblockscnv(p, c.depth, c.status, c.span_all, c.RDmedian, c.cands))
        elif c.stage == "merge":
            put(c.name, "out", R.mergesegments(p, c.depth, c.RDmedian, c.cands))
        else:
            rec = r[-1]
            if not c.expect.get("crossed_refine"):      # (there the reference's second call leaves its vector: the restatement's rule judges it)
                assert all(K.sc.stays_inside(x) for x in rec["sharpen"]), f"{c.name}: an edge refinement would leave the reference's vector"
                refined = [dict(b, **dict(zip(("start", "end"), R.optimize_with_derivative(c.depth, b["start"], b["end"], b["type"])))) for b in rec["based"]]
                put(c.name, "refined", refined)
            put(c.name, "merged", R.mergesegments(p, c.depth, c.RDmedian, rec["sharpened"]))
            put(c.name, "tested", R.isitcnvwrap_in_order(p, c.depth, n, c.RDmedian, rec["merged"]))
            put(c.name, "kept", R.sd_filters(c.P["m"], c.RDmedian, c.RDsd, r[1]))
            if len(c.noncode):
                pos = expand_positions(c, rec)
                out[f"{c.name}/expand"] = np.stack([np.array(pos, dtype=np.int32), R.expand_coordinate(c.noncode, pos)])
        print(f"{c.name}: {c.stage}, n {n}, {len(c.cands)} candidates, {len(r[-1]['tests'])} tests restated", flush=True)
    path = K.GOLDEN
    write_npz(path, out)
    print(f"{path}: {os.path.getsize(path) / 1024:.0f} KB, {len(K.all_cases())} cases")


if __name__ == "__main__":
    main()
