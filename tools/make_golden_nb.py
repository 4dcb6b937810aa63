#!/usr/bin/env python3
"""Generate tests/golden/nb_edges.npz from the REAL reference (oracle/_ref/libref.so, built by oracle/Makefile.ref) and this machine's
libm.  Data only, never reference source.

  python tools/make_golden_nb.py

1. For every depth array of tests/nb_cases.py (stored_inputs; rebuilt from seeds, not stored): the reference's
   negative_binomial_transfer (rsi.cpp:1120-1188), and the RDmedian and r it computes on its way (rsi.cpp:1127-1143), taken with the
   reference's own _median -- the restatement of the transform from the bin sums on is pinned to these answers.
2. The hard list: inputs of the realistic domain (half-integer medians 5 .. 100, half-integer MADs up to the median, m = 101, every sum
   0 .. 2^16 - 1: 1.3e9 of them) whose double 2 sqrt(r) log(..) lies within 8 units of its last place of the midpoint between two floats,
   on either side of it.  numpy's log finds the candidates (a window of 72 units), math.log -- the libm the reference links -- confirms
   each and gives the stored answer.  About 50 are expected (17 / 2^29 of the domain); up to 64 are stored, spread over the domain.
"""
import json
import math
import os
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from make_golden_per_base import write_npz  # noqa: E402  (same folder: the archive with fixed time stamps)

M = 101
SUMS = 1 << 16
KEEP = 64


def reference_scalars(R, rd):
    """RDmedian and r as negative_binomial_transfer computes them (rsi.cpp:1127-1143), each median the reference's own _median."""
    RDmedian = R.median(rd)
    ns = 31
    k = rd.size // ns
    mads = np.zeros(ns, dtype=np.float64)
    for j in range(ns):
        sub = rd[j::ns][:k]
        tmp = np.abs(sub.astype(np.float32).astype(np.float64) - RDmedian).astype(np.int32)    # RDtmp[k]=abs((float)RD[i]-RDmedian), an int array
        mads[j] = R.median(tmp)
    return RDmedian, RDmedian / R.median(mads)


def hard_list(nc):
    sums = np.arange(SUMS, dtype=np.float64)
    hits = []
    half = 1 << 28
    for med2 in range(10, 201):                      # medians 5.0 .. 100.0
        med = med2 / 2.0
        for mad2 in range(1, med2 + 1):              # MADs 0.5 .. the median
            mad = mad2 / 2.0
            r = med / mad
            q = (sums + 0.25) / (M * r - 0.5)
            t = 2.0 * math.sqrt(r) * np.log(np.sqrt(q) + np.sqrt(1.0 + q))
            low = t.view(np.int64) & ((1 << 29) - 1)
            for i in np.nonzero(np.abs(low - half) <= nc.HARD_D + 64)[0]:
                tv = nc.nbt(float(i), float(M), r)
                if nc.is_hard(tv):
                    hits.append((med, mad, int(i), tv))
        print(f"median {med}: {len(hits)} hard inputs so far", flush=True)
    return hits


def main():
    import oracle
    import nb_cases as nc
    R = oracle.Ref()
    names, Ts, meds, rs = [], [], [], []
    for name, rd, m in nc.stored_inputs():
        T = R.negative_binomial_transfer(rd, m)
        RDmedian, r = reference_scalars(R, rd)
        names.append(name)
        Ts.append(T)
        meds.append(RDmedian)
        rs.append(r)
        print(f"{name}: nb {T.size} m {m} RDmedian {RDmedian} r {r}", flush=True)
    hits = hard_list(nc)
    total = len(hits)
    if total > KEEP:
        hits = [hits[(k * total) // KEEP] for k in range(KEEP)]
    side = [(struct.unpack("<q", struct.pack("<d", h[3]))[0] & ((1 << 29) - 1)) - (1 << 28) for h in hits]
    assert min(side) < 0 < max(side) and all(abs(s) <= nc.HARD_D for s in side), side
    out = dict(names=np.array(json.dumps(names)), off=np.cumsum([0] + [a.size for a in Ts]).astype(np.int64), T=np.concatenate(Ts).astype(np.float32),
               RDmedian=np.array(meds, dtype=np.float64), r=np.array(rs, dtype=np.float64),
               hard_median=np.array([h[0] for h in hits], dtype=np.float64), hard_mad=np.array([h[1] for h in hits], dtype=np.float64),
               hard_sum=np.array([h[2] for h in hits], dtype=np.int64), hard_t=np.array([h[3] for h in hits], dtype=np.float64),
               hard_found=np.array([total, 200 * 201 // 2 - 45, SUMS], dtype=np.int64))
    path = os.path.join(ROOT, "tests", "golden", "nb_edges.npz")
    write_npz(path, out)
    print(f"{path}: {os.path.getsize(path) / 1024:.0f} KB, {len(names)} cases, {len(hits)} of {total} hard inputs")


if __name__ == "__main__":
    main()
