#!/usr/bin/env python3
"""Generate tests/golden/oracle_vs_ref.npz from the REAL reference (oracle/_ref/libref.so, built by
oracle/Makefile.ref).  Runs only where the reference has been compiled; the file holds data (the
reference's answers and the hashes of the seeded inputs), never reference source.

  python tools/make_golden_ref_checks.py

Contents: the reference's histogram median / IQR, exact median and pnorm on the inputs of
tests/test_oracle_vs_ref.py, and for each of its 2 Mb whole-path cases (key prefix = the test id)
what tools/make_golden.py stores per case: sha256 of the per-base arrays after GC adjust / cap /
compaction, the N regions, the bin arrays, the scan scalars and status arrays, segments and calls.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import oracle
    from conftest import make_case
    from golden_util import sha
    from make_golden import calls_array
    from rsicnv_amd import api
    import test_oracle_vs_ref as T
    lib = api.load_library()
    R = oracle.Ref()
    out = {}

    cases = T.quantile_inputs()
    out["quantile_inputs_sha"] = T.inputs_sha([a for c in cases for a in c])
    out["median"] = np.array([R.median(x) for c in cases for x in c], dtype=np.float64)
    out["iqr"] = np.array([R.iqr(x) for xi, xf, _ in cases for x in (xi, xf)], dtype=np.float64)
    out["median_const"] = np.float64(R.median(np.full(17, 5, dtype=np.int32)))
    out["median_grid"] = np.float64(R.median((30.0 + 0.001 * np.arange(9)).astype(np.float32)))
    xs, pn = T.exact_median_inputs()
    out["exact_inputs_sha"] = T.inputs_sha(xs + [pn])
    out["exact_median"] = np.array([R.exact_median(x) for x in xs], dtype=np.float64)
    out["pnorm"] = np.array([R.pnorm(float(v)) for v in pn], dtype=np.float64)

    for case, flags in zip(T.WHOLE_PATH_IDS, T.WHOLE_PATH_FLAGS):
        _, fasta, depth = make_case(lib, T.whole_path_plan(flags))
        p = oracle.make_params(**flags)
        R.load(p, depth, fasta)
        g = dict(flags=json.dumps(flags), fasta_sha=sha(fasta), depth_sha=sha(depth), noncode=R.noncode())
        R.stage_gc()
        g["rd_gc_sha"] = sha(R.rd())
        R.stage_cap()
        g["rd_cap_sha"] = sha(R.rd())
        R.stage_concat()
        g["rd_concat_sha"] = sha(R.rd())
        g["chrom"] = np.array(R.chrom_scalars())
        g["binmed"], g["binmedint"], g["binnb"] = R.stage_bins()
        trans = flags.get("trans", 0)
        for use_med in ([True] if trans == 1 else [False] if trans == 0 else [True, False]):
            sc, st, segs = R.scan(use_med)
            assert sc.stepwise_matches_reference == 1, "stage driver diverged from the reference's own scan driver"
            pre = "med" if use_med else "nb"
            g[f"{pre}_scan"] = np.array([sc.tmedian1, sc.tsigma1, sc.tlamda1, sc.tmedian2, sc.tsigma2, sc.tlamda2,
                                         sc.target_tlamda, sc.Lmax, sc.cal_max])
            g[f"{pre}_status1"], g[f"{pre}_status1f"], g[f"{pre}_status2"] = st
            g[f"{pre}_segs"] = calls_array(segs)
        raw, fin, _ = R.detect()
        g["calls_raw"], g["calls"] = calls_array(raw), calls_array(fin)
        out.update({f"{case}/{k}": v for k, v in g.items()})
        print(f"{case}: calls raw/final {len(raw)}/{len(fin)}")

    path = os.path.join(ROOT, "tests", "golden", "oracle_vs_ref.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path) / 1024:.0f} KB")


if __name__ == "__main__":
    main()
