#!/usr/bin/env python3
"""Generate tests/golden/per_base_edges.npz from the REAL reference (oracle/_ref/libref.so, built by oracle/Makefile.ref): its
answers on the per-base stages for every case of tests/per_base_cases.py.  Data only, never reference source.

  python tools/make_golden_per_base.py

Per case: sha256 of the inputs, of the array after the GC adjustment, after the cap and after the compaction, the N regions, the
bins' integer medians (and their sha256; that alone above 4096 bins), and the scalars
[RDmedian, RDsd, cap median, mean of the positive depths] -- the cap median is the reference's _median of the adjusted array
(what apply_cap takes, loaddata.cpp:233), the mean is the exact quotient gccontent.cpp:109-112 forms.

Each stage of each case runs in the reference inside THIS process: a case on which the compiled reference exits or aborts would
end the script, and has to leave tests/per_base_cases.py (its docstring then says which and why).  None does today.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

MAX_BINS_STORED = 4096


def write_npz(path, arrays):
    """np.savez_compressed with the archive's time stamps fixed: the same data gives the same file, byte for byte."""
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            with z.open(info, "w") as f:
                np.lib.format.write_array(f, np.asanyarray(arrays[k]), allow_pickle=False)


def main():
    import oracle
    import per_base_cases as pc
    from golden_util import sha
    R = oracle.Ref()
    meta, chrom, noncode, medints = {}, [], [], []
    for cid in pc.case_ids():
        case = pc.get_case(cid)
        _, fasta0, depth0, flags, _, _ = case
        fasta, depth = pc.checker_inputs(case)
        p = oracle.make_params(**flags)
        R.load(p, depth, fasta)
        g = dict(flags=flags, fasta_sha=sha(fasta0), depth_sha=sha(depth0))
        noncode.append(R.noncode().astype(np.int32))
        R.stage_gc()
        rd_gc = R.rd()
        g["rd_gc_sha"] = sha(rd_gc)
        cap_median = R.median(rd_gc) if flags["cap"] > 1 else 0.0
        R.stage_cap()
        g["rd_cap_sha"] = sha(R.rd())
        R.stage_concat()
        rdc = R.rd()
        g["rd_concat_sha"] = sha(rdc)
        g["n_compact"] = int(rdc.size)
        rdmed, rdsd = R.chrom_scalars()
        pos = depth[depth > 0].astype(np.int64)
        rdmean = float(pos.sum()) / float(pos.size) if pos.size and flags["gcadjust"] else 0.0
        chrom.append([rdmed, rdsd, cap_median, rdmean])
        _, medint, _ = R.stage_bins()
        g["nbins"] = int(medint.size)
        g["binmedint_sha"] = sha(medint)
        medints.append(medint if medint.size <= MAX_BINS_STORED else medint[:0])
        meta[cid] = g
        print(f"{cid}: n {depth.size} n' {rdc.size} bins {medint.size} regions {noncode[-1].size // 2} cap median {cap_median}", flush=True)
    # one entry per kind, not per case: an archive of a few thousand tiny members is mostly member headers
    out = dict(meta=np.array(json.dumps(meta, sort_keys=True)), ids=np.array(json.dumps(list(meta))),
               chrom=np.array(chrom, dtype=np.float64),
               noncode=np.concatenate(noncode), noncode_off=np.cumsum([0] + [a.size for a in noncode]).astype(np.int64),
               binmedint=np.concatenate(medints), binmedint_off=np.cumsum([0] + [a.size for a in medints]).astype(np.int64))
    path = os.path.join(ROOT, "tests", "golden", "per_base_edges.npz")
    write_npz(path, out)
    print(f"{path}: {os.path.getsize(path) / 1024:.0f} KB")


if __name__ == "__main__":
    main()
