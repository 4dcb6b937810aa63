#!/usr/bin/env python3
"""The golden depth arrays of the BAM path: what the REAL reference (oracle/_ref/rsicnv_ref -b ... -s) counts.

  small   tests/golden/bam_small.npz: the deterministic synthetic BAM of tests/bam_util.py, for two (minq, min_baseQ)
          settings and two chromosomes.
  edges   tests/golden/bam_edges.npz: every case of tests/bam_edge_cases.py that the reference has a defined answer for,
          for every reference and setting of the case, each array as its change points (bam_edge_cases.pack_depth).

usage: make_golden_bam.py small|edges ...   Each output is written only when it is named, so making one leaves the other
as it is.  Data only: the plan of the synthetic reads + the reference's outputs."""
import os, sys, tempfile
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import bam_util as bu
import oracle
from conftest import make_case
from test_hot_extra import _write_case
from rsicnv_amd import api

libref = os.path.join(os.path.dirname(oracle.REF_BIN), "libref.so")
tmp = tempfile.mkdtemp()


def make_small():
    lib = api.load_library()
    spec = bu.golden_spec()
    out = {}
    bam, refs, recs = bu.build_golden_bam(tmp)
    for chrom, n in refs:
        _, fasta, depth = make_case(lib, dict(n=n, seed=0xBA4 + len(chrom), model=0, n_events=2, gaps=1, max_len=8000, end_n=3000, gap_len=5000))
        d = os.path.join(tmp, chrom); os.makedirs(d, exist_ok=True)
        fa, _ = _write_case(d, fasta, depth, chrom=chrom)
        for q, Q in spec["settings"]:
            rd, _ = bu.reference_depth_dump(oracle.REF_BIN, libref, bam, fa, chrom, d, extra=("-q", str(q), "-Q", str(Q)))
            out[f"{chrom}_q{q}_Q{Q}"] = rd
            print(chrom, q, Q, "mean depth %.2f" % rd.mean())
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "bam_small.npz"), **out)
    print("written", os.path.getsize(os.path.join(ROOT, "tests", "golden", "bam_small.npz")) // 1024, "KB")


def write_fasta(d, chrom, n):
    """A FASTA of the reference's length with its .fai: the reference wants one, the depth dump does not depend on it."""
    fa = os.path.join(d, "ref.fa")
    seq = np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(n).integers(0, 4, n)].tobytes()
    with open(fa, "wb") as f:
        f.write(f">{chrom}\n".encode())
        for i in range(0, n, 60):
            f.write(seq[i:i + 60] + b"\n")
    with open(fa + ".fai", "w") as f:
        f.write(f"{chrom}\t{n}\t{len(chrom) + 2}\t60\t61\n")
    return fa


def make_edges():
    import bam_edge_cases as ec
    out = {}
    for name in ec.IN_REFERENCE:
        c = ec.case(name)
        assert c.golden
        bam = c.write(tmp)
        for key, t, chrom, n, q, Q in c.keys():
            d = os.path.join(tmp, name, chrom); os.makedirs(d, exist_ok=True)
            fa = write_fasta(d, chrom, n)
            rd, _ = bu.reference_depth_dump(oracle.REF_BIN, libref, bam, fa, chrom, d, extra=("-q", str(q), "-Q", str(Q)))
            assert rd.size == n, (key, rd.size)
            at, val = ec.pack_depth(rd)
            assert np.array_equal(ec.unpack_depth(at, val, n), rd)
            out[key + ":n"], out[key + ":at"], out[key + ":val"] = np.int64(n), at, val
            print(key, "max depth", int(rd.max()), "change points", at.size, flush=True)
    path = os.path.join(ROOT, "tests", "golden", "bam_edges.npz")
    np.savez_compressed(path, **out)
    print("written", os.path.getsize(path) // 1024, "KB")


if __name__ == "__main__":
    what = sys.argv[1:]
    if not what or set(what) - {"small", "edges"}:
        sys.exit(__doc__)
    if "small" in what: make_small()
    if "edges" in what: make_edges()
