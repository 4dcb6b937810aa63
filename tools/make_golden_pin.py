#!/usr/bin/env python
"""Generate tests/golden/pin_edges.npz from the REAL reference (oracle/_ref/rsicnv_ref and oracle/_ref/libref.so, built by
oracle/Makefile.ref): `rsicnv_ref pin` and `rsicnv_ref stat` on the BAM of every case of tests/pin_cases.py, indexed with the
reference's own bam_index_build.  Per case: START and END of every output row of pin, RP and Q0 (as printed) of every row of stat,
and the sample's six log lines.  Recorded results only.

Usage: python tools/make_golden_pin.py   (needs oracle/_ref: make -f oracle/Makefile all)"""
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
REF_BIN = os.path.join(ROOT, "oracle", "_ref", "rsicnv_ref")
LIBREF = os.path.join(ROOT, "oracle", "_ref", "libref.so")
SAMPLE_KEYS = ("sample chr", "read length", "rd mean", "rd sd", "drd mean", "drd sd")


def index(bam):
    L = ctypes.CDLL(LIBREF)
    L.bam_index_build.argtypes = [ctypes.c_char_p]
    if L.bam_index_build(os.fsencode(bam)) != 0:
        raise RuntimeError("bam_index_build failed")


def run_ref(function, bam, cnv, tmp, m):
    out = os.path.join(tmp, function + ".out")
    r = subprocess.run([REF_BIN, function, "-b", bam, "-v", cnv, "-o", out, "-m", str(m)], cwd=tmp, capture_output=True, text=True, timeout=600)
    if r.returncode != 0 or not os.path.exists(out):
        raise RuntimeError(f"rsicnv_ref {function} failed ({r.returncode}): {r.stderr[-800:]}")
    rows = [ln.split("\t") for ln in open(out).read().splitlines() if ln and not ln.startswith("#")]
    return rows, r.stderr


def sample_lines(stderr):
    """the first sample's six values as printed"""
    vals = {}
    for ln in stderr.splitlines():
        k, _, v = ln.partition(":")
        if k.strip() in SAMPLE_KEYS and k.strip() not in vals:
            vals[k.strip()] = v.strip()
    return [vals.get(k, "") for k in SAMPLE_KEYS]


def golden_of(tmp, tag, bam, cnv_text, m):
    cnv = os.path.join(tmp, tag + ".cnv")
    open(cnv, "w").write(cnv_text + "\n")
    index(bam)
    pin_rows, pin_err = run_ref("pin", bam, cnv, tmp, m)
    stat_rows, _ = run_ref("stat", bam, cnv, tmp, m)
    return {tag + ".pin": np.array([[int(r[1]), int(r[2])] for r in pin_rows], dtype=np.int64).reshape(-1, 2),
            tag + ".sample": np.array(sample_lines(pin_err)),
            tag + ".stat": np.array([r[-1] for r in stat_rows])}


def main():
    import bam_util as bu
    import pin_cases as pn
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, case in pn.cases().items():
            # the reference segfaults on a chromosome the header does not name: those lines are this build's own business
            known = "\n".join(ln for ln in case.cnv.split("\n") if not ln.startswith(pn.NO_CHROM))
            bam = os.path.join(tmp, name + ".bam")
            pn.write_case_bam(bam, case.reads)
            out.update(golden_of(tmp, name, bam, known, case.m))
            print(name, out[name + ".pin"].tolist(), out[name + ".stat"].tolist(), out[name + ".sample"].tolist())
        refs, reads, cnv = pn.stat_two_chromosomes()
        bam = os.path.join(tmp, "two.bam")
        bu.write_bam(bam, refs, pn.encode(reads, 0) + pn.encode(reads, 1), block=20000)
        out.update(golden_of(tmp, "two_chromosomes", bam, cnv, 101))
        print("two_chromosomes", out["two_chromosomes.stat"].tolist())
    path = os.path.join(ROOT, "tests", "golden", "pin_edges.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
