"""Stored reference answers for the depth-text number rule: every case of tests/text_rules.py's corpus read by the reference's
own load_data_from_text (oracle/_ref/libref.so, ref_load_text; GC adjustment and cap off) -> tests/golden/text_rules.npz:
rd_<case> (int32, one value per base) and sha_<case> (the SHA-256 of the case's text).
Usage: python tools/make_golden_text_rules.py   (needs oracle/_ref/libref.so: make -f oracle/Makefile all)"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle  # noqa: E402
import text_rules as tr  # noqa: E402

N = 3001


def write_fasta(path, n, name="chrS"):
    seq = ("ACGT" * (n // 4 + 1))[:n]
    body = "".join(seq[i:i + 60] + "\n" for i in range(0, n, 60))
    with open(path, "w") as f:
        f.write(f">{name}\n{body}")
    with open(path + ".fai", "w") as f:
        f.write(f"{name}\t{n}\t{len(name) + 2}\t60\t61\n")


def reference_answers(ref, tmp):
    fa = os.path.join(tmp, "ref.fa")
    write_fasta(fa, N)
    out = {}
    for case in tr.CASES:
        b = tr.case_bytes(case, N)
        p = os.path.join(tmp, f"{case}.txt")
        with open(p, "wb") as f:
            f.write(b)
        rd = ref.load_text(p, fa, "chrS")
        assert rd.size == N, (case, rd.size)
        out[f"rd_{case}"] = rd
        out[f"sha_{case}"] = np.array(tr.text_hash(b))
    return out


def main():
    ref = oracle.Ref()
    with tempfile.TemporaryDirectory() as tmp:
        out = reference_answers(ref, tmp)
    dst = os.path.join(ROOT, "tests", "golden", "text_rules.npz")
    np.savez_compressed(dst, **out)
    print(f"wrote {dst}: {len(tr.CASES)} cases, {os.path.getsize(dst)} bytes")


if __name__ == "__main__":
    main()
