"""The BGZF inflate kernel alone (rsi_hot_inflate_bgzf): HIP-event time of the launches over >= 1 GB of depth text written
as BGZF (level 6, 65280-byte members, bgzip's layout) -> GB/s of text out, ISIZE and CRC32 checks included.

  python tools/inflate_bench.py [--gb 1.0] [--out profiles/inflate_bgzf.json]

64 MiB of "RNAME pos depth" text is compressed once and its members repeated up to the size asked for."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def depth_block(nbytes, seed=5):
    rng = np.random.default_rng(seed)
    lines, total, pos = [], 0, 1
    while total < nbytes:
        d = rng.poisson(30, 100_000)
        chunk = "".join(f"chr7\t{pos + i}\t{int(x)}\n" for i, x in enumerate(d))
        pos += d.size
        lines.append(chunk)
        total += len(chunk)
    return "".join(lines).encode()[:nbytes]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gb", type=float, default=1.0)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import bgzf_util as bz
    from rsicnv_amd import api
    text = depth_block(64 << 20)
    text = text[:text.rfind(b"\n") + 1]
    t0 = time.time()
    unit = bz.bgzf(text, eof=False)
    t_zlib = time.time() - t0
    reps = max(1, int(np.ceil(a.gb * 1e9 / len(text))))
    data = unit * reps + bz.EOF_BLOCK
    hot = api.RsiHot(0)
    hot.inflate_bgzf(bz.bgzf(text[:1 << 20]))   # warm-up (code load, allocations)
    runs = []
    for _ in range(3):
        out = hot.inflate_bgzf(data)
        st = hot.inflate_stats()
        runs.append(st["t_inflate_kernel_ms"])
    assert out == text * reps, "inflated text differs"
    best = min(runs)
    rec = {"what": "rsi_hot_inflate_bgzf: HIP-event time of the inflate launches (256 MiB of text per launch), ISIZE + CRC32 checked on the device",
           "text_bytes": len(text) * reps, "compressed_bytes": len(data), "ratio": round(len(text) * reps / len(data), 3),
           "members": st["blocks"], "kernel_ms_runs": [round(x, 3) for x in runs],
           "text_GBps": round(len(text) * reps / best / 1e6, 2), "compressed_GBps": round(len(data) / best / 1e6, 2),
           "host_zlib_compress_s_per_64MiB_one_thread": round(t_zlib, 2), "target_text_GBps": 10.0}
    print(json.dumps(rec))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
    hot.close()


if __name__ == "__main__":
    main()
