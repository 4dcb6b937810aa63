#!/usr/bin/env python3
"""Times the depth-track writer (rsi_hot_write_track_device: runs found, measured and formatted on the GPU, bedGraph out)
against the loop plain -s saves a depth with (one fprintf per base, tools/track_probe_fprintf.c) on the same array: one
synthetic chromosome, 60 Mb at 30x by default.  Prints one JSON line.

  python tools/track_probe.py [--n 60000000] [--mean 30] [--repeat 3] [--dir DIR] [--smooth W]

--smooth W: the depth changes every W bases on average instead of at every base (real coverage moves in steps: reads
start and end at a few percent of the positions), which is what makes a bedGraph smaller than per-base text."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=60_000_000)
    ap.add_argument("--mean", type=float, default=30.0)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--smooth", type=int, default=0)
    ap.add_argument("--dir", default=None, help="where the files go (default: a temporary directory)")
    ap.add_argument("--no-baseline", action="store_true")
    a = ap.parse_args()
    import torch
    from rsicnv_amd import api

    rng = np.random.default_rng(0x7AC)
    if a.smooth > 1:
        k = a.n // a.smooth + 2
        depth = np.repeat(rng.poisson(a.mean, k), rng.geometric(1.0 / a.smooth, k))[:a.n].astype(np.int32)
        depth = np.concatenate([depth, np.full(a.n - depth.size, int(a.mean), dtype=np.int32)])
    else:
        depth = rng.poisson(a.mean, a.n).astype(np.int32)
    d_depth = torch.from_numpy(depth).to("cuda:0")
    torch.cuda.synchronize()
    hot = api.RsiHot(0)
    out = {"n": a.n, "mean": a.mean, "smooth": a.smooth}
    with tempfile.TemporaryDirectory(dir=a.dir) as tmp:
        track = os.path.join(tmp, "probe.bedgraph")
        runs = []
        for _ in range(a.repeat + 1):   # the first call allocates the workspace and the pinned buffers: warm-up
            t0 = time.perf_counter()
            st = hot.write_track_device(d_depth.data_ptr(), a.n, "chrProbe", track)
            st["wall_s"] = time.perf_counter() - t0
            runs.append(st)
        best = min(runs[1:], key=lambda s: s["wall_s"])
        out["track"] = {"lines": best["lines"], "bytes": best["bytes"], "slices": best["slices"], "first_call_s": round(runs[0]["wall_s"], 4),
                        "wall_s": round(best["wall_s"], 4), "MB_per_s": round(best["bytes"] / 1e6 / best["wall_s"], 1),
                        "kernel_s": round(best["t_kernel_ms"] * 1e-3, 4), "write_s": round(best["t_write_ms"] * 1e-3, 4),
                        "copy_and_waits_s": round((best["t_total_ms"] - best["t_kernel_ms"] - best["t_write_ms"]) * 1e-3, 4),
                        "all_wall_s": [round(s["wall_s"], 4) for s in runs]}
        os.unlink(track)
        if not a.no_baseline:
            exe, raw, dump = os.path.join(tmp, "fprintf_loop"), os.path.join(tmp, "depth.i32"), os.path.join(tmp, "probe_rd")
            subprocess.run(["cc", "-O2", "-o", exe, os.path.join(ROOT, "tools", "track_probe_fprintf.c")], check=True)
            depth.tofile(raw)
            secs = []
            for _ in range(max(1, min(a.repeat, 2))):
                s, nbytes = subprocess.run([exe, raw, dump], check=True, capture_output=True, text=True).stdout.split()
                secs.append(float(s))
            out["fprintf_loop"] = {"bytes": int(nbytes), "wall_s": round(min(secs), 4), "MB_per_s": round(int(nbytes) / 1e6 / min(secs), 1),
                                   "all_wall_s": [round(s, 4) for s in secs]}
            out["speedup"] = round(min(secs) / best["wall_s"], 2)
            out["bytes_ratio"] = round(int(nbytes) / max(best["bytes"], 1), 2)
    hot.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
