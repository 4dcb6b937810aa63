#!/usr/bin/env python3
"""Times the depth-track writer (rsi_hot_write_track_device: runs found, measured and formatted on the GPU, bedGraph out)
against the loop plain -s saves a depth with (one fprintf per base, tools/track_probe_fprintf.c) on the same array: one
synthetic chromosome, 60 Mb at 30x by default.  Prints one JSON line.

  python tools/track_probe.py [--n 60000000] [--mean 30] [--repeat 3] [--dir DIR] [--smooth W] [--format text|bgzf]

--smooth W: the depth changes every W bases on average instead of at every base (real coverage moves in steps: reads
start and end at a few percent of the positions), which is what makes a bedGraph smaller than per-base text.

--format bgzf: the track deflated on the GPU.  The JSON then also holds the file's bytes, members, stored members
and the two kernels' time ("bgzf"), the plain-text call on the same array and disk beside it ("track"), and what zlib makes of
the same 65280-byte members at level 1 and 6 -- of the first --zlib-members members, read back from the file.

--index (with --format bgzf): the same BGZF call without and with a tabix index set, alternating, --repeat times
each after a warm-up pair; "index" holds the medians of t_total_ms and t_kernel_ms and what the index holds."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def bgzf_runs(api, hot, d_depth, a, path, text_best):
    """The BGZF call, best of a.repeat after a warm-up (each into a new file, as the text calls' best is), and zlib on its members."""
    runs = []
    for _ in range(a.repeat + 1):
        if os.path.exists(path):
            os.unlink(path)
        t0 = time.perf_counter()
        st = hot.write_track_device(d_depth.data_ptr(), a.n, "chrProbe", path, format="bgzf")
        st["wall_s"] = time.perf_counter() - t0
        ds = hot.deflate_stats()
        st.update(members=ds["members"], stored_members=ds["stored_members"], text_bytes=ds["text_bytes"], file_bytes=ds["file_bytes"],
                  deflate_ms=ds["t_kernel_ms"])
        runs.append(st)
    api.bgzf_write_eof(path)
    best = min(runs[1:], key=lambda s: s["t_total_ms"])
    slices, text = max(best["slices"], 1), max(best["text_bytes"], 1)
    r = {"text_bytes": best["text_bytes"], "file_bytes": best["file_bytes"], "members": best["members"], "stored_members": best["stored_members"],
         "text_over_file": round(best["text_bytes"] / max(best["file_bytes"], 1), 3), "slices": best["slices"],
         "first_call_s": round(runs[0]["wall_s"], 4), "wall_s": round(best["wall_s"], 4), "inside_call_s": round(best["t_total_ms"] * 1e-3, 4),
         "text_inside_call_s": round(text_best["t_total_ms"] * 1e-3, 4),
         "call_over_text_call": round(best["t_total_ms"] / max(text_best["t_total_ms"], 1e-9), 2),
         "format_kernel_s": round(best["t_kernel_ms"] * 1e-3, 4), "deflate_kernel_s": round(best["deflate_ms"] * 1e-3, 4),
         "deflate_ms_per_slice": round(best["deflate_ms"] / slices, 3), "deflate_ns_per_text_byte": round(best["deflate_ms"] * 1e6 / text, 3),
         "deflate_text_GB_per_s": round(text / 1e9 / max(best["deflate_ms"] * 1e-3, 1e-9), 2),
         "write_s": round(best["t_write_ms"] * 1e-3, 4), "all_inside_call_s": [round(s["t_total_ms"] * 1e-3, 4) for s in runs]}
    # zlib on the same members (the file's first ones): what level 1 and bgzip's level 6 make of this text
    with open(path, "rb") as f:
        data = f.read(a.zlib_members * 65536)
    p, ours, texts = 0, 0, []
    while p + 18 <= len(data) and len(texts) < a.zlib_members:
        bsize = int.from_bytes(data[p + 16:p + 18], "little") + 1
        if p + bsize > len(data) or bsize == 28:
            break
        texts.append(zlib.decompress(data[p + 18:p + bsize - 8], -15))
        ours += bsize
        p += bsize
    sample = {"members": len(texts), "text_bytes": sum(len(t) for t in texts), "file_bytes": ours}
    for level in (1, 6):
        total = 0
        for t in texts:
            c = zlib.compressobj(level, zlib.DEFLATED, -15)
            total += len(c.compress(t) + c.flush()) + 26
        sample[f"zlib{level}_bytes"] = total
        sample[f"file_over_zlib{level}"] = round(ours / max(total, 1), 3)
    r["zlib_sample"] = sample
    return r


def index_runs(api, hot, d_depth, a, path):
    import statistics
    med = lambda xs: round(statistics.median(xs), 3)
    runs = {"plain": [], "indexed": []}
    ix = api.TrackIndex()
    for k in range(a.repeat + 1):       # the first pair warms up
        for mode in ("plain", "indexed"):
            if os.path.exists(path):
                os.unlink(path)
            if mode == "indexed":
                ix.close()
                ix = api.TrackIndex()
            hot.set_track_index(ix if mode == "indexed" else None)
            st = hot.write_track_device(d_depth.data_ptr(), a.n, "chrProbe", path, format="bgzf")
            hot.set_track_index(None)
            if k:
                runs[mode].append(st)
    res = {mode: {"t_total_ms": med([s["t_total_ms"] for s in rs]), "t_kernel_ms": med([s["t_kernel_ms"] for s in rs]),
                  "all_t_total_ms": [round(s["t_total_ms"], 3) for s in rs]} for mode, rs in runs.items()}
    res.update({"index_" + k: v for k, v in ix.counts().items()})
    ix.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=60_000_000)
    ap.add_argument("--mean", type=float, default=30.0)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--smooth", type=int, default=0)
    ap.add_argument("--dir", default=None, help="where the files go (default: a temporary directory)")
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--format", default="text", choices=["text", "bgzf"])
    ap.add_argument("--zlib-members", type=int, default=256, help="members of the BGZF file that zlib compresses for comparison")
    ap.add_argument("--index", action="store_true", help="with --format bgzf: time the call without and with the tabix index (DESIGN.md 6i)")
    a = ap.parse_args()
    if a.index and a.format != "bgzf":
        ap.error("--index needs --format bgzf: a plain-text track has no index")
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
        if a.format == "bgzf":
            out["bgzf"] = bgzf_runs(api, hot, d_depth, a, os.path.join(tmp, "probe.bedgraph.gz"), best)
        if a.index:
            out["index"] = index_runs(api, hot, d_depth, a, os.path.join(tmp, "probe_index.bedgraph.gz"))
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
