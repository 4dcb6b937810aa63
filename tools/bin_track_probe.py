#!/usr/bin/env python3
"""Times the bin-track writer (rsi_hot_write_bin_track: one value per bin as bedGraph, pieces found and formatted on the GPU)
after a run of synth.config_plan(3) -- 250 Mb, resident in HBM, default flags -- against the host loop it replaces: the bin
medians and regions fetched, one fprintf per line (tools/bin_track_probe_fprintf.c).  Medians of --repeat calls after a
warm-up call.  Prints one JSON line.  --format bgzf: the device writer deflates its text on the GPU; its entries
then also hold the file's bytes, members, stored members and the two kernels' time.

--index (with --format bgzf): the tabix index built from the device -- the depth track of the same run
(rsi_hot_write_track) and the bin track, each written --repeat times without and with an index set, alternating; the JSON's
"index" holds the medians of t_total_ms and t_kernel_ms of both, and what the index holds.

  python tools/bin_track_probe.py [--repeat 7] [--scale 1.0] [--dir DIR] [--value ratio|median] [--format text|bgzf] [--index]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def index_runs(api, hot, a, tmp):
    """The depth track and the bin track of the run the context holds, as BGZF, without and with an index set: alternating calls,
    medians of the writer's own figures."""
    med = lambda xs: round(statistics.median(xs), 3)
    res = {}
    writers = {"track": lambda path: hot.write_track(0, "chrProbe", path, format="bgzf"),
               "bintrack": lambda path: hot.write_bin_track(a.value, "chrProbe", path, format="bgzf")}
    for what, write in writers.items():
        path = os.path.join(tmp, f"index_{what}.bedgraph.gz")
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
                st = write(path)
                hot.set_track_index(None)
                if k:
                    runs[mode].append(st)
        res[what] = {mode: {"t_total_ms": med([s["t_total_ms"] for s in rs]), "t_kernel_ms": med([s["t_kernel_ms"] for s in rs]),
                            "all_t_total_ms": [round(s["t_total_ms"], 3) for s in rs]} for mode, rs in runs.items()}
        res[what].update(lines=runs["plain"][0]["lines"], slices=runs["plain"][0]["slices"], **{"index_" + k: v for k, v in ix.counts().items()})
        t0 = time.perf_counter()
        api.bgzf_write_eof(path)
        ix.write_tbi(path + ".tbi")
        res[what]["write_tbi_s"] = round(time.perf_counter() - t0, 4)
        res[what]["tbi_bytes"] = os.path.getsize(path + ".tbi")
        ix.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--scale", type=float, default=1.0, help="shrinks the chromosome (a quick look)")
    ap.add_argument("--value", default="ratio", choices=["ratio", "median"])
    ap.add_argument("--dir", default=None, help="where the files go (default: a temporary directory)")
    ap.add_argument("--format", default="text", choices=["text", "bgzf"], help="bgzf: the device writer's calls deflate on the GPU (DESIGN.md 6h)")
    ap.add_argument("--index", action="store_true", help="with --format bgzf: time the tracks without and with the tabix index (DESIGN.md 6i)")
    a = ap.parse_args()
    if a.index and a.format != "bgzf":
        ap.error("--index needs --format bgzf: a plain-text track has no index")
    import torch
    from rsicnv_amd import api, synth

    lib = api.load_library()
    torch.cuda.set_device(0)
    plan = synth.config_plan(3, chrom=0, scale=a.scale)
    n = plan["n"]
    d_fa = torch.empty(n + 64, dtype=torch.uint8, device="cuda")
    d_rd = torch.empty(n + 16, dtype=torch.int32, device="cuda")
    synth.generate_device(lib, plan, d_fa.data_ptr(), d_rd.data_ptr())
    torch.cuda.synchronize()
    params = api.make_params(**synth.config_flags(3))
    hot = api.RsiHot(0)
    t0 = time.perf_counter()
    res = hot.run_device(params, d_rd.data_ptr(), d_fa.data_ptr(), n)
    run_s = time.perf_counter() - t0
    m, med2 = params.m, int(2 * res.stats["RDmedian"])
    out = {"n": n, "m": m, "value": a.value, "bins": res.stats["nbins"], "regions": res.stats["n_noncode"], "RDmedian": res.stats["RDmedian"],
           "run_s": round(run_s, 4)}
    med = lambda xs: round(statistics.median(xs), 6)
    with tempfile.TemporaryDirectory(dir=a.dir) as tmp:
        for target, path in (("dev_null", "/dev/null"), ("file", os.path.join(tmp, "probe.bedgraph"))):
            runs = []
            for _ in range(a.repeat + 1):   # the first call allocates the workspace and the pinned buffers: warm-up
                if target == "file" and os.path.exists(path):
                    os.unlink(path)         # (replacing a file costs its truncation: not the writer's)
                t0 = time.perf_counter()
                st = hot.write_bin_track(a.value, "chrProbe", path, format=a.format)
                st["wall_s"] = time.perf_counter() - t0
                st["deflate"] = hot.deflate_stats()
                runs.append(st)
            warm = runs[1:]
            out[target] = {"lines": warm[0]["lines"], "bytes": warm[0]["bytes"], "slices": warm[0]["slices"],
                           "first_call_s": round(runs[0]["wall_s"], 6), "wall_s": med([s["wall_s"] for s in warm]),
                           "kernel_s": med([s["t_kernel_ms"] * 1e-3 for s in warm]), "write_s": med([s["t_write_ms"] * 1e-3 for s in warm]),
                           "inside_call_s": med([s["t_total_ms"] * 1e-3 for s in warm])}
            if a.format == "bgzf":
                ds = warm[0]["deflate"]
                out[target].update(file_bytes=ds["file_bytes"], members=ds["members"], stored_members=ds["stored_members"],
                                   deflate_kernel_s=med([s["deflate"]["t_kernel_ms"] * 1e-3 for s in warm]))
        if a.index:
            out["index"] = index_runs(api, hot, a, tmp)
        # the host loop: fetch the arrays (timed: the loop needs them on the host), then one fprintf per line
        t_fetch = []
        for _ in range(a.repeat):
            t0 = time.perf_counter()
            binmed = hot.fetch("binmedint")
            t_fetch.append(time.perf_counter() - t0)
        exe = os.path.join(tmp, "fprintf_loop")
        subprocess.run(["cc", "-O2", "-o", exe, os.path.join(ROOT, "tools", "bin_track_probe_fprintf.c")], check=True)
        f_med, f_pairs, dump = os.path.join(tmp, "binmed.i32"), os.path.join(tmp, "pairs.i32"), os.path.join(tmp, "loop.bedgraph")
        binmed.tofile(f_med)
        np.asarray(res.noncode, dtype=np.int32).tofile(f_pairs)
        loops = {}
        for target, path in (("dev_null", "/dev/null"), ("file", dump)):
            secs = []
            for _ in range(a.repeat):
                if target == "file" and os.path.exists(path):
                    os.unlink(path)
                s, lines, nbytes = subprocess.run([exe, f_med, f_pairs, str(m), str(n), str(max(med2, 1)), path], check=True, capture_output=True,
                                                  text=True).stdout.split()
                secs.append(float(s))
            loops[target] = {"lines": int(lines), "wall_s": med(secs)}
            if target == "file":
                loops[target]["bytes"] = int(nbytes)
        if a.value == "ratio":
            hot.write_bin_track("ratio", "chrProbe", os.path.join(tmp, "probe.bedgraph"))
            loops["same_text"] = open(os.path.join(tmp, "probe.bedgraph"), "rb").read() == open(dump, "rb").read()
        out["fprintf_loop"] = loops
        out["fetch_binmed_s"] = med(t_fetch)
        out["speedup_file"] = round((loops["file"]["wall_s"] + out["fetch_binmed_s"]) / out["file"]["wall_s"], 2)
    hot.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
