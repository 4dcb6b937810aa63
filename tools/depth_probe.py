"""`rsicnv depth` on the device beside what it replaces.

  python tools/depth_probe.py [--scale 1.0] [--window 500] [--regions 10000] [--reps 7] [--out profiles/depth_device.json]

The depth of synth.config_plan(3) -- 250 Mb at 30x -- resident in HBM, no run.  Timed, after warm-up calls, every timing kept: the
summary pass (HIP events around the kernel, and the wall around the call), the window track at W as plain text and as BGZF, a list
of regions of 1 kb to 1 Mb (records, and their track).  Then the road these replace, in the same process: the array fetched to the
host (1 GB), numpy.bincount for the distribution, numpy.add.reduceat for the windows, a prefix sum for the regions.  The two roads'
results are compared: every number, and every line of the window and region files."""
import argparse, json, os, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from rsicnv_amd import api, synth
import depth_cases as dc


def spread(ms):
    ms = sorted(ms)
    return {"min": ms[0], "median": ms[len(ms) // 2], "max": ms[-1], "all": ms}


def timed(fn, warmup, reps, own=None):
    for _ in range(warmup):
        fn()
    wall, mine = [], []
    for _ in range(reps):
        t = time.perf_counter()
        out = fn()
        wall.append((time.perf_counter() - t) * 1e3)
        if own:
            mine.append(own())
    return out, spread(wall), (spread(mine) if own else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--window", type=int, default=500)
    ap.add_argument("--regions", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_device.json"))
    a = ap.parse_args()
    import torch
    lib = api.load_library()
    torch.cuda.set_device(0)
    plan = synth.config_plan(3, chrom=0, scale=a.scale)
    n = plan["n"]
    d_fa = torch.empty(n + 64, dtype=torch.uint8, device="cuda")
    d_rd = torch.empty(n + 16, dtype=torch.int32, device="cuda")
    synth.generate_device(lib, plan, d_fa.data_ptr(), d_rd.data_ptr())
    torch.cuda.synchronize()
    del d_fa
    hot = api.RsiHot(0)
    ptr = d_rd.data_ptr()
    result = {"bases": n, "reps": a.reps, "warmup": a.warmup, "window": a.window, "cpus": os.cpu_count(), "device": torch.cuda.get_device_name(0)}
    rng = np.random.default_rng(0xDE97)
    length = np.exp(rng.uniform(np.log(1000.0), np.log(max(2000.0, 1e6 * a.scale)), a.regions)).astype(np.int64)
    start = (rng.uniform(0, 1, a.regions) * (n - length - 1)).astype(np.int64)
    end = start + length
    with tempfile.TemporaryDirectory() as tmp:
        (rec, bins), wall, kern = timed(lambda: hot.depth_summary(ptr, n), a.warmup, a.reps, lambda: hot.depth_stats()["kernel_ms"])
        st = hot.depth_stats()
        result["summary"] = {"wall_ms": wall, "kernel_ms": kern, "workgroups": st["workgroups"], "launches": st["launches"], "workspace_bytes": st["bytes"],
                             "TBps_at_kernel_min": 4.0 * n / (kern["min"] * 1e-3) / 1e12, "TBps_at_kernel_median": 4.0 * n / (kern["median"] * 1e-3) / 1e12}
        print(json.dumps(result["summary"]), flush=True)
        files = {}
        for fmt in ("text", "bgzf"):
            path = os.path.join(tmp, "win." + fmt)
            tk, wall, _ = timed(lambda: hot.write_window_track(ptr, n, "chr1", a.window, path, format=fmt), a.warmup, a.reps)
            files[fmt] = path
            result["windows_" + fmt] = {"wall_ms": wall, "lines": tk["lines"], "text_bytes": tk["bytes"], "slices": tk["slices"], "file_bytes": os.path.getsize(path),
                                        "kernel_ms_last": tk["t_kernel_ms"], "write_ms_last": tk["t_write_ms"], "launches": hot.depth_stats()["launches"]}
            print(json.dumps(result["windows_" + fmt]), flush=True)
        regs, wall, own = timed(lambda: hot.depth_regions(ptr, n, start, end), a.warmup, a.reps, lambda: hot.depth_stats()["ms"])
        result["regions"] = {"count": a.regions, "bases": int(regs["n"].sum()), "wall_ms": wall, "own_ms": own, "tiles": hot.depth_stats()["workgroups"],
                             "launches": hot.depth_stats()["launches"]}
        rpath = os.path.join(tmp, "regions.txt")
        tk, wall, _ = timed(lambda: hot.write_region_track(ptr, n, "chr1", start, end, rpath, format="text"), a.warmup, a.reps)
        result["regions"]["track_wall_ms"] = wall
        print(json.dumps(result["regions"]), flush=True)

        # the road these replace
        t = time.perf_counter(); rd = d_rd[:n].cpu().numpy(); fetch = (time.perf_counter() - t) * 1e3
        t = time.perf_counter()
        hbins = np.bincount(np.minimum(rd, dc.BINS - 1), minlength=dc.BINS)
        hsum, hmin, hmax = int(rd.sum(dtype=np.int64)), int(rd.min()), int(rd.max())
        t_summary = (time.perf_counter() - t) * 1e3
        t = time.perf_counter()
        wsum = np.add.reduceat(rd, np.arange(0, n, a.window), dtype=np.int64)
        t_windows = (time.perf_counter() - t) * 1e3
        t = time.perf_counter()
        cs = np.concatenate(([0], np.cumsum(rd, dtype=np.int64)))
        rsum = cs[end] - cs[start]
        t_regions = (time.perf_counter() - t) * 1e3
        result["host"] = {"fetch_ms": fetch, "bincount_sum_min_max_ms": t_summary, "reduceat_ms": t_windows, "prefix_sum_regions_ms": t_regions}
        same = {"summary": (int(rec["sum"]), int(rec["min"]), int(rec["max"]), int(rec["n"])) == (hsum, hmin, hmax, n) and bool(np.array_equal(bins, hbins)),
                "regions": bool(np.array_equal(regs["sum"], rsum) and np.array_equal(regs["n"], length))}
        want = "".join(f"chr1\t{k * a.window}\t{min(n, (k + 1) * a.window)}\t{dc.fixed2(int(s), min(n, (k + 1) * a.window) - k * a.window)}\n" for k, s in enumerate(wsum))
        same["windows_text"] = open(files["text"]).read() == want
        import gzip
        same["windows_bgzf"] = gzip.open(files["bgzf"], "rt").read() == want
        same["regions_text"] = open(rpath).read() == "".join(f"chr1\t{s}\t{e}\t{dc.fixed2(int(v), e - s)}\n" for s, e, v in zip(start.tolist(), end.tolist(), rsum.tolist()))
        result["equal"] = same
        print(json.dumps({"host": result["host"], "equal": same}), flush=True)
    hot.close()
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
    assert all(same.values()), "the device and the host road disagree"


if __name__ == "__main__":
    main()
