"""`rsicnv geno` on the device beside what it replaces.

  python tools/geno_probe.py [--scale 1.0] [--lines 1000,10000] [--reps 7] [--host-reps 2] [--out profiles/geno_device.json]

A run of synth.config_plan(3) -- 250 Mb at 30x, resident in HBM, default flags -- then lists of regions of 1 kb to 1 Mb (lengths
log-uniform, starts uniform, seeded).  Per list: rsi_hot_geno_calls (wall around the call and the library's own figure, launches,
jobs, tiles; warm-up calls first, every timing kept), and the road it replaces, in the same process: the fetch of rd_concat to the
host, then the same statistic there by hostmath.h's grid_quantiles<int> (tools/geno_host_stat.cpp, compiled here with -O3).  The
two roads' quantiles are compared line by line."""
import argparse, ctypes as C, json, os, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from rsicnv_amd import api, synth
import geno_cases as gc


def spread(ms):
    ms = sorted(ms)
    return {"min": ms[0], "median": ms[len(ms) // 2], "max": ms[-1], "all": ms}


def host_library(tmp):
    so = os.path.join(tmp, "geno_host_stat.so")
    subprocess.run(["g++", "-O3", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", os.path.join(ROOT, "tools", "geno_host_stat.cpp"), "-o", so], check=True)
    L = C.CDLL(so)
    L.geno_host_stat.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    L.geno_host_stat.restype = None
    return L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--lines", default="1000,10000")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "geno_device.json"))
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
    hot = api.RsiHot(0)
    params = api.make_params()
    res = hot.run_device(params, d_rd.data_ptr(), d_fa.data_ptr(), n)
    nc = int(res.stats["n_compact"])
    pairs = [(int(res.noncode[2 * k]), int(res.noncode[2 * k + 1])) for k in range(len(res.noncode) // 2)]
    result = {"bases": n, "n_compact": nc, "regions_removed": len(pairs), "chrom_median": res.stats["RDmedian"], "m": params.m, "reps": a.reps,
              "warmup": a.warmup, "host_reps": a.host_reps, "cpus": os.cpu_count(), "device": torch.cuda.get_device_name(0), "lists": []}
    with tempfile.TemporaryDirectory() as tmp:
        H = host_library(tmp)
        for nl in [int(v) for v in a.lines.split(",")]:
            rng = np.random.default_rng(0x6E00 + nl)
            hi_len = max(2000.0, 1e6 * a.scale)
            length = np.exp(rng.uniform(np.log(1000.0), np.log(hi_len), nl)).astype(np.int64)
            start = (1 + rng.uniform(0, 1, nl) * (n - length - 1)).astype(np.int64)
            end = start + length - 1
            for _ in range(a.warmup):
                hot.geno_calls(params.m, start, end)
            wall, own = [], []
            for _ in range(a.reps):
                t = time.perf_counter()
                rec = hot.geno_calls(params.m, start, end)
                wall.append((time.perf_counter() - t) * 1e3)
                own.append(hot.geno_stats()["ms"])
            st = hot.geno_stats()
            jobs = np.array([gc.line_job(*gc.map_line(int(s), int(e), n, pairs), params.m, nc) for s, e in zip(start, end)], dtype=np.int64)
            fetch, stat = [], []
            out = np.zeros((nl, 6), dtype=np.float64)
            for _ in range(a.host_reps):
                t = time.perf_counter()
                rd = hot.fetch("rd_concat")
                fetch.append((time.perf_counter() - t) * 1e3)
                t = time.perf_counter()
                H.geno_host_stat(rd.ctypes.data, nl, jobs.ctypes.data, out.ctypes.data)
                stat.append((time.perf_counter() - t) * 1e3)
            has_body, has_flank = rec["n_body"] > 0, rec["n_flank"] > 0
            same = bool(np.array_equal(rec["body_q"][has_body], out[has_body, :3]) and np.array_equal(rec["flank_q"][has_flank], out[has_flank, 3:]) and
                        np.array_equal(rec["n_body"], jobs[:, 1] - jobs[:, 0]))
            entry = {"lines": nl, "bases_in_bodies": int(rec["n_body"].sum()), "bases_in_flanks": int(rec["n_flank"].sum()), "launches": st["launches"],
                     "jobs": st["jobs"], "tiles": st["tiles"], "passes": st["passes"], "workspace_bytes": st["bytes"], "device_wall_ms": spread(wall),
                     "device_own_ms": spread(own), "host_fetch_ms": spread(fetch), "host_stat_ms": spread(stat),
                     "host_total_min_ms": min(fetch) + min(stat), "quantiles_equal": same}
            print(json.dumps(entry), flush=True)
            result["lists"].append(entry)
            assert same, "the device and the host road disagree"
    hot.close()
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
