"""Plot data from the device beside the road it replaces.

  python tools/plot_probe.py [--scale 1.0] [--calls 100,1000] [--reps 7] [--out profiles/plot_device.json]

A run of synth.config_plan(3) -- 250 Mb at 30x, resident in HBM, default flags -- then lists of calls of 1 kb to 1 Mb (lengths
log-uniform, starts uniform, seeded).  Per list: rsi_hot_plot_run (warm-up calls first, then every timing kept: wall around the
call, the expansion's own events, launches, batches, tiles, the bytes that crossed PCIe), and the files written from the filled
batch into a RAM-backed folder.  The road it replaces, in the same process, once, its parts apart: the fetch of rd_concat to the
host, rsi_plot_expand, the array's median by counting (numpy.bincount and a walk, what partition_stat_tp does), and
rsi_plot_write_files for every call, the files going to the same RAM-backed folder.  For the first list the two roads' numbers are
compared call by call (a host fill of the same batch)."""
import argparse, ctypes as C, json, os, shutil, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from rsicnv_amd import api, synth


def spread(ms):
    ms = sorted(ms)
    return {"min": ms[0], "median": ms[len(ms) // 2], "max": ms[-1], "all": ms}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--calls", default="100,1000")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--ram", default="/dev/shm")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plot_device.json"))
    a = ap.parse_args()
    import torch
    lib = api.load_library()
    lib.rsi_plot_expand.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_int64]
    lib.rsi_plot_write_files.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int64, C.c_double, C.c_int, C.c_double, C.c_double,
                                         C.c_char_p, C.c_double, C.c_char_p, C.c_char_p, C.c_char_p]
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
    result = {"bases": n, "n_compact": nc, "regions_removed": len(res.noncode) // 2, "m": params.m, "reps": a.reps, "warmup": a.warmup,
              "cpus": os.cpu_count(), "device": torch.cuda.get_device_name(0), "lists": []}
    folder = tempfile.mkdtemp(dir=a.ram if os.path.isdir(a.ram) else None)
    try:
        for li, nl in enumerate(int(v) for v in a.calls.split(",")):
            rng = np.random.default_rng(0x706C00 + nl)
            hi_len = max(2000.0, 1e6 * a.scale)
            length = np.exp(rng.uniform(np.log(1000.0), np.log(hi_len), nl)).astype(np.int64)
            start = (1 + rng.uniform(0, 1, nl) * (n - length - 2)).astype(np.int64)
            end = start + length - 1
            calls = []
            for s, e in zip(start, end):
                c = api.RsiCall()
                c.start, c.end, c.type, c.length, c.p1 = int(s), int(e), 0, int(e - s + 1), 1e-9
                calls.append(c)

            def planned():
                b = api.PlotBatch(n, params.m, params.minmlen, params.chklen)
                for c in calls:
                    b.add(0, 0, call=c)
                return b
            names = [os.path.join(folder, "rsi_chrS_%d_%d_DEL" % (c.start, c.end)) for c in calls]
            dev = planned()
            for _ in range(a.warmup):
                hot.plot_run(res, dev)
            wall, own, expand = [], [], []
            for _ in range(a.reps):
                t = time.perf_counter()
                hot.plot_run(res, dev)
                wall.append((time.perf_counter() - t) * 1e3)
                st = hot.plot_stats()
                own.append(st["ms"]); expand.append(st["expand_ms"])
            t = time.perf_counter()
            for k, nm in enumerate(names):
                assert dev.write(k, "t", nm + ".dat", nm + ".gp", nm + ".ps")
                os.unlink(nm + ".dat"); os.unlink(nm + ".gp")
            dev_write = (time.perf_counter() - t) * 1e3
            # the road it replaces
            t = time.perf_counter()
            rdc = hot.fetch("rd_concat")
            fetch = (time.perf_counter() - t) * 1e3
            full = np.zeros(n, dtype=np.int32)
            pairs = np.ascontiguousarray(res.noncode, dtype=np.int32)
            t = time.perf_counter()
            assert lib.rsi_plot_expand(rdc.ctypes.data, rdc.size, pairs.ctypes.data, pairs.size // 2, full.ctypes.data, n) == 0
            expand_host = (time.perf_counter() - t) * 1e3
            t = time.perf_counter()
            lo = int(full.min())
            cum = np.cumsum(np.bincount(full - lo))
            med = float(lo + int(np.searchsorted(cum, n // 2, side="left")))
            median_host = (time.perf_counter() - t) * 1e3
            t = time.perf_counter()
            for c, nm in zip(calls, names):
                assert lib.rsi_plot_write_files(C.byref(c), b"t", full.ctypes.data, n, med, params.m, params.minmlen, params.chklen, b"ps", 5.0,
                                                (nm + ".dat").encode(), (nm + ".gp").encode(), (nm + ".ps").encode()) == 0
                os.unlink(nm + ".dat"); os.unlink(nm + ".gp")
            write_host = (time.perf_counter() - t) * 1e3
            same = None
            if li == 0:
                host = planned()
                host.fill_host(full)
                same = dev.compare(host) == 0 and dev.chrom_median() == med
            entry = {"calls": nl, "queries": st["queries"], "launches": st["launches"], "batches": st["batches"], "tiles": st["tiles"],
                     "bytes_up": st["bytes_up"], "bytes_down": st["bytes_down"], "device_bytes_held": st["bytes"],
                     "plot_run_wall_ms": spread(wall), "plot_run_own_ms": spread(own), "expand_kernel_ms": spread(expand), "device_road_write_files_ms": dev_write,
                     "host_fetch_ms": fetch, "host_fetch_bytes": int(rdc.size) * 4, "host_expand_ms": expand_host, "host_median_ms": median_host,
                     "host_write_files_ms": write_host, "numbers_equal": same}
            print(json.dumps(entry), flush=True)
            result["lists"].append(entry)
            assert same is not False, "the device and the host road disagree"
    finally:
        shutil.rmtree(folder, ignore_errors=True)
    hot.close()
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
