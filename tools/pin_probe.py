"""`rsicnv pin` on the device, step by step, beside the reference binary on the same file and host.

  python tools/pin_probe.py [Mb=12] [cov=30] [--calls 200] [--reps 3] [--out profiles/pin_device.json]

The synthetic BAM of tools/pairs_probe.py (one chromosome past 10 Mb, reads of 95M5S with the fields of a proper pair; for the
reference it is indexed with libref.so's bam_index_build, the device needs no index) and a list of --calls deletions of 5 kb spread over it.  Measured: the BAM load unarmed, armed for
the pair table, and armed for pin (wall; HIP events for the k_bam_pin launches), rsi_hot_pin_sample and rsi_hot_pin_calls (wall
and HIP events), the `rsicnv pin` command as a whole, and `oracle/_ref/rsicnv_ref pin` on the same list where that binary
exists; START and END of the two outputs are compared row by row."""
import argparse, json, os, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
from rsicnv_amd import api
from pairs_probe import synth_paired_bam

EXE = os.path.join(ROOT, "rsicnv_amd", "bin", "rsicnv")
REF = os.path.join(ROOT, "oracle", "_ref", "rsicnv_ref")
LIBREF = os.path.join(ROOT, "oracle", "_ref", "libref.so")


def best(fn, reps):
    out, times = None, []
    for _ in range(reps):
        t = time.perf_counter()
        out = fn()
        times.append((time.perf_counter() - t) * 1e3)
    return out, min(times), times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mb", nargs="?", type=float, default=12.0)
    ap.add_argument("cov", nargs="?", type=float, default=30.0)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pin_device.json"))
    a = ap.parse_args()
    n = int(a.mb * 1e6) + 17
    with tempfile.TemporaryDirectory() as tmp:
        bam = os.path.join(tmp, "probe.bam")
        nreads, inflated = synth_paired_bam(bam, n, a.cov)
        starts = np.linspace(200_000, n - 300_000, a.calls).astype(np.int64)
        cnv = os.path.join(tmp, "probe.cnv")
        with open(cnv, "w") as f:
            for s in starts:
                f.write(f"chrS\t{s}\t{s + 5000}\tDEL\n")
        start, end, type_ = starts.astype(np.int32), (starts + 5000).astype(np.int32), np.zeros(a.calls, dtype=np.int32)
        result = {"bases": n, "coverage": a.cov, "reads": nreads, "bam_bytes": os.path.getsize(bam), "inflated_bytes": inflated, "calls": a.calls,
                  "cpus": os.cpu_count(), "reps": a.reps}
        hot = api.RsiHot(0)
        hot.load_depth_bam(bam, "chrS")                                   # the run that allocates
        for tag, arm in (("unarmed", lambda: None), ("pairs", lambda: hot.set_bam_pairs(True)), ("pin", lambda: hot.set_bam_pin(True))):
            arm()
            hot.load_depth_bam(bam, "chrS")
            _, ms, every = best(lambda: hot.load_depth_bam(bam, "chrS"), a.reps)
            result["load_" + tag + "_ms"] = ms
            result["load_" + tag + "_all_ms"] = every
        st = hot.pin_stats()
        result.update(table_bytes=st["table_bytes"], pool_words=st["pool_words"], t_table_ms=st["t_table_ms"])
        sample, ms, _ = best(hot.pin_sample, a.reps)
        result.update(sample_wall_ms=ms, sample_kernels_ms=sample["t_sample_ms"], l_qseq=sample["l_qseq"], rd=sample["rd"], rd_sd=sample["rd_sd"],
                      drd=sample["drd"], drd_sd=sample["drd_sd"], sample_reads=sample["sample_reads"])
        got, ms, _ = best(lambda: hot.pin_calls(101, start, end, type_), a.reps)
        st = hot.pin_stats()
        result.update(windows_wall_ms=ms, windows_kernel_ms=st["t_windows_ms"], breakpoints=st["breakpoints"], r_len=st["r_len"],
                      moved=int(np.sum(got[0] != start) + np.sum(got[1] != end)))
        hot.close()
        out = os.path.join(tmp, "dev.txt")
        _, ms, _ = best(lambda: subprocess.run([EXE, "pin", "-b", bam, "-v", cnv, "-o", out], check=True, capture_output=True), 1)
        result["command_wall_ms"] = ms
        dev_rows = [ln.split("\t")[1:3] for ln in open(out).read().splitlines()]
        assert dev_rows == [[str(s), str(e)] for s, e in zip(got[0].tolist(), got[1].tolist())]
        if os.path.exists(REF) and os.path.exists(LIBREF):
            import ctypes
            L = ctypes.CDLL(LIBREF)                                      # the reference's own index: its iterator wants every bin
            L.bam_index_build.argtypes = [ctypes.c_char_p]
            t = time.perf_counter()
            result["reference_index_exit"] = L.bam_index_build(os.fsencode(bam))
            result["reference_index_ms"] = (time.perf_counter() - t) * 1e3
            ref_out = os.path.join(tmp, "ref.txt")
            r, ms, _ = best(lambda: subprocess.run([REF, "pin", "-b", bam, "-v", cnv, "-o", ref_out], capture_output=True, cwd=tmp), 1)
            result["reference_wall_ms"] = ms
            result["reference_exit"] = r.returncode
            if r.returncode == 0 and os.path.exists(ref_out):
                ref_rows = [ln.split("\t")[1:3] for ln in open(ref_out).read().splitlines() if ln and not ln.startswith("#")]
                result["rows_match_reference"] = ref_rows == dev_rows
    print(json.dumps(result), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
