"""RP / Q0 annotation: the host's second pass over the BAM against the device's pass over the pair table.

  python tools/pairs_probe.py [Mb=12] [cov=30] [--loaders 1,4,8] [--reps 3] [--out FILE.json]

A synthetic BAM in the manner of tools/bam_ingest_bench.py -- one chromosome, past 10 Mb so that the insert-size sample has
reads -- whose reads carry two CIGAR operations and the fields of a proper pair, thinned to half inside forty windows so that
the run has calls, with a .bai beside it.  Measured: the wall time of rsi_result_annotate_bam (the host pass, the code path
before this option existed) and of rsi_result_annotate_device on the same result, with the results compared; the kernel
times of the device pass; and the wall time of K concurrent BAM loads, unarmed and armed, whose difference is what
k_bam_pairs adds."""
import argparse, json, os, struct, sys, tempfile, threading, time
from concurrent.futures import ThreadPoolExecutor
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np
import bam_util as bu
from rsicnv_amd import api, synth


def synth_paired_bam(path, n, cov, read_len=100, seed=7):
    """Sorted reads of read_len - 5 M + 5 S, each with the fields of a proper FR pair (mate 300 +- 25 bases on, mapq 0 for one
    in twenty), half of them dropped inside forty windows of 5-20 kb; BGZF blocks of 0xff00 bytes cut wherever that falls, and
    the .bai (one bin, the linear index).  Built as byte arrays: a per-read Python loop takes minutes at this size."""
    rng = np.random.default_rng(seed)
    nreads = int(n * cov / read_len)
    pos = np.sort(rng.integers(1, n - 2 * read_len - 500, nreads)).astype(np.int64)
    keep = np.ones(nreads, dtype=bool)
    for s in rng.integers(n // 50, n - n // 50, 40):
        w = (pos >= s) & (pos < s + int(rng.integers(5000, 20000)))
        keep &= ~(w & (rng.random(nreads) < 0.5))
    pos = pos[keep]
    nreads = int(pos.size)
    L = read_len
    size = 4 + 32 + 9 + 8 + (L + 1) // 2 + L
    a = np.zeros((nreads, size), dtype=np.uint8)
    def put(col, fmt, values):
        v = np.asarray(values).astype(fmt)
        a[:, col:col + v.dtype.itemsize] = v.view(np.uint8).reshape(nreads, v.dtype.itemsize)
    isize = np.maximum(L + 10, rng.normal(300, 25, nreads).astype(np.int64))
    put(0, "<i4", np.full(nreads, size - 4))
    put(4, "<i4", np.zeros(nreads))
    put(8, "<i4", pos)
    a[:, 12] = 9
    a[:, 13] = np.where(rng.random(nreads) < 0.05, 0, rng.integers(20, 61, nreads))
    bins = np.full(nreads, -1, dtype=np.int64)               # reg2bin(pos, pos + L - 5): samtools' own index is built from this field
    for shift, first in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        m = (bins < 0) & ((pos >> shift) == ((pos + L - 6) >> shift))
        bins[m] = first + (pos[m] >> shift)
    put(14, "<u2", np.maximum(bins, 0))
    put(16, "<u2", np.full(nreads, 2))
    put(18, "<u2", np.full(nreads, 0x1 | 0x2 | 0x20 | 0x40))
    put(20, "<i4", np.full(nreads, L))
    put(24, "<i4", np.zeros(nreads)); put(28, "<i4", pos + isize - L); put(32, "<i4", isize)
    names = np.char.zfill(np.arange(nreads).astype("U8"), 8).astype("S8")
    a[:, 36:44] = names.view(np.uint8).reshape(nreads, 8)
    put(45, "<u4", np.full(nreads, (L - 5) << 4)); put(49, "<u4", np.full(nreads, (5 << 4) | 4))
    a[:, 53:53 + (L + 1) // 2] = 0x11
    a[:, 53 + (L + 1) // 2:] = rng.integers(14, 41, (nreads, L), dtype=np.uint8)
    data = a.tobytes()
    text = f"@HD\tVN:1.0\tSO:coordinate\n@SQ\tSN:chrS\tLN:{n}\n"
    hdr = b"BAM\1" + struct.pack("<i", len(text)) + text.encode() + struct.pack("<i", 1) + struct.pack("<i", 5) + b"chrS\0" + struct.pack("<i", n)
    step = bu.BGZF_MAX_PAYLOAD
    coffs = []
    with ThreadPoolExecutor(16) as ex, open(path, "wb") as f:
        f.write(bu._bgzf_block(hdr))
        for blk in ex.map(lambda o: bu._bgzf_block(data[o:o + step]), range(0, len(data), step)):
            coffs.append(f.tell())
            f.write(blk)
        end = f.tell()
        f.write(bu._bgzf_block(b""))
    # the .bai: record k begins at inflated byte k * size, in block k * size // step
    at = np.arange(nreads, dtype=np.int64) * size
    voff = (np.array(coffs, dtype=np.int64)[at // step] << 16) | (at % step)
    nw = int((pos[-1] + L - 5 - 1) >> 14) + 1
    lin = np.zeros(nw, dtype=np.uint64)
    for w in (pos >> 14, (pos + L - 5 - 1) >> 14):          # a read overlaps one window or two; the first read to do so wins
        first = np.unique(w, return_index=True)
        cur = lin[first[0]]
        lin[first[0]] = np.where((cur == 0) | (voff[first[1]] < cur), voff[first[1]], cur).astype(np.uint64)
    with open(path + ".bai", "wb") as f:
        f.write(b"BAI\1" + struct.pack("<i", 1) + struct.pack("<iIiQQ", 1, 4681, 1, int(voff[0]), end << 16) + struct.pack("<i", nw) + lin.astype("<u8").tobytes())
    return nreads, len(data)


def timed(fn, reps):
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        dt = (time.perf_counter() - t0) * 1e3
        best = dt if best is None or dt < best else best
    return best


def loads(ctxs, bam, armed, reps):
    for h in ctxs:
        h.set_bam_pairs(armed)
    best = None
    for rep in range(reps + 1):
        gate = threading.Barrier(len(ctxs) + 1)
        def work(h):
            gate.wait()
            h.load_depth_bam(bam, "chrS")
        th = [threading.Thread(target=work, args=(h,)) for h in ctxs]
        for t in th: t.start()
        gate.wait()
        t0 = time.perf_counter()
        for t in th: t.join()
        wall = (time.perf_counter() - t0) * 1e3
        if rep and (best is None or wall < best):           # round 0 allocates
            best = wall
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mb", nargs="?", type=float, default=12)
    ap.add_argument("cov", nargs="?", type=float, default=30)
    ap.add_argument("--loaders", default="1,4,8")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    n = int(a.mb * 1e6) + 17
    d = tempfile.mkdtemp()
    bam = os.path.join(d, "x.bam")
    t0 = time.time()
    nreads, inflated = synth_paired_bam(bam, n, a.cov)
    print(f"wrote {nreads} reads, {os.path.getsize(bam) / 1e6:.0f} MB compressed ({inflated / 1e6:.0f} MB inflated) in {time.time() - t0:.0f} s", flush=True)
    lib = api.load_library()
    fasta = synth.generate_host(lib, synth.make_plan(n=n, seed=0x5EED, model=0, n_events=0, gaps=0, end_n=0))[0]
    ks = [int(k) for k in a.loaders.split(",")]
    ctxs = [api.RsiHot(0) for _ in range(max(ks))]
    h = ctxs[0]
    h.set_bam_pairs(True)
    res = h.run_bam(api.make_params(), bam, "chrS", fasta)
    ncalls = len(res.calls("calls"))
    h.annotate_device(res)                                   # allocates
    t_dev = timed(lambda: h.annotate_device(res), a.reps)
    dev, st = res.pairs(), h.pairs_stats()
    t_host = timed(lambda: res.annotate_bam(bam, "chrS"), a.reps)
    host = res.pairs()
    assert dev == host, "the two passes disagree"
    result = {"chromosome_mb": a.mb, "coverage": a.cov, "reads": nreads, "bytes_compressed": os.path.getsize(bam), "bytes_inflated": inflated,
              "cpus": len(os.sched_getaffinity(0)), "calls": ncalls, "calls_with_rp": sum(1 for rp, _ in dev if rp > 0),
              "annotate_host_wall_ms": t_host, "annotate_device_wall_ms": t_dev, "pairs_stats": st, "loads": []}
    print(json.dumps({k: v for k, v in result.items() if k != "loads"}), flush=True)
    for k in ks:
        row = {"loaders": k, "unarmed_wall_ms": loads(ctxs[:k], bam, False, a.reps), "armed_wall_ms": loads(ctxs[:k], bam, True, a.reps)}
        row["k_bam_pairs_ms"] = ctxs[0].pairs_stats()["t_table_ms"]
        result["loads"].append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
    for c in ctxs:
        c.close()
    os.remove(bam); os.remove(bam + ".bai"); os.rmdir(d)


if __name__ == "__main__":
    main()
