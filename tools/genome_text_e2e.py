"""End to end from ONE whole-genome depth file: the 24 chromosomes of configs[N - 1] written as a single "RNAME pos depth" file
(samtools depth -a's layout, about 17 bytes per base) plus one FASTA, then one `rsicnv rsi -f REF -d genome.depth -o OUT -np`
process -- reading, device parse and detection of all chromosomes overlapped inside it.  Compare with tools/e2e_genome.py
(one process per chromosome on per-chromosome files, profiles/r5_e2e_genome.json).  When the scratch directory cannot hold
the whole genome, the largest prefix of chromosomes (in file order) that fits is run, and the record says so.

rows_match: the process's rows equal those of every chromosome run on its own through the library (depth from the arrays,
last base 0 as the text path leaves it, App. A Q7), concatenated in file order.

--compress bgzf writes the file as BGZF (rsi_synth_append_genome_bgzf: bgzip's layout, level 6, 16 host threads; the
process inflates it on the device), --compress gzip as ordinary gzip (one member per chromosome; inflated on the host).

--samples K writes a cohort file instead, "RNAME pos d1 ... dK" (rsi_synth_append_genome_samples; sample s's depth is the
config's chromosome with the seed and mean shifted, the FASTA is sample 1's), and runs it once through `-samples all`
(warm-up run, then the timed one).  Then, one at a time to bound the disk, each derived single-sample file (the same lines
with column k alone) is written, run the same way and deleted; the rows of OUT.k must equal that run's.  The record
(default profiles/e2e_genome_samples.json) holds the cohort run's wall time against the sum of the K single-sample runs'.

--format bedgraph also writes the same depth as a bedGraph file, "RNAME start end d" per run of equal depth
(rsi_synth_append_genome_bedgraph: mosdepth's layout; --compress none or bgzf), runs `rsicnv rsi -d genome.bed[.gz]` and the
per-base file in the same call, and records both: wall time, text bytes per base, parse kernel time and text bytes parsed
per second.  The synthetic depth is i.i.d. per base, so its runs are about one base long and the bedGraph text is LARGER
than the per-base one; compare bytes parsed per second, not only wall time (real mosdepth files are smaller per base).

--index-read K times `-d FILE.bed.gz -c RNAME` by index and nothing else: the first K chromosomes of the config,
shrunk by --index-scale, are written as one BGZF bedGraph by the project's own track writer with its .tbi
(rsi_hot_write_track_device, rsi_track_index_write_tbi), and the LAST one is read `--index-repeat` times with the index and
with -dindex none, alternating after a warm-up pair.  The record holds the medians of the wall time and of the log's inflate
figures, and says whether the rows agree.

usage: genome_text_e2e.py [--dir SCRATCH] [--out JSON] [--config 4] [--workers 4] [--max-gb G] [--compress none|bgzf|gzip]
                          [--samples K] [--format depth|bedgraph] [--index-read K [--index-scale S] [--index-repeat R]]
                          [--refread host|device]

--refread host|device passes -refread to the timed whole-genome run (the reference through read_fasta or through the device
reader), so that two calls compare the two end to end."""
import argparse, json, os, re, shutil, subprocess, sys, tempfile, time, zlib
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ctypes as C
import numpy as np
import torch
from rsicnv_amd import api, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--dir", default=os.path.join(tempfile.gettempdir(), "rsi_genome_e2e"))
ap.add_argument("--out", default=None, help="also write the record to this JSON file (default: the JSON line on stdout only)")
ap.add_argument("--config", type=int, default=4)
ap.add_argument("--workers", type=int, default=4)
ap.add_argument("--max-gb", type=float, default=0.0, help="cap on the bytes of files (0: what the scratch directory has free, minus 4 GB)")
ap.add_argument("--compress", choices=["none", "bgzf", "gzip"], default="none")
ap.add_argument("--samples", type=int, default=0, help="K > 0: a K-column cohort file through -samples all, against its K derived files")
ap.add_argument("--format", choices=["depth", "bedgraph"], default="depth",
                help="bedgraph: also a bedGraph file of the same depth, run beside the per-base one")
ap.add_argument("--index-read", type=int, default=0, help="K > 0: only time -c on the last of K chromosomes of a BGZF bedGraph, with and without its index")
ap.add_argument("--index-scale", type=float, default=0.05, help="--index-read: shrinks the chromosomes")
ap.add_argument("--index-repeat", type=int, default=3)
ap.add_argument("--refread", choices=["host", "device"], default=None,
                help="the timed whole-genome run with -refread host or device (DESIGN.md 6j); default: the command line's own default")
args = ap.parse_args()
if args.format == "bedgraph" and (args.samples > 0 or args.compress == "gzip"):
    raise SystemExit("genome_text_e2e: --format bedgraph takes --compress none or bgzf, without --samples")
if args.samples > 0 and args.out is None:
    args.out = os.path.join(ROOT, "profiles", "e2e_genome_samples.json")



def index_read():
    """-c on the last chromosome of a K-chromosome BGZF bedGraph the track writer wrote and indexed: by index, and without."""
    import statistics
    K = args.index_read
    os.makedirs(args.dir, exist_ok=True)
    lib = api.load_library()
    exe = os.path.join(ROOT, "rsicnv_amd", "bin", "rsicnv")
    bed, fa = os.path.join(args.dir, "indexed.bed.gz"), os.path.join(args.dir, "indexed_ref.fa")
    for f in (bed, bed + ".tbi"):
        if os.path.exists(f):
            os.unlink(f)
    hot = api.RsiHot(0)
    hot.set_track_format("bgzf")
    ix = api.TrackIndex()
    hot.set_track_index(ix)
    bases, t0 = 0, time.perf_counter()
    for c in range(K):
        plan = synth.config_plan(args.config, chrom=c, scale=args.index_scale)
        n = plan["n"]
        d_fa = torch.empty(n + 64, dtype=torch.uint8, device="cuda")
        d_rd = torch.empty(n + 16, dtype=torch.int32, device="cuda")
        synth.generate_device(lib, plan, d_fa.data_ptr(), d_rd.data_ptr())
        torch.cuda.synchronize()
        hot.write_track_device(d_rd.data_ptr(), n, f"chr{c + 1}", bed, append=True)
        bases += n
        if c == K - 1:                                  # the FASTA of the chromosome that is read, 60 columns a line, and its .fai
            seq = d_fa[:n].cpu().numpy()
            head = f">chr{K}\n".encode()
            with open(fa, "wb") as f:
                f.write(head)
                full = n // 60 * 60
                body = np.concatenate([seq[:full].reshape(-1, 60), np.full((full // 60, 1), 10, dtype=np.uint8)], axis=1).tobytes()
                f.write(body + (seq[full:].tobytes() + b"\n" if full < n else b""))
            with open(fa + ".fai", "w") as f:
                f.write(f"chr{K}\t{n}\t{len(head)}\t60\t61\n")
            last_n = n
    hot.set_track_index(None)
    hot.close()
    api.bgzf_write_eof(bed)
    ix.write_tbi(bed + ".tbi")
    t_files = time.perf_counter() - t0
    flags = synth.config_flags(args.config)
    flag_args = ["-m", str(flags["m"])] + (["-MED"] if flags.get("trans", 0) == 1 else []) + (["-cap", str(flags["cap"])] if "cap" in flags else [])
    runs = {"indexed": [], "whole": []}
    rows = {}
    for k in range(args.index_repeat + 1):              # the first pair warms up (page cache, first allocations)
        for mode in ("whole", "indexed"):
            out = os.path.join(args.dir, f"indexed_{mode}.txt")
            t = time.perf_counter()
            r = subprocess.run([exe, "rsi", "-f", fa, "-d", bed, "-c", f"chr{K}", "-o", out, "-np", "-workers", str(args.workers)] + flag_args +
                               (["-dindex", "none"] if mode == "whole" else []), capture_output=True, text=True, timeout=1800)
            wall = time.perf_counter() - t
            if r.returncode != 0:
                raise RuntimeError(r.stderr[-2000:])
            z = re.search(r"#depth file: (\w+), (\d+) compressed bytes, (\d+) text bytes, inflate ([0-9.e+-]+) ms", r.stderr)
            rows[mode] = [l for l in open(out).read().splitlines() if not l.startswith("#")]
            if k:
                runs[mode].append({"s": wall, "compressed_bytes": int(z.group(2)), "text_bytes": int(z.group(3)), "inflate_ms": float(z.group(4))})
    med = lambda xs: round(statistics.median(xs), 4)
    rec = {"what": f"tools/genome_text_e2e.py --index-read {K} --index-scale {args.index_scale}: rsicnv rsi -d indexed.bed.gz -c chr{K} with "
                   "indexed.bed.gz.tbi beside the file, and with -dindex none; medians of alternating runs after a warm-up pair",
           "chromosomes": K, "bases": bases, "bases_of_the_chromosome_read": last_n, "file_bytes": os.path.getsize(bed),
           "tbi_bytes": os.path.getsize(bed + ".tbi"), "files_written_in_s": round(t_files, 1), "index": ix.counts(), "rows_match": rows["indexed"] == rows["whole"],
           "calls": len(rows["whole"])}
    for mode, rs in runs.items():
        rec[mode] = {"s": med([x["s"] for x in rs]), "all_s": [round(x["s"], 4) for x in rs], "compressed_bytes": rs[0]["compressed_bytes"],
                     "text_bytes": rs[0]["text_bytes"], "inflate_ms": med([x["inflate_ms"] for x in rs])}
    ix.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
    print(json.dumps(rec), flush=True)
    shutil.rmtree(args.dir, ignore_errors=True)


if args.index_read > 0:
    index_read()
    raise SystemExit(0)

lib = api.load_library()
lib.rsi_synth_append_genome_text.argtypes = [C.c_char_p, C.c_char_p, C.c_void_p, C.c_int64]
lib.rsi_synth_append_genome_bgzf.argtypes = [C.c_char_p, C.c_char_p, C.c_void_p, C.c_int64]
lib.rsi_synth_append_genome_samples.argtypes = [C.c_char_p, C.c_char_p, C.c_void_p, C.c_int, C.c_int64, C.c_int]
lib.rsi_synth_append_genome_bedgraph.argtypes = [C.c_char_p, C.c_char_p, C.c_void_p, C.c_int64, C.c_int]
bytes_per_base = {"none": 19.5, "bgzf": 5.5, "gzip": 5.5 + 17.5 / 24}[args.compress]   # file + FASTA, margin (gzip: one chromosome's text at a time)
if args.samples > 0:   # the cohort file (~4 more text bytes per sample) and one derived file at a time
    bytes_per_base = {"none": 19.5 + 4.5 * (args.samples - 1) + 18.5, "bgzf": 5.5 + 1.5 * (args.samples - 1) + 4.5,
                      "gzip": 5.5 + 1.5 * (args.samples - 1) + 4.5 + (17.5 + 4.5 * args.samples) / 24}[args.compress]
if args.format == "bedgraph":   # one-base runs: ~27 bytes of bedGraph text per base (~8 as BGZF) beside the per-base file
    bytes_per_base += {"none": 28.0, "bgzf": 8.5}[args.compress]
os.makedirs(args.dir, exist_ok=True)
free = shutil.disk_usage(args.dir).free
budget = (args.max_gb * (1 << 30)) if args.max_gb > 0 else max(0, free - 4 * (1 << 30))
plans = [synth.config_plan(args.config, chrom=c) for c in range(24)]
chosen, need = [], 0
for c in range(24):                 # file order: chr1 .. chr24, the prefix that fits
    b = int(plans[c]["n"] * bytes_per_base)   # ~17 bytes of text per base (or ~4 compressed) + 1 of FASTA, with margin
    if need + b > budget:
        break
    chosen.append(c); need += b
if not chosen:
    raise SystemExit(f"genome_text_e2e: {free / 1e9:.1f} GB free under {args.dir}: not even the first chromosome fits")
flags = synth.config_flags(args.config)
exe = os.path.join(ROOT, "rsicnv_amd", "bin", "rsicnv")
flag_args = ["-m", str(flags["m"])] + (["-MED"] if flags.get("trans", 0) == 1 else []) + (["-cap", str(flags["cap"])] if "cap" in flags else [])
params = api.make_params(**flags)

genome, fa = os.path.join(args.dir, "genome.depth"), os.path.join(args.dir, "ref.fa")
bed = os.path.join(args.dir, "genome.bed" + (".gz" if args.compress == "bgzf" else ""))


def append_lines(path, name, depths):
    """depths: K x n int32 (K = 1: a three-column file) appended to `path` in the --compress form."""
    depths = np.ascontiguousarray(depths, dtype=np.int32)
    k, n = depths.shape
    if args.compress == "gzip":
        part = path + ".part"
        if lib.rsi_synth_append_genome_samples(part.encode(), name.encode(), depths.ctypes.data, k, n, 0) != 0:
            raise RuntimeError("rsi_synth_append_genome_samples failed")
        z = zlib.compressobj(6, zlib.DEFLATED, 31)
        with open(part, "rb") as fi, open(path, "ab") as fo:
            for blk in iter(lambda: fi.read(16 << 20), b""):
                fo.write(z.compress(blk))
            fo.write(z.flush())
        os.remove(part)
    elif lib.rsi_synth_append_genome_samples(path.encode(), name.encode(), depths.ctypes.data, k, n, int(args.compress == "bgzf")) != 0:
        raise RuntimeError("rsi_synth_append_genome_samples failed")


def sample_depth(c, s, d_fa=None):
    """Sample s (0-based) of chromosome c on the device: the config's plan, seed and mean shifted for s > 0; the last base 0."""
    p = dict(plans[c])
    if s:
        p.update(seed=p["seed"] + 0x1000 * s, mean=p["mean"] * (1.0 + 0.15 * s))
    d_rd = torch.empty(p["n"] + 16, dtype=torch.int32, device="cuda")
    scratch = d_fa if d_fa is not None else torch.empty(p["n"] + 64, dtype=torch.uint8, device="cuda")
    synth.generate_device(lib, p, scratch.data_ptr(), d_rd.data_ptr())
    d_rd[p["n"] - 1] = 0        # the text path never sets the last base (App. A Q7)
    torch.cuda.synchronize()
    return d_rd


def run_cli(depth_file, out, extra):
    t = time.perf_counter()
    r = subprocess.run([exe, "rsi", "-f", fa, "-d", depth_file, "-o", out, "-np", "-workers", str(args.workers)] + flag_args + extra,
                       capture_output=True, text=True, timeout=3600)
    wall = time.perf_counter() - t
    if r.returncode != 0:
        raise RuntimeError(r.stderr[-2000:])
    m = re.search(r"timing: whole-genome depth text ([0-9.e+-]+) s, (\d+) chromosomes, boundary kernels ([0-9.e+-]+) ms, parse kernels ([0-9.e+-]+) ms", r.stderr)
    return wall, m


def rows_of(path):
    return [l for l in open(path).read().splitlines() if not l.startswith("#")]


if args.samples > 0:
    K = args.samples
    for p in (genome, fa):
        if os.path.exists(p):
            os.remove(p)
    torch.cuda.set_device(0)
    t0 = time.time()
    fai, off = [], 0
    with open(fa, "wb") as ff:
        for c in chosen:
            name = f"chr{c + 1}"
            d_fa = torch.empty(plans[c]["n"] + 64, dtype=torch.uint8, device="cuda")
            depths = np.stack([sample_depth(c, s, d_fa if s == 0 else None)[:plans[c]["n"]].cpu().numpy() for s in range(K)])
            fasta = d_fa[:plans[c]["n"]].cpu().numpy()
            del d_fa
            append_lines(genome, name, depths)
            head = f">{name}\n".encode()
            ff.write(head); off += len(head)
            full = (fasta.size // 60) * 60
            body = np.concatenate([fasta[:full].reshape(-1, 60), np.full((full // 60, 1), 10, np.uint8)], axis=1).tobytes()
            if fasta.size > full:
                body += fasta[full:].tobytes() + b"\n"
            ff.write(body)
            fai.append(f"{name}\t{fasta.size}\t{off}\t60\t61")
            off += len(body)
            del fasta, depths
    with open(fa + ".fai", "w") as f:
        f.write("\n".join(fai) + "\n")
    torch.cuda.empty_cache()
    t_files = time.time() - t0
    bases = sum(plans[c]["n"] for c in chosen)
    cohort_bytes = os.path.getsize(genome)
    print(f"[genome_text_e2e] cohort of {K}: {len(chosen)} of 24 chromosomes, {bases / 1e9:.3f} Gb, {cohort_bytes / 1e9:.1f} GB "
          f"{args.compress} file written in {t_files:.0f} s", flush=True)
    out = os.path.join(args.dir, "cohort.txt")
    run_cli(genome, out, ["-samples", "all"])                # page cache, the device's first allocations
    wall, m = run_cli(genome, out, ["-samples", "all"])
    cohort_rows = {k: rows_of(f"{out}.{k}") for k in range(1, K + 1)}
    cohort_text = int(re.search(r"(\d+) text bytes", open(out + ".log").read()).group(1)) if args.compress != "none" else cohort_bytes
    singles, rows_equal = [], {}
    os.remove(genome)
    for k in range(1, K + 1):   # derived file k: the same lines with column k alone, written from the same depths
        one = os.path.join(args.dir, f"derived_{k}.depth")
        for c in chosen:
            append_lines(one, f"chr{c + 1}", sample_depth(c, k - 1)[:plans[c]["n"]].cpu().numpy()[None, :])
        torch.cuda.empty_cache()
        o1 = os.path.join(args.dir, f"one_{k}.txt")
        run_cli(one, o1, [])
        w1, m1 = run_cli(one, o1, [])
        size = os.path.getsize(one)
        os.remove(one)
        rows_equal[k] = rows_of(o1) == cohort_rows[k]
        singles.append({"sample": k, "s": round(w1, 3), "file_bytes": size, "reader_s": float(m1.group(1)) if m1 else None,
                        "parse_kernels_ms": float(m1.group(4)) if m1 else None, "calls": len(rows_of(o1))})
        print(f"[genome_text_e2e] derived file {k}: {w1:.2f} s, rows equal: {rows_equal[k]}", flush=True)
    sum_single = sum(x["s"] for x in singles)
    parse_ms = float(m.group(4)) if m else None
    single_parse = [x["parse_kernels_ms"] for x in singles if x["parse_kernels_ms"]]
    rec = {"what": f"tools/genome_text_e2e.py --samples {K} --compress {args.compress}: one {K}-column cohort file through "
                   f"`rsicnv rsi -d COHORT -samples all`, against the {K} derived single-sample files run one after the other in the same session",
           "config": f"configs[{args.config - 1}]: {flags}", "chromosomes_run": len(chosen), "chromosomes_of_genome": 24, "bases": bases,
           "whole_genome": len(chosen) == 24, "genome_used": f"chr1..chr{len(chosen)} of the 3 Gb synthetic genome, {bases / 1e9:.3f} Gb "
                                                           f"(--max-gb {args.max_gb}: the files must fit)",
           "samples": K, "compress": args.compress, "workers": args.workers, "cohort_file_bytes": cohort_bytes, "cohort_text_bytes": cohort_text,
           "files_written_in_s": round(t_files, 1),
           "cohort": {"s": round(wall, 3), "reader_s": float(m.group(1)) if m else None,
                      "boundary_kernels_ms": float(m.group(3)) if m else None, "parse_kernels_ms": parse_ms,
                      "parse_kernel_text_bytes_per_s": round(cohort_text / (parse_ms * 1e-3), 1) if parse_ms else "not measured",
                      "sample_bases_per_s": round(K * bases / wall, 1)},
           "single_sample_runs": singles, "sum_single_s": round(sum_single, 3),
           "single_parse_kernel_text_bytes_per_s": round(sum(x["file_bytes"] for x in singles) / (sum(single_parse) * 1e-3), 1)
           if len(single_parse) == K and args.compress == "none" else "not measured",
           "cohort_over_sum": round(wall / sum_single, 3), "bar_met": wall < sum_single,
           "rows_equal": all(rows_equal.values()), "rows_equal_per_sample": rows_equal,
           "calls_per_sample": {k: len(v) for k, v in cohort_rows.items()},
           "compare": "profiles/e2e_genome_bgzf.json: one text run of the whole genome, 3.3e8 bases/s",
           "note": "wall times of whole processes (start, FASTA reads, one pass over the depth file, detection, output); each the "
                   "second of two runs of the same file (the file in the page cache as far as it holds it)"}
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec), flush=True)
    shutil.rmtree(args.dir, ignore_errors=True)
    sys.exit(0)

for p in (genome, fa, bed):
    if os.path.exists(p):
        os.remove(p)
torch.cuda.set_device(0)
pool = api.RsiPool(0, args.workers)
t0 = time.time()
fai, off, own_rows = [], 0, []
with open(fa, "wb") as ff:
    for c in chosen:
        p = plans[c]
        name = f"chr{c + 1}"
        d_fa = torch.empty(p["n"] + 64, dtype=torch.uint8, device="cuda"); d_rd = torch.empty(p["n"] + 16, dtype=torch.int32, device="cuda")
        synth.generate_device(lib, p, d_fa.data_ptr(), d_rd.data_ptr())
        d_rd[p["n"] - 1] = 0        # the text path never sets the last base (App. A Q7)
        torch.cuda.synchronize()
        own_rows += pool.run(params, [(d_rd.data_ptr(), d_fa.data_ptr(), p["n"])])[0].format_rows(name)
        fasta = d_fa[:p["n"]].cpu().numpy(); depth = d_rd[:p["n"]].cpu().numpy()
        del d_fa, d_rd
        depth[p["n"] - 1] = 0
        if args.compress == "bgzf":
            if lib.rsi_synth_append_genome_bgzf(genome.encode(), name.encode(), depth.ctypes.data, depth.size) != 0:
                raise RuntimeError("rsi_synth_append_genome_bgzf failed")
        elif args.compress == "gzip":
            part = genome + ".part"
            if lib.rsi_synth_append_genome_text(part.encode(), name.encode(), depth.ctypes.data, depth.size) != 0:
                raise RuntimeError("rsi_synth_append_genome_text failed")
            z = zlib.compressobj(6, zlib.DEFLATED, 31)
            with open(part, "rb") as fi, open(genome, "ab") as fo:
                for blk in iter(lambda: fi.read(16 << 20), b""):
                    fo.write(z.compress(blk))
                fo.write(z.flush())
            os.remove(part)
        elif lib.rsi_synth_append_genome_text(genome.encode(), name.encode(), depth.ctypes.data, depth.size) != 0:
            raise RuntimeError("rsi_synth_append_genome_text failed")
        if args.format == "bedgraph" and lib.rsi_synth_append_genome_bedgraph(bed.encode(), name.encode(), depth.ctypes.data, depth.size,
                                                                             int(args.compress == "bgzf")) != 0:
            raise RuntimeError("rsi_synth_append_genome_bedgraph failed")
        head = f">{name}\n".encode()
        ff.write(head); off += len(head)
        full = (fasta.size // 60) * 60
        body = np.concatenate([fasta[:full].reshape(-1, 60), np.full((full // 60, 1), 10, np.uint8)], axis=1).tobytes()
        if fasta.size > full:
            body += fasta[full:].tobytes() + b"\n"
        ff.write(body)
        fai.append(f"{name}\t{fasta.size}\t{off}\t60\t61")
        off += len(body)
        del fasta, depth
with open(fa + ".fai", "w") as f:
    f.write("\n".join(fai) + "\n")
pool.close()
torch.cuda.empty_cache()
t_files = time.time() - t0
bases = sum(plans[c]["n"] for c in chosen)
file_bytes = os.path.getsize(genome)
print(f"[genome_text_e2e] {len(chosen)} of 24 chromosomes, {bases / 1e9:.3f} Gb, {file_bytes / 1e9:.1f} GB of {args.compress} depth file written in {t_files:.0f} s", flush=True)


def run_once(tag, depth_file=genome):
    out = os.path.join(args.dir, f"out_{tag}.txt")
    t = time.perf_counter()
    r = subprocess.run([exe, "rsi", "-f", fa, "-d", depth_file, "-o", out, "-np", "-workers", str(args.workers)] + flag_args +
                       (["-refread", args.refread] if args.refread else []), capture_output=True, text=True, timeout=1800)
    wall = time.perf_counter() - t
    if r.returncode != 0:
        raise RuntimeError(r.stderr[-2000:])
    m = re.search(r"timing: whole-genome depth text ([0-9.e+-]+) s, (\d+) chromosomes, boundary kernels ([0-9.e+-]+) ms, parse kernels ([0-9.e+-]+) ms", r.stderr)
    z = re.search(r"#depth file: (\w+), (\d+) compressed bytes, (\d+) text bytes, inflate ([0-9.e+-]+) ms", r.stderr)
    return out, wall, m, z


if args.format == "bedgraph":
    run_once("bed_warm", bed)
    b_out, b_wall, b_m, b_z = run_once("bed_timed", bed)
run_once("warm")                    # page cache, the device's first allocations
out, wall, m, z = run_once("timed")
text_bytes = int(z.group(3)) if z else file_bytes
# depth-file bytes over PCIe: the text (plain text; gzip, inflated on the host), or the members' deflate payloads (BGZF)
pcie_bytes = int(z.group(2)) if (z and args.compress == "bgzf") else text_bytes
rows = [l for l in open(out).read().splitlines() if not l.startswith("#")]
rec = {"config": f"configs[{args.config - 1}]: {flags}", "chromosomes_run": len(chosen), "chromosomes_of_genome": 24, "bases": bases,
       "whole_genome": len(chosen) == 24, "compress": args.compress, "depth_text_bytes": text_bytes, "depth_file_bytes": file_bytes,
       "pcie_depth_bytes": pcie_bytes, "inflate_ms": float(z.group(4)) if z else None,
       "inflate_where": {"none": None, "bgzf": "device (summed kernel time)", "gzip": "host zlib (wall time)"}[args.compress],
       "scratch_free_bytes_at_start": free,
       "page_cache_may_hold_file": file_bytes < os.sysconf("SC_PAGE_SIZE") * os.sysconf("SC_PHYS_PAGES") * 0.8,
       "files_written_in_s": round(t_files, 1), "workers": args.workers,
       "one_process": {"s": round(wall, 3), "bases_per_s": round(bases / wall, 1), "text_bytes_per_s": round(text_bytes / wall, 1)},
       "reader_s": float(m.group(1)) if m else None, "boundary_kernels_ms": float(m.group(3)) if m else None,
       "parse_kernels_ms": float(m.group(4)) if m else None,
       "calls": len(rows), "rows_match": rows == own_rows, "refread": args.refread or "default",
       "compare": "profiles/r5_e2e_genome.json: one process per chromosome, 1.85e8 bases/s one at a time, 5.75e8 with four at once",
       "note": "rsicnv rsi -f REF -d genome.depth -o OUT -np: process start, FASTA reads, one pass of the depth text through the device, "
               "detection of every chromosome on a pool, one output file; second of two runs (the file in the page cache as far as it holds it)"}
if args.format == "bedgraph":
    def side(path, wall_s, mm, zz):
        tb = int(zz.group(3)) if zz else os.path.getsize(path)
        pm = float(mm.group(4)) if mm else None
        return {"file_bytes": os.path.getsize(path), "text_bytes": tb, "text_bytes_per_base": round(tb / bases, 3), "s": round(wall_s, 3),
                "bases_per_s": round(bases / wall_s, 1), "parse_kernels_ms": pm, "boundary_kernels_ms": float(mm.group(3)) if mm else None,
                "parse_kernel_text_GB_per_s": round(tb / (pm * 1e-3) / 1e9, 3) if pm else "not measured",
                "inflate_ms": float(zz.group(4)) if zz else None}
    b_rows = [l for l in open(b_out).read().splitlines() if not l.startswith("#")]
    rec = {"what": f"tools/genome_text_e2e.py --format bedgraph --compress {args.compress}: the same depth as a bedGraph file "
                   "(one line per run of equal depth, mosdepth's layout) and as per-base RNAME POS DEPTH lines, each through one "
                   "`rsicnv rsi -d FILE` process",
           "config": rec["config"], "chromosomes_run": len(chosen), "chromosomes_of_genome": 24, "bases": bases,
           "whole_genome": len(chosen) == 24, "compress": args.compress, "workers": args.workers,
           "bedgraph": side(bed, b_wall, b_m, b_z), "per_base": side(genome, wall, m, z), "calls": len(rows),
           "rows_match": b_rows == rows == own_rows, "bedgraph_rows_equal_per_base_rows": b_rows == rows,
           "caution": "synthetic depth is i.i.d. per base: its runs are about one base long, so the bedGraph text is larger than the "
                      "per-base text; compare text bytes parsed per second.  Real mosdepth files are smaller per base (not measured here).",
           "note": rec["note"]}
if args.out:
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
print(json.dumps(rec), flush=True)
shutil.rmtree(args.dir, ignore_errors=True)
