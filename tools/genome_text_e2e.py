"""End to end from ONE whole-genome depth file: the 24 chromosomes of configs[N - 1] written as a single "RNAME pos depth" file
(samtools depth -a's layout, about 17 bytes per base) plus one FASTA, then one `rsicnv rsi -f REF -d genome.depth -o OUT -np`
process -- reading, device parse and detection of all chromosomes overlapped inside it.  Compare with tools/e2e_genome.py
(one process per chromosome on per-chromosome files, profiles/r5_e2e_genome.json).  When the scratch directory cannot hold
the whole genome, the largest prefix of chromosomes (in file order) that fits is run, and the record says so.

rows_match: the process's rows equal those of every chromosome run on its own through the library (depth from the arrays,
last base 0 as the text path leaves it, App. A Q7), concatenated in file order.

--compress bgzf writes the file as BGZF (rsi_synth_append_genome_bgzf: bgzip's layout, level 6, 16 host threads; the
process inflates it on the device), --compress gzip as ordinary gzip (one member per chromosome; inflated on the host).

usage: genome_text_e2e.py [--dir SCRATCH] [--out JSON] [--config 4] [--workers 4] [--max-gb G] [--compress none|bgzf|gzip]"""
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
args = ap.parse_args()

lib = api.load_library()
lib.rsi_synth_append_genome_text.argtypes = [C.c_char_p, C.c_char_p, C.c_void_p, C.c_int64]
lib.rsi_synth_append_genome_bgzf.argtypes = [C.c_char_p, C.c_char_p, C.c_void_p, C.c_int64]
bytes_per_base = {"none": 19.5, "bgzf": 5.5, "gzip": 5.5 + 17.5 / 24}[args.compress]   # file + FASTA, margin (gzip: one chromosome's text at a time)
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
for p in (genome, fa):
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


def run_once(tag):
    out = os.path.join(args.dir, f"out_{tag}.txt")
    t = time.perf_counter()
    r = subprocess.run([exe, "rsi", "-f", fa, "-d", genome, "-o", out, "-np", "-workers", str(args.workers)] + flag_args,
                       capture_output=True, text=True, timeout=1800)
    wall = time.perf_counter() - t
    if r.returncode != 0:
        raise RuntimeError(r.stderr[-2000:])
    m = re.search(r"timing: whole-genome depth text ([0-9.e+-]+) s, (\d+) chromosomes, boundary kernels ([0-9.e+-]+) ms, parse kernels ([0-9.e+-]+) ms", r.stderr)
    z = re.search(r"#depth file: (\w+), (\d+) compressed bytes, (\d+) text bytes, inflate ([0-9.e+-]+) ms", r.stderr)
    return out, wall, m, z


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
       "calls": len(rows), "rows_match": rows == own_rows,
       "compare": "profiles/r5_e2e_genome.json: one process per chromosome, 1.85e8 bases/s one at a time, 5.75e8 with four at once",
       "note": "rsicnv rsi -f REF -d genome.depth -o OUT -np: process start, FASTA reads, one pass of the depth text through the device, "
               "detection of every chromosome on a pool, one output file; second of two runs (the file in the page cache as far as it holds it)"}
if args.out:
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
print(json.dumps(rec), flush=True)
shutil.rmtree(args.dir, ignore_errors=True)
