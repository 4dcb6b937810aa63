"""What reading the reference costs: read_fasta's host loop plus the upload, against the device reader on a plain
FASTA and on the same file as BGZF.  Synthetic data only: a multi-sequence FASTA of about --mb megabases in --seqs sequences
(60-base lines, synth's chromosomes), the same file as BGZF (zlib, 65280-byte members, with the .gzi bgzip -i would write),
and a whole-genome depth file holding the last --depth-seqs sequences (so that the command line has something to call).

Four steps, each a process of its own, to be chained with && under a time limit each:

    python tools/ref_probe.py make  --dir D --mb 96        the files
    python tools/ref_probe.py cli   --dir D --repeat 5      `rsicnv rsi -d genome.depth` with -refread host, -refread device and
                                                            -f ref.fa.gz: wall time and the summed "timing: fasta" of the log
    python tools/ref_probe.py loads --dir D --repeat 5      rsi_ref_load_device per sequence, text and BGZF (.gzi and members walked)
    python tools/ref_probe.py report --dir D --out profiles/ref_read.json
    python tools/ref_probe.py e2e --out profiles/ref_read.json --e2e A.json B.json ...
                                                            adds the records of tools/genome_text_e2e.py --refread host|device
                                                            runs (its --out files) to the record, grouped by their reader

Every figure is the median over --repeat runs behind one warm-up run, with the minimum and maximum beside it."""
import argparse, json, os, re, statistics, struct, subprocess, sys, tempfile, time, zlib
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "rsicnv_amd", "bin", "rsicnv")
ap = argparse.ArgumentParser()
ap.add_argument("step", choices=["make", "cli", "loads", "report", "e2e"])
ap.add_argument("--e2e", nargs="*", default=[], help="step e2e: records written by tools/genome_text_e2e.py --refread ... --out")
ap.add_argument("--dir", default=os.path.join(tempfile.gettempdir(), "rsi_ref_probe"))
ap.add_argument("--mb", type=float, default=96.0, help="megabases in the FASTA")
ap.add_argument("--seqs", type=int, default=8)
ap.add_argument("--depth-seqs", type=int, default=2, help="sequences with depth lines (the last ones of the FASTA)")
ap.add_argument("--repeat", type=int, default=5)
ap.add_argument("--level", type=int, default=6, help="zlib level of the BGZF members")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ref_read.json"))
args = ap.parse_args()
FA, GZ, DEPTH = (os.path.join(args.dir, f) for f in ("ref.fa", "ref.fa.gz", "genome.depth"))


def spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4), "runs": len(xs)}


def make():
    from rsicnv_amd import api, synth
    os.makedirs(args.dir, exist_ok=True)
    import ctypes as C
    lib = api.load_library()
    lib.rsi_synth_append_genome_text.argtypes = [C.c_char_p, C.c_char_p, C.c_void_p, C.c_int64]
    n = int(args.mb * 1e6 / args.seqs)
    for f in (FA, GZ, DEPTH):
        if os.path.exists(f):
            os.unlink(f)
    fai, off, bases, t0 = [], 0, 0, time.perf_counter()
    with open(FA, "wb") as f:
        for k in range(args.seqs):
            plan = synth.make_plan(n=n + 1000 * k + 7, seed=0x9E0 + k, model=k % 2, n_events=9, gaps=1)
            fasta, depth = synth.generate_host(lib, plan)
            head = f">chr{k + 1} synthetic\n".encode()
            full = fasta.size // 60 * 60
            body = np.concatenate([fasta[:full].reshape(-1, 60), np.full((full // 60, 1), 10, dtype=np.uint8)], axis=1).tobytes()
            body += fasta[full:].tobytes() + b"\n" if full < fasta.size else b""
            f.write(head + body)
            fai.append(f"chr{k + 1}\t{fasta.size}\t{off + len(head)}\t60\t61")
            off += len(head) + len(body)
            bases += fasta.size
            if k >= args.seqs - args.depth_seqs:
                depth[-1] = 0
                if lib.rsi_synth_append_genome_text(DEPTH.encode(), f"chr{k + 1}".encode(), depth.ctypes.data, depth.size) != 0:
                    raise RuntimeError("rsi_synth_append_genome_text failed")
    for path in (FA, GZ):
        with open(path + ".fai", "w") as f:
            f.write("\n".join(fai) + "\n")
    # BGZF as bgzip writes it, and the .gzi of bgzip -i: (compressed offset, text offset) of every member but the first
    gzi, coff = [], 0
    with open(FA, "rb") as src, open(GZ, "wb") as dst:
        text_off = 0
        while True:
            raw = src.read(65280)
            if not raw:
                break
            c = zlib.compressobj(args.level, zlib.DEFLATED, -15)
            cdata = c.compress(raw) + c.flush()
            m = b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", len(cdata) + 25) + cdata + struct.pack("<II", zlib.crc32(raw), len(raw))
            if coff:
                gzi.append((coff, text_off))
            dst.write(m)
            coff += len(m); text_off += len(raw)
        gzi.append((coff, text_off))
        dst.write(bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000"))
    with open(GZ + ".gzi", "wb") as f:
        f.write(struct.pack("<Q", len(gzi)) + b"".join(struct.pack("<QQ", a, b) for a, b in gzi))
    rec = {"bases": bases, "sequences": args.seqs, "fasta_bytes": os.path.getsize(FA), "bgzf_bytes": os.path.getsize(GZ), "bgzf_level": args.level,
           "depth_sequences": args.depth_seqs, "depth_bytes": os.path.getsize(DEPTH), "make_s": round(time.perf_counter() - t0, 1)}
    json.dump(rec, open(os.path.join(args.dir, "make.json"), "w"))
    print(json.dumps(rec))


def cli():
    # run inside --dir with relative names, so that the log lines kept in the record name no directory
    modes = {"host": ["-f", "ref.fa", "-refread", "host"], "device_text": ["-f", "ref.fa", "-refread", "device"], "device_bgzf": ["-f", "ref.fa.gz"]}
    runs = {m: {"wall_s": [], "fasta_s": []} for m in modes}
    rows = {}
    for k in range(args.repeat + 1):                      # the first round warms up (page cache, first allocations)
        for mode, ref in modes.items():
            out = os.path.join(args.dir, f"out_{mode}.txt")
            t = time.perf_counter()
            r = subprocess.run([EXE, "rsi"] + ref + ["-d", "genome.depth", "-o", out, "-np"], cwd=args.dir, capture_output=True, text=True, timeout=900)
            wall = time.perf_counter() - t
            if r.returncode != 0:
                raise RuntimeError(r.stderr[-2000:])
            rows[mode] = [l for l in open(out).read().splitlines() if not l.startswith("#")]
            if k:
                runs[mode]["wall_s"].append(wall)
                runs[mode]["fasta_s"].append(sum(float(x) for x in re.findall(r"timing: fasta ([0-9.e+-]+) s", r.stderr)))
                ref_line = re.search(r"#reference: .*", r.stderr)
                runs[mode]["reference_line"] = ref_line.group(0) if ref_line else None
    rec = {m: {"wall_s": spread(v["wall_s"]), "fasta_s": spread(v["fasta_s"]), "reference_line": v.get("reference_line")} for m, v in runs.items()}
    rec["rows_match"] = rows["host"] == rows["device_text"] == rows["device_bgzf"] and len(rows["host"]) > 0
    rec["rows"] = len(rows["host"])
    json.dump(rec, open(os.path.join(args.dir, "cli.json"), "w"))
    print(json.dumps(rec))


def loads():
    import torch
    from rsicnv_amd import api
    rec = {}
    for mode, path, kw in (("text", FA, {}), ("bgzf_gzi", GZ, {}), ("bgzf_walk", GZ, {"gzi": "none"})):
        ref = api.RsiRef(path, **kw)
        seqs = [ref.sequence(i) for i in range(ref.count)]
        buf = torch.empty(max(s["length"] for s in seqs) + 64, dtype=torch.uint8, device="cuda")
        wall = {i: [] for i in range(ref.count)}
        kern = {i: [] for i in range(ref.count)}
        for k in range(args.repeat + 1):
            for i, s in enumerate(seqs):
                t = time.perf_counter()
                st = ref.load_device(i, buf.data_ptr(), buf.numel())
                w = (time.perf_counter() - t) * 1e3
                if k:
                    wall[i].append(w); kern[i].append(st["t_kernel_ms"])
        per = [{"name": s["name"], "bases": s["length"], "wall_ms": spread(wall[i]), "kernel_ms": spread(kern[i]), "bytes_read": st["bytes_read"]} for i, s in enumerate(seqs)]
        total = [sum(wall[i][k] for i in wall) for k in range(args.repeat)]
        rec[mode] = {"all_sequences_wall_ms": spread(total), "bases_per_s": round(sum(s["length"] for s in seqs) / (statistics.median(total) * 1e-3)), "per_sequence": per}
        ref.close()
    json.dump(rec, open(os.path.join(args.dir, "loads.json"), "w"))
    print(json.dumps({m: {k: v for k, v in r.items() if k != "per_sequence"} for m, r in rec.items()}))


def report():
    rec = {"what": "tools/ref_probe.py: the reference through read_fasta (host) and through the device reader, text and BGZF"}
    for part in ("make", "cli", "loads"):
        p = os.path.join(args.dir, part + ".json")
        rec[part] = json.load(open(p)) if os.path.exists(p) else None
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


def e2e():
    rec = json.load(open(args.out))
    runs = [json.load(open(p)) for p in args.e2e]
    by = {}
    for r in runs:
        by.setdefault(r["refread"], []).append(r)
    rec["genome_text_e2e"] = {
        "what": "tools/genome_text_e2e.py --refread MODE: one `rsicnv rsi -d genome.depth` process over the synthetic genome, the second of "
                "two runs of each call; the calls alternate between the readers",
        "bases": runs[0]["bases"], "chromosomes_run": runs[0]["chromosomes_run"], "whole_genome": runs[0]["whole_genome"],
        "depth_text_bytes": runs[0]["depth_text_bytes"], "workers": runs[0]["workers"], "rows_match": all(r["rows_match"] for r in runs),
        **{m: {"one_process_s": spread([r["one_process"]["s"] for r in rs]), "reader_s": spread([r["reader_s"] for r in rs])} for m, rs in by.items()}}
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec["genome_text_e2e"]))


{"make": make, "cli": cli, "loads": loads, "report": report, "e2e": e2e}[args.step]()
