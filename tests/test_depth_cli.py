"""GPU: `rsicnv depth` from the command line.  A two-chromosome BAM of a few hundred reads; the expected files are
the restatement of depth_cases applied to the depth load_depth_bam leaves in HBM.  -by W, -by FILE, -c, -nobase, -trackindex,
-trackformat text; the per-base file read back by `rsi -d` and by `depth -d`; whole-genome text, POS DEPTH with -c, bedGraph and
.gz through -d; every refusal, which leaves no file; the usage text."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import bam_util as bu
import depth_cases as dc
from test_genome_text import write_fasta

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "rsicnv_amd", "bin", "rsicnv")
N = 50_000
REFS = [("chr1", N), ("2", N)]
BGZF_EOF = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])
BED = "#regions\nchr1\t100\t600\tgeneA\n2\t0\t50\nchr2\t49990\t60000\n1\t700\t900\nchr1\t100\t600\nchr1\t60000\t70000\nchr9\t5\t10\nchr9\t7\t8\n1\t300\t300\n"


def run(*args, ok=True):
    r = subprocess.run([EXE, "depth"] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert (r.returncode == 0) == ok, r.stderr[-2000:]
    return r


@pytest.fixture(scope="module")
def case(hotlib, tmp_path_factory):
    from rsicnv_amd import api
    tmp = tmp_path_factory.mktemp("depth_cli")
    bam = str(tmp / "two.bam")
    bu.write_bam(bam, REFS, bu.synth_reads(N, coverage=0.7, seed=0xD0, ntid=2))
    hot = api.RsiHot(0)
    depth = []
    for name, _ in REFS:
        hot.load_depth_bam(bam, name)
        depth.append((name, hot.fetch("depth_in").copy()))
    hot.close()
    assert all(d.size == N and d.max() > 0 for _, d in depth)
    rng = np.random.default_rng(5)
    fa = str(tmp / "ref.fa")
    write_fasta(fa, [(name, np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)]) for name, n in REFS])
    bed = tmp / "regions.bed"
    bed.write_text(BED)
    return dict(tmp=tmp, bam=bam, depth=depth, fa=fa, bed=str(bed))


def bed_regions(name):
    """the lines of BED on `name`, in file order"""
    out = []
    for ln in BED.splitlines():
        t = ln.split()
        if not ln.startswith("#") and (t[0] == name or "chr" + t[0] == name or t[0] == "chr" + name):
            out.append((int(t[1]), int(t[2])))
    return out


def per_base_text(depth):
    out = []
    for name, d in depth:
        cut = np.flatnonzero(d[1:] != d[:-1]) + 1
        starts, ends = np.concatenate(([0], cut)), np.concatenate((cut, [d.size]))
        out += [f"{name}\t{s}\t{e}\t{d[s]}\n" for s, e in zip(starts, ends)]
    return "".join(out)


def read(path):
    return open(path).read()


def as_text(depth):
    """what the depth-text readers make of a chromosome's lines: load_data_from_text stops at POS >= n, so the last base stays 0"""
    out = []
    for name, d in depth:
        d = d.copy()
        d[-1] = 0
        out.append((name, d))
    return out


def check_tables(prefix, depth):
    assert read(prefix + ".mosdepth.summary.txt") == dc.summary_text(depth)
    assert read(prefix + ".mosdepth.global.dist.txt") == dc.dist_text(depth)


def test_by_window(case):
    p = str(case["tmp"] / "win")
    run("-b", case["bam"], "-o", p, "-by", 500, "-trackindex")
    check_tables(p, case["depth"])
    raw = open(p + ".per-base.bed.gz", "rb").read()
    assert raw.endswith(BGZF_EOF) and gzip.decompress(raw).decode() == per_base_text(case["depth"])
    raw = open(p + ".regions.bed.gz", "rb").read()
    assert raw.endswith(BGZF_EOF) and gzip.decompress(raw).decode() == "".join(dc.window_text(nm, d, 500) for nm, d in case["depth"])
    assert os.path.getsize(p + ".per-base.bed.gz.tbi") > 0 and not os.path.exists(p + ".regions.bed.gz.tbi")
    log = read(p + ".log")
    assert log.count("#depth: ") == 2 and "#depth: chr1: length 50000, mean " + dc.fixed2(int(case["depth"][0][1].sum()), N) in log and " launches, " in log
    assert "#bam:" not in log


def test_by_bed_nobase_and_device_read(case):
    p = str(case["tmp"] / "bed")
    run("-b", case["bam"], "-o", p, "-by", case["bed"], "-nobase", "-bamread", "device")
    check_tables(p, case["depth"])
    assert not os.path.exists(p + ".per-base.bed.gz")
    want = "".join(dc.region_text(nm, d, bed_regions(nm)) for nm, d in case["depth"])
    assert gzip.decompress(open(p + ".regions.bed.gz", "rb").read()).decode() == want
    assert "chr1\t60000\t70000\t0.00\n" in want and "2\t49990\t50000\t" in want and want.count("chr1\t100\t600\t") == 2 and "chr1\t300\t300\t0.00\n" in want
    log = read(p + ".log")
    assert "chr9 is not in the input: 2 lines passed over" in log and log.count("#bam: read on the device") == 2


def test_one_chromosome_as_text(case):
    p = str(case["tmp"] / "one")
    run("-b", case["bam"], "-c", "2", "-o", p, "-by", 101, "-trackformat", "text")
    check_tables(p, case["depth"][1:])
    assert read(p + ".per-base.bed") == per_base_text(case["depth"][1:]) and read(p + ".regions.bed") == dc.window_text("2", case["depth"][1][1], 101)
    assert not os.path.exists(p + ".per-base.bed.gz") and not os.path.exists(p + ".regions.bed.gz")


def test_q_filters_as_the_loader(case, hotlib):
    from rsicnv_amd import api
    hot = api.RsiHot(0)
    hot.load_depth_bam(case["bam"], "chr1", minq=30, min_baseq=20)
    d = hot.fetch("depth_in").copy()
    hot.close()
    assert d.sum() < case["depth"][0][1].sum()
    p = str(case["tmp"] / "q")
    run("-b", case["bam"], "-c", "chr1", "-o", p, "-q", 30, "-Q", 20, "-nobase")
    check_tables(p, [("chr1", d)])


def test_per_base_file_reads_back(case):
    p = str(case["tmp"] / "back")
    run("-b", case["bam"], "-o", p, "-trackindex")
    # rsi takes the file as a bedGraph depth file
    r = subprocess.run([EXE, "rsi", "-d", p + ".per-base.bed.gz", "-c", "chr1", "-f", case["fa"], "-o", str(case["tmp"] / "rsi.txt"), "-np"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "#processing chr1" in r.stderr, r.stderr[-2000:]
    assert not any(w in r.stderr for w in ("cannot", "not found", "malformed", "bad line", "unsorted"))
    # ... and so does depth itself: bedGraph in BGZF, whole and one chromosome through the index
    q = str(case["tmp"] / "back2")
    run("-d", p + ".per-base.bed.gz", "-f", case["fa"], "-o", q, "-by", 500)
    check_tables(q, as_text(case["depth"]))
    assert gzip.decompress(open(q + ".per-base.bed.gz", "rb").read()).decode() == per_base_text(as_text(case["depth"]))
    run("-d", p + ".per-base.bed.gz", "-c", "2", "-f", case["fa"], "-o", q, "-nobase")
    check_tables(q, as_text(case["depth"][1:]))
    run("-d", p + ".per-base.bed.gz", "-c", "2", "-dindex", "none", "-f", case["fa"], "-o", q, "-nobase")
    check_tables(q, as_text(case["depth"][1:]))


def test_depth_text_inputs(case):
    tmp = case["tmp"]
    genome = tmp / "genome.depth"
    genome.write_text("".join(f"{nm}\t{i + 1}\t{v}\n" for nm, d in case["depth"] for i, v in enumerate(d.tolist())))
    one = tmp / "chr1.depth"
    one.write_text("".join(f"{i + 1}\t{v}\n" for i, v in enumerate(case["depth"][0][1].tolist())))
    gz = tmp / "genome.depth.gz"
    gz.write_bytes(gzip.compress(genome.read_bytes()))
    plain_bed = tmp / "pb.bedgraph"
    plain_bed.write_text(per_base_text(case["depth"]))
    p = str(tmp / "txt")
    both = as_text(case["depth"])
    for args, want in ((("-d", genome), both), (("-d", gz), both), (("-d", one, "-c", "chr1"), both[:1]), (("-d", plain_bed), both),
                       (("-d", plain_bed, "-c", "chr1"), both[:1])):
        run(*args, "-f", case["fa"], "-o", p, "-by", case["bed"], "-trackformat", "text")
        check_tables(p, want)
        assert read(p + ".per-base.bed") == per_base_text(want)
        assert read(p + ".regions.bed") == "".join(dc.region_text(nm, d, bed_regions(nm)) for nm, d in want)


def test_refusals_leave_no_file(case):
    tmp = case["tmp"] / "refused"
    tmp.mkdir()
    bad = tmp / "bad.bed"
    bad.write_text("chr1\t5\t10\nchr1\tten\t20\n")
    p = str(tmp / "out")
    cohort = case["tmp"] / "cohort.depth"           # RNAME POS D1 D2: what -samples is for elsewhere
    cohort.write_text("".join(f"{nm}\t{i + 1}\t{v}\t{v}\n" for nm, d in case["depth"] for i, v in enumerate(d[:200].tolist())))
    cwd = os.getcwd()
    os.chdir(tmp)
    try:
        for args, msg in ((("-b", case["bam"]), "-o PREFIX"), (("-b", case["bam"], "-o", p, "-gpus", 2), "-gpus"),
                          (("-d", cohort, "-f", case["fa"], "-o", p, "-samples", "all"), "-samples"), (("-b", case["bam"], "-o", p, "-by", 0), "-by 0"),
                          (("-b", case["bam"], "-o", p, "-by", -3), "-by -3"), (("-b", case["bam"], "-o", p, "-by", tmp / "none.bed"), "cannot open"),
                          (("-b", case["bam"], "-o", p, "-by", bad), f"{bad}: line 2: start and end must be non-negative integers")):
            r = run(*args, ok=False)
            assert r.returncode == 1 and msg in r.stderr, (args, r.stderr[-500:])
            assert sorted(os.listdir(tmp)) == ["bad.bed"], args
    finally:
        os.chdir(cwd)


def test_usage_names_depth():
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=60)
    assert "rsicnv depth (-b BAMFILE | -f REFFILE -d DEPTH)" in r.stderr and "PREFIX.mosdepth.summary.txt" in r.stderr
    r = subprocess.run([EXE, "depths", "-b", "x"], capture_output=True, text=True, timeout=60)
    assert "no such function depths" in r.stderr
