"""GPU: `rsicnv geno` on the device.  The debug hook on every case of geno_cases in both storages, every field of
every record against the Python restatement; lists that grow and shrink on one context; the launch counts; a 2 Mb synthetic
chromosome with two N runs, a planted deletion and a planted duplication, whose records equal the restatement on the fetched
compacted depth and removed regions; the command line on every input route; and an unarmed context, which holds nothing."""
import os
import subprocess

import numpy as np
import pytest

import bam_util as bu
import bgzf_util as bz
import geno_cases as gc
from test_genome_text import write_fasta

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "rsicnv_amd", "bin", "rsicnv")
CASES = gc.cases()
M = 101


@pytest.fixture(scope="module")
def hot(hotlib):
    from rsicnv_amd import api
    h = api.RsiHot(0)
    yield h
    h.close()


@pytest.fixture(scope="module")
def restated():
    return {name: [gc.record(c.depth, j) for j in c.jobs] for name, c in CASES.items()}


def expected_passes(case, storage):
    """bytes: one histogram pass; int32: 11 bits of the widest max - min per pass, none when every range is empty or flat."""
    if not case.jobs:
        return 0
    if storage == 1:
        return 1
    spans = [int(v.max()) - int(v.min()) for v in gc.golden_ranges(case) if v is not None]
    return (max(spans, default=0).bit_length() + 10) // 11


def run_hook(hot, case, storage, jobs=None, tile=gc.TILE):
    jobs = case.jobs if jobs is None else jobs
    cols = [[j[k] for j in jobs] for k in range(6)]
    return hot.debug_geno(case.depth, storage, *cols, tile=tile)


@pytest.mark.parametrize("name,storage", [(n, s) for n, c in CASES.items() for s in c.storages])
def test_hook(hot, restated, name, storage):
    got = run_hook(hot, CASES[name], storage)
    assert len(got) == len(CASES[name].jobs)
    for k, (row, want) in enumerate(zip(got, restated[name])):
        assert gc.record_of(row) == want, (name, storage, k, CASES[name].jobs[k])
        assert row["chrom_median"] == 0.0
    st = hot.geno_stats()
    assert st["jobs"] == 2 * len(got) and st["tiles"] == len(gc.tiles_of(CASES[name].jobs, gc.TILE))
    assert st["passes"] == expected_passes(CASES[name], storage)


@pytest.mark.parametrize("storage", [1, 4])
def test_default_tile_and_odd_tiles(hot, restated, storage):
    for name, tile in (("whole_array", 0), ("whole_array", 1000), ("tile_seams", 7), ("overlapping_and_duplicate", 4096)):
        got = run_hook(hot, CASES[name], storage, tile=tile)
        assert [gc.record_of(r) for r in got] == restated[name], (name, tile)


@pytest.mark.parametrize("name,storage", [("batch_3000", 1), ("batch_3000", 4), ("batch_wide_3000", 4)])
def test_lists_grow_and_shrink_on_one_context(hot, restated, name, storage):
    """3000 jobs, then 2, then 3000 again: no count of the longer list is left in the shorter one's histograms, and every record
    is what the same job gives when it runs alone."""
    case, want = CASES[name], restated[name]
    for jobs, expect in ((case.jobs, want), (case.jobs[5:7], want[5:7]), (case.jobs, want), ([], [])):
        got = run_hook(hot, case, storage, jobs)
        assert [gc.record_of(r) for r in got] == expect
    for k in (0, 1, 1500, 2999):
        assert gc.record_of(run_hook(hot, case, storage, case.jobs[k:k + 1])[0]) == want[k]


def test_launch_count_does_not_depend_on_the_list(hot):
    counts = {}
    for name, storage in (("one_job", 1), ("batch_3000", 1), ("one_job", 4), ("batch_3000", 4), ("span_0_and_2p30", 4), ("batch_wide_3000", 4)):
        run_hook(hot, CASES[name], storage)
        st = hot.geno_stats()
        counts[(name, storage)] = (st["launches"], st["passes"])
        assert st["ms"] > 0 and st["bytes"] > 0
    assert counts[("one_job", 1)] == counts[("batch_3000", 1)] == (2, 1)
    assert counts[("one_job", 4)] == counts[("batch_3000", 4)] == (5, 1)
    assert counts[("span_0_and_2p30", 4)] == counts[("batch_wide_3000", 4)] == (9, 3)
    run_hook(hot, CASES["no_jobs"], 1)
    assert hot.geno_stats()["launches"] == 0 and hot.geno_stats()["jobs"] == 0


def test_bad_ranges_are_refused(hot):
    from rsicnv_amd import api
    d = CASES["one_job"].depth
    for job in ((10, 5, 0, 0, 5, 5), (0, d.size + 1, 0, 0, 0, 0), (0, 5, -1, 0, 5, 9), (0, 5, 0, 0, 5, d.size + 1)):
        with pytest.raises(api.RsiError) as e:
            hot.debug_geno(d, 1, *[[v] for v in job], tile=gc.TILE)
        assert api.STATUS_NAMES[e.value.code] == "RSI_ERR_BAD_ARG"
    with pytest.raises(api.RsiError) as e:                    # the hook has overwritten whatever run the context held
        hot.geno_calls(M, [1], [100])
    assert api.STATUS_NAMES[e.value.code] == "RSI_ERR_BAD_ARG" and "compacted depth" in str(e.value)


# ---------------------------------------------------------------------------------------------------------------------
# a run's own depth
# ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def chrom(hotlib):
    """About 2 Mb, two N runs inside, a planted deletion (0.5x) and a planted duplication (1.5x)."""
    from rsicnv_amd import synth
    plan = synth.make_plan(n=2_000_003, seed=0x6E01, model=0, n_events=2, gaps=2, min_len=20000, max_len=60000, end_n=0, gap_len=30000)
    assert len(plan["nruns"]) == 2 and [e[2] for e in plan["events"]] == [synth.CN_HALF, synth.CN_1P5]
    fasta, depth = synth.generate_host(hotlib, plan)
    return plan, fasta, depth


def lines_of(plan, calls, n):
    """1-based inclusive (start, end): the run's calls, the planted events, lines straddling and inside the N runs, the ends."""
    out = [(c["start"] + 1, c["end"] + 1) for c in calls]
    out += [(a + 1, b) for a, b, _ in plan["events"]]
    for a, b in plan["nruns"]:
        out += [(a - 500, b + 700), (a + 10, b - 10), (a - 300, a + 5), (b - 5, b + 300), (a + 1, b), (a, b + 1), (b + 1, b + 1)]
    a0, b1 = plan["nruns"][0][0], plan["nruns"][1][1]
    out += [(a0 - 1000, b1 + 1000), (1, 1), (n, n), (1, n), (n - 50, n + 5000), (n + 1, n + 10), (5000, 4000), (1, 60)]
    return out


def restate_lines(rd, pairs, n, lines, m):
    pr = [(int(pairs[2 * k]), int(pairs[2 * k + 1])) for k in range(len(pairs) // 2)]
    jobs = [gc.line_job(*gc.map_line(s, e, n, pr), m, rd.size) for s, e in lines]
    return jobs, [gc.record(rd, j) for j in jobs]


@pytest.mark.parametrize("cap", [4.0, -1.0])
def test_run_records_equal_the_restatement(hot, chrom, cap):
    """cap 4: the compacted depth is bytes; no cap: int32."""
    from rsicnv_amd import api
    plan, fasta, depth = chrom
    n = plan["n"]
    res = hot.run(api.make_params(m=M, cap=cap), depth, fasta)
    calls = res.calls("calls")
    lines = lines_of(plan, calls, n)
    got = hot.geno_calls(M, [s for s, _ in lines], [e for _, e in lines])
    st = hot.geno_stats()
    rd, pairs = hot.fetch("rd_concat"), res.noncode
    assert rd.size == res.stats["n_compact"] and len(pairs) >= 4
    jobs, want = restate_lines(rd, pairs, n, lines, M)
    for k, (row, w) in enumerate(zip(got, want)):
        assert gc.record_of(row) == w, (k, lines[k], jobs[k])
        assert row["chrom_median"] == res.stats["RDmedian"]
    assert st["launches"] == (2 if cap > 0 else 5) and st["jobs"] == 2 * len(lines)
    ncalls = len(calls)
    cn = [2.0 * r["body_q"][1] / r["chrom_median"] for r in got]
    assert cn[ncalls] < 2.0 < cn[ncalls + 1]                                   # the planted deletion below P, the duplication above
    assert got[ncalls + 2 + 1]["n_body"] == 0 and got[ncalls + 2 + 7 + 1]["n_body"] == 0    # lines wholly inside the N runs
    assert 0 < got[ncalls + 2]["n_body"] < 1201                                # 500 + 700 bases around an N run, less its padding
    assert got[-3]["n_body"] == 0 and got[-2]["n_body"] == 1001 and got[-5]["n_body"] == rd.size > 0


# ---------------------------------------------------------------------------------------------------------------------
# the command line
# ---------------------------------------------------------------------------------------------------------------------

def cli(tmp, args, expect=0):
    r = subprocess.run([EXE, "geno", *args], cwd=str(tmp), capture_output=True, text=True, timeout=300)
    assert r.returncode == expect, r.stderr[-2500:]
    return r


def list_text(lines, chrom, extra=()):
    kinds = ("DEL", "DUP", "gain", "loss", "other")
    return "\n".join([f"{chrom}\t{s}\t{e}\t{kinds[k % 5]}\tx{k}" for k, (s, e) in enumerate(lines)] + list(extra)) + "\n"


def test_cli_one_chromosome(hot, hotlib, chrom, tmp_path):
    """-d RDFILE -c RNAME: every line's field is the restatement's on the arrays of the same run through the library."""
    from rsicnv_amd import api, synth
    plan, fasta, depth = chrom
    n = plan["n"]
    fa, rd_path = synth.write_case_files(hotlib, fasta, depth, str(tmp_path))
    text_depth = depth.copy()
    text_depth[n - 1] = 0                                                       # the text reader never sets the last base
    res = hot.run(api.make_params(m=M), text_depth, fasta)
    lines = lines_of(plan, res.calls("calls"), n)
    _, want = restate_lines(hot.fetch("rd_concat"), res.noncode, n, lines, M)
    cnv = tmp_path / "list.txt"
    cnv.write_text("#a comment\n" + list_text(lines, "chrS", extra=["chrZ\t100\t200\tDEL", "chrS\t10"]))
    out = str(tmp_path / "geno.txt")
    cli(tmp_path, ["-d", rd_path, "-c", "chrS", "-f", fa, "-v", str(cnv), "-o", out, "-m", str(M)])
    rows, log = open(out).read().splitlines(), open(out + ".log").read()
    src = [ln for ln in cnv.read_text().splitlines() if not ln.startswith("#") and len(ln.split()) >= 4]
    assert len(rows) == len(src) == len(lines) + 1
    for k, (row, w) in enumerate(zip(rows, want)):
        assert row == src[k] + "\t" + gc.field(w, res.stats["RDmedian"]), (k, lines[k])
    assert rows[-1] == src[-1] and "#geno: chrZ is not in the input: line written unchanged" in log
    assert log.count("#geno: chrS: ") == 1 and f"{len(lines)} lines, {2 * len(lines)} jobs" in log and "launches" in log
    assert any("CN=NA;RATIO=NA;MED=NA" in r for r in rows) and any("FLANK=" in r and "FLANK=NA" not in r for r in rows)
    assert not os.path.exists(str(tmp_path / "cnv_plots")) and "START\tEND\tTYPE\tSCORE" not in open(out).read()
    # -ploidy
    out1 = str(tmp_path / "geno1.txt")
    cli(tmp_path, ["-d", rd_path, "-c", "chrS", "-f", fa, "-v", str(cnv), "-o", out1, "-m", str(M), "-ploidy", "1"])
    assert open(out1).read().splitlines()[0] == src[0] + "\t" + gc.field(want[0], res.stats["RDmedian"], 1.0)
    # -gpus above 1: refused before any output
    no = str(tmp_path / "no.txt")
    r = cli(tmp_path, ["-d", rd_path, "-c", "chrS", "-f", fa, "-v", str(cnv), "-o", no, "-gpus", "2"], expect=1)
    assert "-gpus" in r.stderr and not os.path.exists(no) and not os.path.exists(no + ".log")
    u = subprocess.run([EXE], capture_output=True, text=True, timeout=60)
    assert "rsicnv geno" in u.stderr
    p = subprocess.run([EXE, "plot", "-d", rd_path, "-v", str(cnv)], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and "not part of the accelerated read-depth path" in p.stderr


def test_cli_cohort(hotlib, tmp_path):
    """Two chromosomes, three depth columns, -samples all: OUT.k is the single-sample run of column k, OUT.matrix their CN columns;
    the same file bgzipped gives the same files."""
    from conftest import make_case
    specs = [("chrA", 200_003, 0x6E10), ("chrB", 150_001, 0x6E20)]
    seqs, cols, lines = [], [], []
    for name, n, seed in specs:
        ds = []
        for s in range(3):
            plan, fa, d = make_case(hotlib, dict(n=n, seed=seed + s, model=0, mean=30.0 + 6 * s, n_events=3, gaps=1, max_len=20000, end_n=3000, gap_len=6000))
            ds.append(d)
            if s == 0:
                seqs.append((name, fa))
                lines += [(name, a + 1, b) for a, b, _ in plan["events"]] + [(name, plan["nruns"][1][0] - 200, plan["nruns"][1][1] + 300), (name, 1, n)]
        cols.append((name, n, np.stack(ds)))
    fa_path = str(tmp_path / "ref.fa")
    write_fasta(fa_path, seqs)
    cohort = "#CHROM\tPOS\tS1\tS2\tS3\n" + "".join("".join(f"{name}\t{p + 1}\t{d[0, p]}\t{d[1, p]}\t{d[2, p]}\n" for p in range(n)) for name, n, d in cols)
    (tmp_path / "cohort.depth").write_text(cohort)
    cnv = tmp_path / "list.txt"
    cnv.write_text("".join(f"{c}\t{s}\t{e}\tDEL\n" for c, s, e in lines[:4]) + "chrQ\t5\t900\tDUP\n" + "".join(f"{c}\t{s}\t{e}\tDUP\n" for c, s, e in lines[4:]))
    out = str(tmp_path / "co.txt")
    cli(tmp_path, ["-d", str(tmp_path / "cohort.depth"), "-f", fa_path, "-v", str(cnv), "-o", out, "-samples", "all"])
    per_sample = []
    for k in (1, 2, 3):
        single = tmp_path / f"single{k}.depth"
        single.write_text("".join("".join(f"{name}\t{p + 1}\t{d[k - 1, p]}\n" for p in range(n)) for name, n, d in cols))
        so = str(tmp_path / f"single{k}.txt")
        cli(tmp_path, ["-d", str(single), "-f", fa_path, "-v", str(cnv), "-o", so])
        rows = open(so).read().splitlines()
        assert open(f"{out}.{k}").read().splitlines() == rows and len(rows) == len(lines) + 1
        assert sum("CN=" in r for r in rows) == len(lines) and rows[4] == "chrQ\t5\t900\tDUP"
        assert "#geno: chrQ is not in the input" in open(f"{out}.{k}.log").read() and open(f"{out}.{k}.log").read().count("#geno: chr") == 3
        per_sample.append([r.split("\t")[-1].split(";")[0][3:] if "CN=" in r else "NA" for r in rows])
    matrix = open(out + ".matrix").read().splitlines()
    src = cnv.read_text().splitlines()
    assert matrix[0] == "#RNAME\tSTART\tEND\tTYPE\t1\t2\t3"
    assert matrix[1:] == ["\t".join(s.split("\t")[:4] + [per_sample[j][i] for j in range(3)]) for i, s in enumerate(src)]
    assert len({tuple(c) for c in per_sample}) == 3                              # the samples differ
    (tmp_path / "cohort.depth.gz").write_bytes(bz.bgzf(cohort.encode()))
    outz = str(tmp_path / "coz.txt")
    cli(tmp_path, ["-d", str(tmp_path / "cohort.depth.gz"), "-f", fa_path, "-v", str(cnv), "-o", outz, "-samples", "all"])
    for suffix in (".1", ".2", ".3", ".matrix"):
        assert open(outz + suffix).read() == open(out + suffix).read()
    assert "BGZF" in open(outz + ".log").read()


def test_cli_bam_equals_its_depth_dump(hotlib, tmp_path):
    """-b BAM: OUT equals the -d run of the depth its own -s dump holds."""
    from conftest import make_case
    n = 150_001
    plan, fasta, depth = make_case(hotlib, dict(n=n, seed=0x6E30, model=0, mean=20.0, n_events=3, gaps=1, max_len=12000, end_n=3000, gap_len=5000))
    fa_path = str(tmp_path / "ref.fa")
    write_fasta(fa_path, [("chrS", fasta), ("chrT", fasta[:9000])])
    bam = str(tmp_path / "small.bam")
    bu.write_bam(bam, [("chrS", n), ("chrT", 9000)], bu.paired_reads_following_depth(depth, n))
    lines = [(a + 1, b) for a, b, _ in plan["events"]] + [(plan["nruns"][1][0] - 100, plan["nruns"][1][1] + 100), (1, n), (70_000, 70_000)]
    cnv = tmp_path / "list.txt"
    cnv.write_text(list_text(lines, "chrS", extra=["chrT\t100\t2000\tDEL"]))
    out_b, out_d = str(tmp_path / "b.txt"), str(tmp_path / "d.txt")
    cli(tmp_path, ["-b", bam, "-f", fa_path, "-v", str(cnv), "-o", out_b, "-s"])
    dump = out_b + ".chrS_rd"
    assert os.path.exists(dump)
    cli(tmp_path, ["-d", dump, "-c", "chrS", "-f", fa_path, "-v", str(cnv), "-o", out_d])
    rows_b, rows_d = open(out_b).read().splitlines(), open(out_d).read().splitlines()
    assert rows_b == rows_d and sum("CN=" in r for r in rows_b) == len(lines) and rows_b[-1] == "chrT\t100\t2000\tDEL"
    assert "#geno: chrT" in open(out_b + ".log").read() and "#geno: chrT is not in the input" in open(out_d + ".log").read()
    out_dev = str(tmp_path / "bdev.txt")
    cli(tmp_path, ["-b", bam, "-c", "chrS", "-f", fa_path, "-v", str(cnv), "-o", out_dev, "-bamread", "device"])
    assert open(out_dev).read().splitlines() == rows_b


def test_unarmed(hotlib, chrom):
    """A plain run allocates and launches nothing for geno, and a context without a run refuses the call."""
    from rsicnv_amd import api
    plan, fasta, depth = chrom
    h = api.RsiHot(0)
    try:
        with pytest.raises(api.RsiError) as e:
            h.geno_calls(M, [1], [100])
        assert api.STATUS_NAMES[e.value.code] == "RSI_ERR_BAD_ARG"
        h.run(api.make_params(m=M), depth[:400_000], fasta[:400_000])
        st = h.geno_stats()
        assert st["launches"] == 0 and st["bytes"] == 0 and st["jobs"] == 0 and st["tiles"] == 0
        assert len(h.geno_calls(M, [], [])) == 0 and h.geno_stats()["bytes"] == 0
        assert h.geno_calls(M, [1000], [2000])[0]["n_body"] > 0 and h.geno_stats()["bytes"] > 0
    finally:
        h.close()


def test_abi(hotlib):
    import ctypes as C
    import re
    from rsicnv_amd import api
    hdr = open(os.path.join(ROOT, "include", "rsi_hot.h")).read()
    for sym in ("rsi_hot_geno_calls", "rsi_hot_last_geno_stats", "rsi_hot_debug_geno"):
        assert re.search(r"\b" + sym + r"\(", hdr) and sym in api.EXPORTS and hasattr(hotlib, sym)
    body = re.search(r"typedef struct rsi_geno_record \{(.*?)\} rsi_geno_record;", hdr, re.S).group(1)
    names = [re.sub(r"\[\d+\]", "", nm.strip()) for _, group in re.findall(r"(int32_t|int64_t|double)\s+([^;]+);", body) for nm in group.split(",")]
    assert names == list(api.GENO_RECORD.names) and api.GENO_RECORD.itemsize == 4 * 4 + 2 * 8 + 7 * 8
    assert C.sizeof(api.RsiGenoStats) == 5 * 8 + 8
