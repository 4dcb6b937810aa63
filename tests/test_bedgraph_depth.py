"""bedGraph depth files: "RNAME start end d" (mosdepth per-base.bed.gz, bedtools genomecov -bg / -bga), read by
rsi_genome_bedgraph_open and `rsicnv rsi -d FILE.bed[.gz]`.  The rule that defines correctness: a line stands for the lines
"RNAME p d", p = start + 1 .. end (start, end, d read as `iss >> start >> end >> d`; none when start or end fails or
end <= start; d = 0 when it fails), "track" / "browser" lines stand for none, and every chromosome's depth, counts and
hand-over order are what today's genome reader gives on that expanded file."""
import gzip
import os
import shutil
import subprocess

import numpy as np
import pytest

import bgzf_util as bz
from conftest import make_case
from text_rules import expand_line
from test_genome_text import EXE, write_fasta

STATS = ("lines", "stored", "beyond", "fallback")


# ---------------------------------------------------------------------------------------------------------------------
# the rule, restated: the expanded per-base file
# ---------------------------------------------------------------------------------------------------------------------

def expand(text):
    out = []
    for line in text.split("\n"):
        out += expand_line(line)
    return "\n".join(out) + "\n"


def runs_of(depth, lo, hi):
    """(start, end, d) runs of equal depth over depth[lo:hi]."""
    if hi <= lo:
        return []
    seg = depth[lo:hi]
    cut = np.flatnonzero(np.diff(seg)) + 1
    starts = np.concatenate(([0], cut))
    ends = np.concatenate((cut, [seg.size]))
    return [(lo + int(a), lo + int(b), int(seg[a])) for a, b in zip(starts, ends)]


def run_depth(n, seed):
    """Piecewise-constant depth with runs of 1 base to 50 kb, a fifth of them zero, and a stretch of per-base depth (runs of
    about one base, as samtools-like depth gives) over a fifth of the chromosome, at most 200 kb."""
    rng = np.random.default_rng(seed)
    d = np.zeros(n, dtype=np.int32)
    i = 0
    while i < n:
        u = rng.random()
        ln = int(rng.integers(1, 11)) if u < 0.6 else (int(rng.integers(10, 1001)) if u < 0.9 else int(rng.integers(1000, 50_001)))
        d[i:i + ln] = 0 if rng.random() < 0.2 else int(rng.integers(1, 200))
        i += ln
    k = min(200_000, n // 5)
    d[n // 3:n // 3 + k] = rng.integers(0, 60, k)
    return d


def quirk_lines(name, depth, seed, bga=True):
    """Text lines of one chromosome's runs with every quirk: mixed blanks, CRLF, a negative start, an interval across n and
    one beyond it, end <= start (also under another name), a missing and a non-numeric depth.  bga=False leaves out the
    zero runs (bedtools genomecov -bg)."""
    rng = np.random.default_rng(seed)
    n = depth.size
    seps = ["\t", " ", " \t", "  "]
    runs = runs_of(depth, 0, n)
    out = []
    zk = 0
    for k, (a, b, d) in enumerate(runs):
        zk += d == 0
        if not bga and d == 0:
            continue
        if k == 0:
            a = -7                                               # positions -6 .. 0 skipped, 1 .. b kept
        sep = seps[int(rng.integers(0, 4))]
        lead = " " if k % 23 == 5 else ""
        cr = "\r" if k % 7 == 3 else ""
        if d == 0 and zk % 50 == 1:
            out.append(f"{lead}{name}{sep}{a}{sep}{b}{cr}")      # missing depth: 0
        elif d == 0 and zk % 50 == 2:
            out.append(f"{name}\t{a}\t{b}\tabc{cr}")             # non-numeric depth: 0
        else:
            out.append(f"{lead}{name}{sep}{a}{sep}{b}{sep}{d}{cr}")
        if k == len(runs) // 3:
            out.append(f"{name}\t{b}\t{b}\t9")                   # end == start: no line
            out.append(f"{name}\t{b + 5}\t{b}\t9")               # end < start: no line
            out.append(f"chrZ_none\t{b}\t{b}\t4")                # nothing under another name: not a chromosome change
    last = runs[-1][1]
    out.append(f"{name}\t{last}\t{last + 40}\t61")                # across n (the runs end at n - 11) ...
    out.append(f"{name}\t{last + 100}\t{last + 300}\t62\r")       # ... and wholly beyond n
    return out


def genome_of(path, names, lens, **kw):
    """{name: (depth or None, stats)} in hand-over order."""
    from rsicnv_amd import api
    out = {}
    with api.GenomeText(str(path), names, lens, **kw) as g:
        for name, ptr, n, st in g:
            out[name] = (None if ptr is None else g.depth(st["slot"]), st)
    return out


def check_equal(got, ref, tag=""):
    assert list(got) == list(ref), (tag, list(got), list(ref))
    for name, (d, st) in ref.items():
        gd, gst = got[name]
        assert gst["slot"] >= 0 if d is not None else gst["slot"] < 0, (tag, name)
        if d is not None:
            assert np.array_equal(gd, d), (tag, name, int(np.sum(gd != d)))
        for s in STATS:
            assert gst[s] == st[s], (tag, name, s, gst[s], st[s])


def bed_case(unsorted_chrom=None):
    """Three chromosomes (-bga, -bg and -bga), an unknown and an MT contig, header and comment lines."""
    specs = [("chrA", 1_000_003, 0xB01, True), ("chrB", 250_001, 0xB02, False), ("chrC", 100_019, 0xB03, True)]
    lines = ["track type=bedGraph name=cov", "browser position chrA:1-1000", "# mosdepth"]
    names, lens = [], []
    for i, (name, n, seed, bga) in enumerate(specs):
        d = run_depth(n - 11, seed)                         # runs over [0, n - 11); quirk_lines adds the lines across n
        body = quirk_lines(name, d, seed, bga)
        if name == unsorted_chrom:                          # overlapping and out-of-order intervals
            body.insert(len(body) // 2, f"{name}\t1000\t9000\t33")
            body.insert(len(body) // 4, f"{name}\t200000\t200300\t44")
            body.append(f"{name}\t10\t20\t55")
        lines += body
        names.append(name); lens.append(n)
        lines += ["", "track name=next"]
        if i == 0:
            lines += [f"chrUn_x\t{p}\t{p + 50}\t7" for p in range(0, 5000, 50)]
            lines += [f"chrMT\t{p}\t{p + 10}\t9" for p in range(0, 1000, 10)]
    return "\r\n".join(lines[:2]) + "\n" + "\n".join(lines[2:]) + "\n", names, lens


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the restatement, the writer, refusals and the ABI
# ---------------------------------------------------------------------------------------------------------------------

def test_expansion_rule():
    assert expand_line("c\t0\t3\t7") == ["c\t1\t7", "c\t2\t7", "c\t3\t7"]
    assert expand_line("c -2 1 4\r") == ["c\t-1\t4", "c\t0\t4", "c\t1\t4"]
    assert expand_line("c\t5\t5\t1") == [] and expand_line("c\t6\t5\t1") == [] and expand_line("c x 5 1") == []
    assert expand_line("c\t1\t2") == ["c\t2\t0"] and expand_line("c\t1\t2\tabc") == ["c\t2\t0"]
    assert expand_line("track\t1\t2\t3") == [] and expand_line("browser 0 1 1") == [] and expand_line("#c\t0\t1\t1") == []


def test_synth_bedgraph_writer(tmp_path):
    from rsicnv_amd import api
    lib = api.load_library()
    d = np.array([0, 0, 3, 3, 3, 0, 5], dtype=np.int32)
    p = tmp_path / "s.bed"
    assert lib.rsi_synth_append_genome_bedgraph(str(p).encode(), b"chrZ", d.ctypes.data, d.size, 0) == 0
    assert p.read_text() == "chrZ\t0\t2\t0\nchrZ\t2\t5\t3\nchrZ\t5\t6\t0\nchrZ\t6\t7\t5\n"
    pz = tmp_path / "s.bed.gz"
    assert lib.rsi_synth_append_genome_bedgraph(str(pz).encode(), b"chrZ", d.ctypes.data, d.size, 1) == 0
    assert gzip.decompress(pz.read_bytes()).decode() == p.read_text()
    assert expand(p.read_text()) == "".join(f"chrZ\t{i + 1}\t{v}\n" for i, v in enumerate(d))


def test_bedgraph_reader_in_the_abi(hotlib):
    from rsicnv_amd import api
    for sym in ("rsi_genome_bedgraph_open", "rsi_synth_append_genome_bedgraph"):
        assert sym in api.EXPORTS and hasattr(hotlib, sym)
    hdr = open(os.path.join(os.path.dirname(EXE), "..", "..", "include", "rsi_hot.h")).read()
    assert "rsi_genome_text* rsi_genome_bedgraph_open(int device, const char* path, int nref" in hdr


BED3 = "chr1\t0\t2\t30\nchr1\t2\t4\t31\n"


def _run_cli(tmp_path, fname, text, args):
    d = tmp_path / fname
    d.write_text(text)
    fa = tmp_path / "ref.fa"
    write_fasta(str(fa), [("chr1", np.frombuffer(b"ACGT" * 10, dtype=np.uint8)), ("chrZ", np.frombuffer(b"ACGT" * 5, dtype=np.uint8))])
    out = tmp_path / "out.txt"
    return subprocess.run([EXE, "rsi", "-f", str(fa), "-d", str(d), "-o", str(out), "-np"] + args,
                          capture_output=True, text=True, timeout=60)


def _refused(tmp_path, fname, text, args):
    r = _run_cli(tmp_path, fname, text, args)
    assert r.returncode == 1, (args, r.returncode, r.stderr)
    assert not os.path.exists(tmp_path / "out.txt"), (args, os.listdir(tmp_path))
    return r.stderr


@pytest.mark.parametrize("args,msg", [
    (["-samples", "all"], "one depth column"),
    (["-gpus", "2"], "one device"),
    (["-dformat", "bed"], "expected depth or bedgraph"),
    (["-c", "chrQ"], "chrQ not found in fai index"),
], ids=["samples", "gpus2", "bad_dformat", "c_not_in_fai"])
def test_bedgraph_refusals(tmp_path, args, msg):
    assert msg in _refused(tmp_path, "g.bed", BED3, args)


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("chrom", ["chrZ", "Z"])
def test_bedgraph_c_absent_from_the_file(tmp_path, chrom):
    """-c naming a .fai sequence the file has no lines for: found by the reader's one pass, exit 1, no output file."""
    err = _refused(tmp_path, "g.bed", BED3, ["-c", chrom])
    assert f"no lines for {chrom} in" in err, err


@pytest.mark.parametrize("fname,bed", [
    ("g.bed", True), ("g.BED.gz", True), ("g.bedgraph.bgz", True), ("g.bg", True), ("G.BedGraph", True), ("x.gz.bed.gz", True),
    ("g.depth", False), ("g.bed.txt", False), ("g.bed.gz.gz", False), ("g.bedx", False), ("bed", False),
])
def test_bedgraph_by_file_name(tmp_path, fname, bed):
    """The format by name, seen through the refusal each format gives to a column that is not there."""
    err = _refused(tmp_path, fname, BED3, ["-samples", "9"])
    assert ("one depth column" in err) == bed and ("not a depth column" in err) == (not bed), err


def test_dformat_overrides_the_name(tmp_path):
    assert "one depth column" in _refused(tmp_path, "g.cov.gz", BED3, ["-samples", "9", "-dformat", "bedgraph"])
    assert "not a depth column" in _refused(tmp_path, "g.bed", BED3, ["-samples", "9", "-dformat", "depth"])


def test_bedgraph_in_the_usage():
    u = subprocess.run([EXE], capture_output=True, text=True)
    assert "-dformat depth|bedgraph" in u.stderr
    assert ".bed, .bedgraph or .bg" in u.stderr and "START END DEPTH" in u.stderr


# ---------------------------------------------------------------------------------------------------------------------
# device: the reader against the expanded file
# ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def case_files(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("bed")
    text, names, lens = bed_case()
    (tmp / "g.bed").write_text(text)
    (tmp / "expanded.depth").write_text(expand(text))
    raw = text.encode()
    rng = np.random.default_rng(3)
    (tmp / "g.bed.gz").write_bytes(bz.gzip_members(raw, parts=3))
    (tmp / "g.bgzf.bed.gz").write_bytes(bz.bgzf(raw, sizes=iter(lambda: int(rng.integers(3000, 65281)), None)))
    return tmp, names, lens


@pytest.mark.gpu
@pytest.mark.timeout(900)
@pytest.mark.parametrize("chunk", [0, 4097, 131_101], ids=["chunk_default", "chunk_4097", "chunk_131101"])
@pytest.mark.parametrize("form", ["g.bed", "g.bed.gz", "g.bgzf.bed.gz"], ids=["text", "gzip", "bgzf"])
def test_bedgraph_equals_expanded_file(case_files, form, chunk):
    tmp, names, lens = case_files
    ref = genome_of(tmp / "expanded.depth", names, lens)
    assert list(ref) == ["chrA", "chrUn_x", "chrB", "chrC"]
    assert all(ref[nm][1]["fallback"] == 0 for nm in names)
    got = genome_of(tmp / form, names, lens, bedgraph=True, chunk_bytes=chunk, max_resident=2)
    check_equal(got, ref, (form, chunk))
    # bytes: from a chromosome's first data line to the next one's (or the end of the file) in the bedGraph text
    text = (tmp / "g.bed").read_bytes().decode()   # the CRs as they are
    first, off = {}, 0
    for line in text.split("\n"):
        lines = expand_line(line)
        if lines:
            first.setdefault(lines[0].split("\t")[0], off)
        off += len(line) + 1
    order = list(first) + [None]                       # file order, the skipped MT contig included
    ends = {nm: (first[nxt] if nxt else len(text)) for nm, nxt in zip(order, order[1:])}
    assert {nm: got[nm][1]["bytes"] for nm in got} == {nm: ends[nm] - first[nm] for nm in got}


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_bedgraph_hundreds_of_tiny_contigs(tmp_path):
    """600 contigs of 100-600 bases, more than one parse launch's segment table holds (kMaxGenomeSegs = 512): a workgroup's
    8 KB of text covers some twenty contigs and a thread's 32 bytes cross from one into the next, so the counts leave per
    thread and the default chunk takes two parse launches.  Runs of 1-40 bases, in every fifth contig one of 129-400 (the
    run list beside the inline writes), every third contig with the quirks of quirk_lines."""
    rng = np.random.default_rng(0xB1D)
    lines, names, lens = ["track type=bedGraph name=tiny"], [], []
    for i in range(600):
        n = int(rng.integers(100, 601))
        while i % 5 == 0 and n < 420:                            # room for the long run in front of quirk_lines' n - 11
            n = int(rng.integers(100, 601))
        quirks = i % 3 == 0
        d = np.zeros(n - 11 if quirks else n, dtype=np.int32)
        p = 0
        while p < d.size:
            ln = int(rng.integers(1, 41))
            d[p:p + ln] = int(rng.integers(0, 90))
            p += ln
        if i % 5 == 0:
            ln = int(rng.integers(129, 401))
            a = int(rng.integers(1, d.size - ln))
            d[a:a + ln] = 200 + i % 50                           # no neighbour has this depth: one run of ln bases
            assert (a, a + ln, 200 + i % 50) in runs_of(d, 0, d.size)
        name = f"ctg{i:04d}"
        names.append(name); lens.append(n)
        lines += quirk_lines(name, d, 0xB1D + i) if quirks else [f"{name}\t{a}\t{b}\t{v}" for a, b, v in runs_of(d, 0, d.size)]
        if i % 17 == 0:
            lines.append("")
    text = "\n".join(lines) + "\n"
    assert len(text) < 1_000_000
    (tmp_path / "tiny.bed").write_text(text)
    (tmp_path / "tiny.depth").write_text(expand(text))
    ref = genome_of(tmp_path / "tiny.depth", names, lens)
    assert list(ref) == names
    for kw in ({}, dict(chunk_bytes=4097, max_resident=2)):
        got = genome_of(tmp_path / "tiny.bed", names, lens, bedgraph=True, **kw)
        check_equal(got, ref, kw)
        assert list(got) == names and all(got[nm][1]["fallback"] == 0 for nm in names), kw


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_bedgraph_long_runs(tmp_path):
    """A 201 Mb chromosome that is one zero run but for a few long runs that start and end off 16-byte boundaries (and runs
    at the inline bound): the depth against numpy, no fallback, -bga and -bg alike."""
    n = 201_000_017
    runs = [(5_000_003, 5_000_003 + 3_333_335, 17), (50_000_001, 57_654_321, 3), (100_000_002, 100_000_002 + 129, 9),
            (100_001_000, 100_001_128, 4), (120_000_001, 120_000_001 + 2 * (1 << 20) + 3, 77), (150_000_000, 150_000_001, 6),
            (n - 2_500_001, n, 5)]
    want = np.zeros(n, dtype=np.int32)
    for a, b, d in runs:
        want[a:min(b, n - 1)] = d
    bga, bg, prev = [], [], 0
    for a, b, d in runs:
        if a > prev:
            bga.append(f"chrL\t{prev}\t{a}\t0")
        bga.append(f"chrL\t{a}\t{b}\t{d}")
        bg.append(f"chrL\t{a}\t{b}\t{d}")
        prev = b
    for tag, lines in (("bga", bga), ("bg", bg)):
        p = tmp_path / f"{tag}.bed"
        p.write_text("\n".join(lines) + "\n")
        got = genome_of(p, ["chrL"], [n], bedgraph=True)
        d, st = got["chrL"]
        assert st["fallback"] == 0, tag
        assert np.array_equal(d, want), (tag, int(np.sum(d != want)))
        pos = sum(b - a for a, b, _ in (runs if tag == "bg" else [(0, n, 0)]))
        assert st["lines"] == pos and st["beyond"] == 1 and st["stored"] == pos - 1, (tag, st)
        del d, got


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_bedgraph_unsorted_chromosome_falls_back_alone(tmp_path):
    text, names, lens = bed_case(unsorted_chrom="chrB")
    (tmp_path / "u.bed").write_text(text)
    (tmp_path / "u.depth").write_text(expand(text))
    ref = genome_of(tmp_path / "u.depth", names, lens)
    assert {nm: ref[nm][1]["fallback"] for nm in names} == {"chrA": 0, "chrB": 1, "chrC": 0}
    for chunk in (0, 4097):
        check_equal(genome_of(tmp_path / "u.bed", names, lens, bedgraph=True, chunk_bytes=chunk), ref, chunk)


def sequential(lines, n):
    """numpy restatement of the sequential loop on (start, end, d) lines of one chromosome: later lines overwrite earlier
    ones, reading stops at the first position >= n.  (depth, lines, stored, beyond)"""
    rd = np.zeros(n, dtype=np.int32)
    nl = ns = nb = 0
    for a0, b, d in lines:
        a = max(a0, 0)
        if b <= a:
            continue
        hi = min(b, n - 1)
        if hi > a:
            rd[a:hi] = d
            nl += hi - a
            ns += hi - a
        if b >= n:
            nl += 1
            nb += 1
            break
    return rd, nl, ns, nb


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_bedgraph_run_list_overflow_falls_back(tmp_path):
    """Overlapping multi-Mb intervals, ~200 lines of 4 pieces each per 4097-byte chunk: more pieces than the run list holds
    (bedgraph_run_cap: 4097 / 8 + 2 + 4 = 518).  That chromosome is rebuilt by the host loop (fallback = 1, depth and counts
    of the sequential rules); the chromosomes around it, whose long runs are listed in chunks of their own, are untouched."""
    nA, nB, nC = 100_003, 4_000_037, 100_003
    chrA = [(300 * i, 300 * i + 300, (i % 3) * 20) for i in range(200)] + [(60_000 + i, 60_001 + i, 1 + i % 50) for i in range(600)]
    chrA.append((60_600, nA, 12))
    chrC = [(i, i + 1, 1 + i % 40) for i in range(600)] + [(600 + 300 * i, 900 + 300 * i, 5 + i % 4) for i in range(200)]
    chrC.append((60_600, nC, 3))
    chrB = [(3 * i, 4_000_000 - 7 * i, i + 1) for i in range(300)] + [(3_999_000, 4_000_100, 999), (10, 20, 7)]
    def text_of(name, lines):
        return "".join(f"{name}\t{a}\t{b}\t{d}\n" for a, b, d in lines)
    bed = text_of("chrA", chrA) + text_of("chrB", chrB) + text_of("chrC", chrC)
    per_chunk = 4097 // max(len(f"chrB\t{a}\t{b}\t{d}\n") for a, b, d in chrB)
    assert per_chunk * 4 > 4097 // 8 + 2 + (nA + nB + nC) // (1 << 20)      # the list overflows at chunk_bytes=4097
    (tmp_path / "o.bed").write_text(bed)
    (tmp_path / "ac.depth").write_text(expand(text_of("chrA", chrA) + text_of("chrC", chrC)))
    names, lens = ["chrA", "chrB", "chrC"], [nA, nB, nC]
    ref = genome_of(tmp_path / "ac.depth", names, lens)
    wantB, lB, sB, bB = sequential(chrB, nB)
    for chunk in (4097, 0):
        got = genome_of(tmp_path / "o.bed", names, lens, bedgraph=True, chunk_bytes=chunk)
        assert list(got) == names, chunk
        for nm in ("chrA", "chrC"):
            assert ref[nm][1]["fallback"] == 0 and np.array_equal(got[nm][0], ref[nm][0]), (chunk, nm)
            assert all(got[nm][1][s] == ref[nm][1][s] for s in STATS), (chunk, nm, got[nm][1], ref[nm][1])
        d, st = got["chrB"]
        assert st["fallback"] == 1, chunk
        assert np.array_equal(d, wantB), (chunk, int(np.sum(d != wantB)))
        assert (st["lines"], st["stored"], st["beyond"]) == (lB, sB, bB), (chunk, st)


# ---------------------------------------------------------------------------------------------------------------------
# command line
# ---------------------------------------------------------------------------------------------------------------------

def rows_of(path):
    return [l for l in open(path).read().splitlines() if not l.startswith("#")]


@pytest.fixture(scope="module")
def cli_files(hotlib, tmp_path_factory):
    """Three chromosomes with calls and a skipped MT contig, as BGZF bedGraph (mosdepth's layout) and as RNAME POS DEPTH."""
    from rsicnv_amd import api
    import ctypes as C
    lib = api.load_library()
    lib.rsi_synth_append_genome_text.argtypes = [C.c_char_p, C.c_char_p, C.c_void_p, C.c_int64]
    tmp = str(tmp_path_factory.mktemp("bedcli"))
    specs = [("chrP", dict(n=400_007, seed=0xC21, model=1, n_events=5, gaps=1, max_len=20000, end_n=5000, gap_len=8000)),
             ("chrQ", dict(n=350_019, seed=0xC22, model=0, n_events=4, gaps=1, max_len=20000, end_n=5000, gap_len=8000)),
             ("chrR", dict(n=300_001, seed=0xC23, model=1, n_events=4, gaps=0, max_len=15000, end_n=4000))]
    bed, depth = os.path.join(tmp, "g.bed.gz"), os.path.join(tmp, "g.depth")
    seqs, slices = [], []
    for i, (name, kw) in enumerate(specs):
        _, fasta, d = make_case(hotlib, kw)
        d = np.ascontiguousarray(d, dtype=np.int32)
        d[5000:25000] = d[5000]                              # a long run as well
        seqs.append((name, fasta))
        assert lib.rsi_synth_append_genome_bedgraph(bed.encode(), name.encode(), d.ctypes.data, d.size, 1) == 0
        assert lib.rsi_synth_append_genome_text(depth.encode(), name.encode(), d.ctypes.data, d.size) == 0
        if i == 0:
            mt = np.full(500, 9, dtype=np.int32)
            assert lib.rsi_synth_append_genome_bedgraph(bed.encode(), b"chrMT", mt.ctypes.data, mt.size, 1) == 0
            assert lib.rsi_synth_append_genome_text(depth.encode(), b"chrMT", mt.ctypes.data, mt.size) == 0
        sl = os.path.join(tmp, f"slice_{name}.txt")
        with open(sl, "w") as f:
            f.write("".join(f"{p + 1}\t{v}\n" for p, v in enumerate(d.tolist())))
        slices.append((name, sl))
    fa = os.path.join(tmp, "ref.fa")
    write_fasta(fa, list(reversed(seqs)))
    return tmp, fa, bed, depth, slices


def _cli(args, timeout=600):
    return subprocess.run([EXE, "rsi"] + args, capture_output=True, text=True, timeout=timeout)


@pytest.mark.gpu
@pytest.mark.timeout(2400)
@pytest.mark.parametrize("extra", [[], ["-MED", "-m", "51"], ["-NOGC"]], ids=["nb", "med51", "nogc"])
def test_cli_bedgraph_equals_per_base_file(cli_files, extra):
    tmp, fa, bed, depth, slices = cli_files
    tag = "_".join(extra) or "nb"
    out, ref = os.path.join(tmp, f"bed_{tag}.txt"), os.path.join(tmp, f"depth_{tag}.txt")
    r = _cli(["-f", fa, "-d", bed, "-o", out, "-np"] + extra)
    assert r.returncode == 0, r.stderr[-3000:]
    r = _cli(["-f", fa, "-d", depth, "-o", ref, "-np"] + extra)
    assert r.returncode == 0, r.stderr[-3000:]
    mine = rows_of(out)
    assert mine == rows_of(ref) and len(mine) >= 3
    assert open(out).read().startswith(f"#input {bed}\n")
    assert "#depth file: bedGraph" in open(out + ".log").read()
    if extra:
        return
    # -c: one chromosome's rows alone
    oc = os.path.join(tmp, "bed_chrQ.txt")
    r = _cli(["-f", fa, "-d", bed, "-o", oc, "-np", "-c", "chrQ"])
    assert r.returncode == 0, r.stderr[-3000:]
    q = rows_of(oc)
    assert q and q == [l for l in mine if l.split("\t")[0] == "chrQ"]
    assert [l.split()[1] for l in open(oc + ".log") if l.startswith("#processing ")] == ["chrQ"]
    # a name the suffix rule does not know, with -dformat bedgraph
    cov = os.path.join(tmp, "sample.cov.gz")
    shutil.copyfile(bed, cov)
    oz = os.path.join(tmp, "cov.txt")
    r = _cli(["-f", fa, "-d", cov, "-o", oz, "-np", "-dformat", "bedgraph"])
    assert r.returncode == 0, r.stderr[-3000:]
    assert rows_of(oz) == mine


@pytest.mark.gpu
@pytest.mark.timeout(2400)
@pytest.mark.parametrize("extra", [[], ["-MED", "-m", "51"], ["-NOGC"]], ids=["nb", "med51", "nogc"])
def test_cli_bedgraph_equals_reference_per_chromosome(cli_files, extra):
    """The rows of the bedGraph run against the compiled reference on each chromosome's two-column slice."""
    import oracle
    if not os.path.exists(oracle.REF_BIN):
        pytest.skip(f"the compiled reference is not built ({oracle.REF_BIN}): build() makes it where the reference sources are")
    tmp, fa, bed, depth, slices = cli_files
    tag = "_".join(extra) or "nb"
    out = os.path.join(tmp, f"bed_ref_{tag}.txt")
    r = _cli(["-f", fa, "-d", bed, "-o", out, "-np"] + extra)
    assert r.returncode == 0, r.stderr[-3000:]
    theirs = []
    for name, sl in slices:
        o2 = os.path.join(tmp, f"ref_{tag}_{name}.txt")
        subprocess.run([oracle.REF_BIN, "rsi", "-f", fa, "-d", sl, "-c", name, "-o", o2, "-np"] + extra, check=True,
                       capture_output=True, timeout=900, cwd=tmp)
        theirs += rows_of(o2)
    assert rows_of(out) == theirs and len(theirs) >= 3
