"""Whole-genome depth text: "RNAME pos depth" lines, every chromosome in one file (rsi_genome_text_*, `rsicnv rsi -d FILE`
without -c).  The rule that defines correctness: for every chromosome X, what the genome reader (and the command line) gives
equals what today's single-chromosome path gives on X's slice -- the lines whose name token is X, with the name and the
blanks after it removed."""
import os
import subprocess

import numpy as np
import pytest

from conftest import make_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "rsicnv_amd", "bin", "rsicnv")


# ---------------------------------------------------------------------------------------------------------------------
# file builders: every data line is kept as (name, rest, pos, depth) -- rest is the slice line, pos / depth what the
# reference's `iss >> pos >> d` reads from it
# ---------------------------------------------------------------------------------------------------------------------

def chrom_lines(name, depth, n, seed, quirks=True, unsorted=False):
    """Data lines of one chromosome in mixed formatting, running past the end (pos == n and pos > n)."""
    rng = np.random.default_rng(seed)
    out = []
    seps = ["\t", " ", "  ", "\t "]
    for pos in range(1, n + 3):
        if pos % 1009 == 0:
            continue                                        # missing position: stays 0
        d = int(depth[pos - 1]) if pos <= n else 55
        k = pos % 4
        rest = f"{pos}{seps[k]}{d}" + ("\r" if quirks and pos % 7 == 0 else "")
        out.append((name, rest, pos, d))
    if quirks:
        mid = len(out) // 2
        out.insert(mid, (name, "0\t99", 0, 99))            # pos < 1: skipped
        out.insert(mid + 1, (name, "-4 12", -4, 12))
        p = out[mid + 2][2]                                 # a line without a depth field: stores 0 at a position of its own
        out[mid + 2] = (name, f"{p}", p, 0)
    if unsorted:                                            # a repeated position: the order-dependent rules are in play
        q = len(out) // 3
        out.insert(q + 1, out[q - 5])
    return out


def render(lines, seed):
    """The genome file's text.  lines: data tuples and plain strings (comments, empty lines)."""
    rng = np.random.default_rng(seed)
    text = []
    for i, ln in enumerate(lines):
        if isinstance(ln, str):
            text.append(ln)
            continue
        name, rest = ln[0], ln[1]
        lead = " " if i % 11 == 0 else ("\t" if i % 13 == 0 else "")
        sep = "\t" if i % 3 else (" " if i % 2 else " \t")
        text.append(f"{lead}{name}{sep}{rest}")
    return "\n".join(text) + "\n"


def slice_text(lines, name):
    return "\n".join(ln[1] for ln in lines if not isinstance(ln, str) and ln[0] == name) + "\n"


def restate(lines, name, n):
    """numpy restatement of load_data_from_text's loop on the slice (loaddata.cpp:496-517)."""
    rd = np.zeros(n, dtype=np.int32)
    for ln in lines:
        if isinstance(ln, str) or ln[0] != name or ln[2] < 1:
            continue
        if ln[2] >= n:
            break
        rd[ln[2] - 1] = ln[3]
    return rd


def write_fasta(path, seqs):
    """seqs: [(name, uint8 array)] -> FASTA with 60-column lines and its .fai."""
    fai = []
    with open(path, "wb") as f:
        off = 0
        for name, seq in seqs:
            head = f">{name}\n".encode()
            f.write(head)
            off += len(head)
            body = b"".join(seq[i:i + 60].tobytes() + b"\n" for i in range(0, len(seq), 60))
            f.write(body)
            fai.append(f"{name}\t{len(seq)}\t{off}\t60\t61")
            off += len(body)
    with open(path + ".fai", "w") as f:
        f.write("\n".join(fai) + "\n")


def genome_case(hotlib, unsorted_chrom=None):
    """Six chromosomes (odd lengths, N regions) in one file, plus a contig missing from the .fai, an MT and a dotted
    contig (both skipped) and a .fai entry with no lines; comments and empty lines in between."""
    specs = [("chrA", dict(n=300_007, seed=0x6E01, model=0, n_events=3, gaps=1, max_len=15000, end_n=4000, gap_len=6000)),
             ("5", dict(n=412_331, seed=0x6E02, model=1, n_events=4, gaps=1, max_len=20000, end_n=5000, gap_len=7000)),
             ("chrC", dict(n=1_200_013, seed=0x6E03, model=1, n_events=5, gaps=2, max_len=30000, end_n=6000, gap_len=9000)),
             ("chrD", dict(n=333_333, seed=0x6E04, model=0, n_events=3, gaps=0, max_len=15000, end_n=0)),
             ("chrE", dict(n=654_321, seed=0x6E05, model=1, n_events=4, gaps=1, max_len=20000, end_n=5000, gap_len=8000)),
             ("chrF", dict(n=500_001, seed=0x6E06, model=0, n_events=4, gaps=1, max_len=20000, end_n=5000, gap_len=8000))]
    cases = {}
    for name, kw in specs:
        _, fasta, depth = make_case(hotlib, kw)
        cases[name] = (fasta, depth)
    rng = np.random.default_rng(3)
    lines = ["#RNAME\tPOS\tDEPTH", ""]
    order = []
    for i, (name, _) in enumerate(specs):
        fasta, depth = cases[name]
        lines += chrom_lines(name, depth, fasta.size, 100 + i, unsorted=(name == unsorted_chrom))
        order.append(name)
        lines += ["# between chromosomes", ""]
        if i == 1:
            lines += [("chrUn_missing", f"{p}\t7", p, 7) for p in range(1, 2000)]
            lines += [("chrMT", f"{p}\t9", p, 9) for p in range(1, 1500)]
        if i == 3:
            lines += [("GL000220.1", f"{p}\t3", p, 3) for p in range(1, 800)]
    fai_seqs = [("chrA", cases["chrA"][0]), ("chr5", cases["5"][0]), ("chrNoLines", cases["chrD"][0][:50_000])]
    fai_seqs += [(nm, cases[nm][0]) for nm in ("chrC", "chrD", "chrE", "chrF")]
    return cases, lines, order, fai_seqs


def fai_of(fai_seqs):
    return [nm for nm, _ in fai_seqs], [int(s.size) for _, s in fai_seqs]


def read_all(g):
    out = []
    for name, ptr, n, st in g:
        out.append((name, None if ptr is None else g.depth(st["slot"]), n, st))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# device: the reader against the slices
# ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def hot():
    from rsicnv_amd import api
    h = api.RsiHot(0)
    yield h
    h.close()


@pytest.mark.gpu
def test_genome_depth_equals_slices(hotlib, hot, tmp_path):
    from rsicnv_amd import api
    cases, lines, order, fai_seqs = genome_case(hotlib)
    path = tmp_path / "genome.depth"
    path.write_text(render(lines, 1))
    names, lens = fai_of(fai_seqs)
    with api.GenomeText(str(path), names, lens) as g:
        got = read_all(g)
    assert [x[0] for x in got] == ["chrA", "5", "chrUn_missing", "chrC", "chrD", "chrE", "chrF"]
    for name, depth, n, st in got:
        if name == "chrUn_missing":
            assert depth is None and st["slot"] == -1
            continue
        assert n == cases[name][0].size
        sl = tmp_path / f"slice_{name}.txt"
        sl.write_text(slice_text(lines, name))
        ref_st = hot.load_depth_text(str(sl), n)
        ref = hot.fetch("depth_in")
        assert np.array_equal(depth, ref), (name, int(np.sum(depth != ref)))
        assert np.array_equal(depth, restate(lines, name, n)), name
        assert depth[n - 1] == 0                             # the last base is never set (App. A Q7)
        for k in ("lines", "stored", "beyond", "fallback"):
            assert st[k] == ref_st[k], (name, k, st[k], ref_st[k])
        assert st["fallback"] == 0 and st["beyond"] == 3 and st["stored"] > 0.99 * n - 2000


@pytest.mark.gpu
def test_unsorted_chromosome_alone_falls_back(hotlib, hot, tmp_path):
    from rsicnv_amd import api
    cases, lines, order, fai_seqs = genome_case(hotlib, unsorted_chrom="chrC")
    path = tmp_path / "genome.depth"
    path.write_text(render(lines, 2))
    names, lens = fai_of(fai_seqs)
    with api.GenomeText(str(path), names, lens) as g:
        got = read_all(g)
    for name, depth, n, st in got:
        if depth is None:
            continue
        assert st["fallback"] == (1 if name == "chrC" else 0), (name, st)
        sl = tmp_path / f"slice_{name}.txt"
        sl.write_text(slice_text(lines, name))
        ref_st = hot.load_depth_text(str(sl), n)
        assert ref_st["fallback"] == st["fallback"]
        assert np.array_equal(depth, hot.fetch("depth_in")), name
        assert np.array_equal(depth, restate(lines, name, n)), name
        for k in ("lines", "stored", "beyond"):
            assert st[k] == ref_st[k], (name, k)


@pytest.mark.gpu
def test_chunk_geometry_does_not_change_the_depth(hotlib, tmp_path):
    """Chunks of 4 KiB (odd), 1 MiB and the default: boundaries fall before, inside and at name changes."""
    from rsicnv_amd import api
    cases, lines, order, fai_seqs = genome_case(hotlib)
    path = tmp_path / "genome.depth"
    text = render(lines, 3)
    path.write_text(text)
    names, lens = fai_of(fai_seqs)
    runs = {}
    for chunk in (4097, (1 << 20) + 3, 0):
        with api.GenomeText(str(path), names, lens, chunk_bytes=chunk) as g:
            runs[chunk] = read_all(g)
    base = runs[0]
    for chunk, got in runs.items():
        assert [x[0] for x in got] == [x[0] for x in base], chunk
        for (name, d, n, st), (_, d0, _, st0) in zip(got, base):
            if d0 is None:
                assert d is None
                continue
            assert np.array_equal(d, d0), (chunk, name)
            assert (st["lines"], st["stored"], st["beyond"], st["fallback"]) == (st0["lines"], st0["stored"], st0["beyond"], st0["fallback"])
    # a chunk boundary exactly at a name change: the chunk ends right behind chrA's last line
    cut = text.index("# between chromosomes")
    with api.GenomeText(str(path), names, lens, chunk_bytes=cut) as g:
        got = read_all(g)
    for (name, d, n, st), (_, d0, _, _) in zip(got, base):
        assert (d is None and d0 is None) or np.array_equal(d, d0), name


@pytest.mark.gpu
@pytest.mark.parametrize("chunk,max_resident", [(0, 2), (4097, 3), (0, 6)], ids=["one_chunk_2buf", "4k_3buf", "one_chunk_6buf"])
def test_hundreds_of_tiny_contigs(tmp_path, chunk, max_resident):
    """360 contigs of 200-2000 bases inside one chunk: the boundary list and the segment tables carry many entries, and
    with few depth buffers the reader stops inside the chunk until the caller gives one back."""
    from rsicnv_amd import api
    rng = np.random.default_rng(11)
    lines, names, lens, depths = ["# tiny"], [], [], {}
    for i in range(360):
        n = int(rng.integers(200, 2001))
        name = f"ctg{i:04d}"
        depth = rng.integers(0, 90, n).astype(np.int32)
        names.append(name); lens.append(n); depths[name] = depth
        for pos in range(1, n + 2 if i % 5 == 0 else n + 1):
            d = int(depth[pos - 1]) if pos <= n else 4
            lines.append((name, f"{pos}\t{d}", pos, d))
        if i % 17 == 0:
            lines.append("")
    path = tmp_path / "tiny.depth"
    path.write_text(render(lines, 4))
    seen = []
    with api.GenomeText(str(path), names, lens, chunk_bytes=chunk, max_resident=max_resident) as g:
        for name, ptr, n, st in g:
            assert ptr is not None and st["fallback"] == 0
            d = g.depth(st["slot"])
            assert np.array_equal(d, restate(lines, name, n)), name
            seen.append(name)
    assert seen == names


@pytest.mark.gpu
def test_contiguity_error_names_the_chromosome(tmp_path):
    from rsicnv_amd import api
    lines = [("chrA", f"{p}\t5", p, 5) for p in range(1, 3000)] + [("chrB", f"{p}\t6", p, 6) for p in range(1, 3000)]
    lines += [("chrA", f"{p}\t7", p, 7) for p in range(3000, 3100)]
    path = tmp_path / "broken.depth"
    path.write_text(render(lines, 5))
    with api.GenomeText(str(path), ["chrA", "chrB"], [5000, 5000]) as g:
        with pytest.raises(api.RsiError) as e:
            list(g)
    assert "chrA" in str(e.value) and "contiguous" in str(e.value)


@pytest.mark.gpu
def test_run_genome_text_through_a_pool(hotlib, tmp_path):
    """The convenience call: every chromosome through an RsiPool; the calls equal the single-chromosome text path's."""
    from rsicnv_amd import api
    cases, lines, order, fai_seqs = genome_case(hotlib)
    path = tmp_path / "genome.depth"
    path.write_text(render(lines, 6))
    names, lens = fai_of(fai_seqs)
    by_file_name = {"chrA": "chrA", "5": "chr5", "chrC": "chrC", "chrD": "chrD", "chrE": "chrE", "chrF": "chrF"}
    fasta = {nm: cases[nm][0] for nm in by_file_name}
    res = api.run_genome_text(str(path), names, lens, fasta, workers=3)
    assert list(res) == order
    h = api.RsiHot(0)
    for name in order:
        sl = tmp_path / f"slice_{name}.txt"
        sl.write_text(slice_text(lines, name))
        r1 = h.run_text(api.make_params(), str(sl), cases[name][0])
        assert res[name].format_rows(name) == r1.format_rows(name), name
    h.close()


# ---------------------------------------------------------------------------------------------------------------------
# command line
# ---------------------------------------------------------------------------------------------------------------------

def cli_case(hotlib, tmp):
    """Three chromosomes with calls, a skipped MT contig and comments: the genome file, its slices, the reference."""
    specs = [("chrP", dict(n=400_007, seed=0xC21, model=1, n_events=5, gaps=1, max_len=20000, end_n=5000, gap_len=8000)),
             ("chrQ", dict(n=350_019, seed=0xC22, model=0, n_events=4, gaps=1, max_len=20000, end_n=5000, gap_len=8000)),
             ("chrR", dict(n=300_001, seed=0xC23, model=1, n_events=4, gaps=0, max_len=15000, end_n=4000))]
    lines, seqs = ["#genome"], []
    for i, (name, kw) in enumerate(specs):
        _, fasta, depth = make_case(hotlib, kw)
        seqs.append((name, fasta))
        lines += chrom_lines(name, depth, fasta.size, 200 + i, quirks=False)
        if i == 0:
            lines += [("chrMT", f"{p}\t9", p, 9) for p in range(1, 500)] + [""]
    fa = os.path.join(tmp, "ref.fa")
    write_fasta(fa, list(reversed(seqs)))                   # .fai order differs from the file's: rows follow the file
    genome = os.path.join(tmp, "genome.depth")
    with open(genome, "w") as f:
        f.write(render(lines, 7))
    slices = []
    for name, _ in specs:
        sl = os.path.join(tmp, f"slice_{name}.txt")
        with open(sl, "w") as f:
            f.write(slice_text(lines, name))
        slices.append((name, sl))
    return fa, genome, slices


def rows_of(path):
    return [l for l in open(path).read().splitlines() if not l.startswith("#")]


def processing_order(path):
    return [l.split()[1] for l in open(path + ".log").read().splitlines() if l.startswith("#processing ")]


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [[], ["-MED", "-m", "51"], ["-NOGC"]], ids=["nb", "med51", "nogc"])
def test_cli_genome_mode_equals_per_chromosome_runs(hotlib, tmp_path, extra):
    import oracle
    tmp = str(tmp_path)
    fa, genome, slices = cli_case(hotlib, tmp)
    out = os.path.join(tmp, "out.txt")
    r = subprocess.run([EXE, "rsi", "-f", fa, "-d", genome, "-o", out, "-np"] + extra, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    text = open(out).read()
    assert text.startswith(f"#input {genome}\n") and text.count("#CHROM") == 1
    assert ("#GC adjusted\n" in text) == ("-NOGC" not in extra)
    assert processing_order(out) == [nm for nm, _ in slices]
    # our own single-chromosome path on each slice
    mine = []
    for name, sl in slices:
        o1 = os.path.join(tmp, f"one_{name}.txt")
        subprocess.run([EXE, "rsi", "-f", fa, "-d", sl, "-c", name, "-o", o1, "-np"] + extra, check=True, capture_output=True, timeout=300)
        mine += rows_of(o1)
    assert rows_of(out) == mine and len(mine) >= 3
    # the log blocks: the same lines, timing lines aside
    def blocks(path):
        t = open(path + ".log").read().splitlines()
        t = t[next(i for i, l in enumerate(t) if l.startswith("#processing ")):]
        return [l for l in t if not l.startswith(("timing:", "output written to"))]
    assert blocks(out) == sum((blocks(os.path.join(tmp, f"one_{name}.txt")) for name, _ in slices), [])
    # the compiled reference on each slice
    if os.path.exists(oracle.REF_BIN):
        theirs = []
        for name, sl in slices:
            o2 = os.path.join(tmp, f"ref_{name}.txt")
            subprocess.run([oracle.REF_BIN, "rsi", "-f", fa, "-d", sl, "-c", name, "-o", o2, "-np"] + extra, check=True,
                           capture_output=True, timeout=900, cwd=tmp)
            theirs += rows_of(o2)
        assert rows_of(out) == theirs
    # one worker or four: the same file
    out1 = os.path.join(tmp, "out_w1.txt")
    subprocess.run([EXE, "rsi", "-f", fa, "-d", genome, "-o", out1, "-np", "-workers", "1"] + extra, check=True, capture_output=True, timeout=600)
    out4 = os.path.join(tmp, "out_w4.txt")
    subprocess.run([EXE, "rsi", "-f", fa, "-d", genome, "-o", out4, "-np", "-workers", "4"] + extra, check=True, capture_output=True, timeout=600)
    assert open(out1).read() == open(out4).read() == text


@pytest.mark.gpu
def test_cli_genome_contiguity_error_leaves_no_output(tmp_path):
    tmp = str(tmp_path)
    rng = np.random.default_rng(2)
    seqs = [(nm, rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), 20_000)) for nm in ("chrA", "chrB")]
    fa = os.path.join(tmp, "ref.fa")
    write_fasta(fa, seqs)
    lines = [("chrA", f"{p}\t30", p, 30) for p in range(1, 20_000)] + [("chrB", f"{p}\t30", p, 30) for p in range(1, 20_000)]
    lines += [("chrA", "20000\t30", 20000, 30)]
    genome = os.path.join(tmp, "broken.depth")
    with open(genome, "w") as f:
        f.write(render(lines, 8))
    out = os.path.join(tmp, "out.txt")
    r = subprocess.run([EXE, "rsi", "-f", fa, "-d", genome, "-o", out, "-np"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "chrA" in r.stderr and "contiguous" in r.stderr
    assert not os.path.exists(out)


def test_cli_refuses_two_column_file_without_chromosome(tmp_path):
    """A "pos depth" file without -c is not read as chromosomes named 1, 2, ...: today's message."""
    path = tmp_path / "two.txt"
    path.write_text("# pos depth\n1\t30\n2\t31\n3\t29\n")
    fa = tmp_path / "ref.fa"
    write_fasta(str(fa), [("chr1", np.frombuffer(b"ACGT" * 10, dtype=np.uint8))])
    r = subprocess.run([EXE, "rsi", "-f", str(fa), "-d", str(path), "-o", str(tmp_path / "out.txt"), "-np"],
                       capture_output=True, text=True, timeout=60)
    assert "readdepth file and chromosome must be specified together" in r.stderr
    assert not os.path.exists(tmp_path / "out.txt")


def test_cli_genome_mode_is_one_device_and_in_the_usage(tmp_path):
    path = tmp_path / "g.depth"
    path.write_text("chr1\t1\t30\n")
    r = subprocess.run([EXE, "rsi", "-f", str(tmp_path / "ref.fa"), "-d", str(path), "-gpus", "2", "-o", str(tmp_path / "o.txt")],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "one device" in r.stderr
    u = subprocess.run([EXE], capture_output=True, text=True)
    assert "-d GENOME.depth" in u.stderr


def test_genome_reader_in_the_abi(hotlib):
    from rsicnv_amd import api
    for sym in ("rsi_genome_text_open", "rsi_genome_text_next", "rsi_genome_text_release", "rsi_genome_text_close",
                "rsi_genome_text_last_error", "rsi_hot_run_depth_device"):
        assert sym in api.EXPORTS and hasattr(hotlib, sym)
    import ctypes as C
    assert C.sizeof(api.RsiGenomeChrom) == 8 + 8 + 8 + C.sizeof(api.RsiTextStats) + 256
