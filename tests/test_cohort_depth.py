"""Cohort depth files: "RNAME pos d1 d2 ... dK" (samtools depth -a s1.bam ... sK.bam), every selected depth column called as a
sample of its own (rsi_genome_text_open_samples, `rsicnv rsi -d COHORT -samples all|LIST`).  The rule that defines
correctness: sample k of a line is what `iss >> pos >> d1 >> ... >> dk` leaves in dk (0 once an extraction fails or the line
has fewer tokens), and for every selected k the reader and the command line give what today's genome reader gives on the
derived file k -- the same lines with the depth part replaced by that dk."""
import os
import subprocess

import numpy as np
import pytest

import bgzf_util as bz
import text_rules as tr
from conftest import make_case
from test_genome_text import EXE, render, slice_text, write_fasta

STATS = ("lines", "stored", "beyond", "fallback")


# ---------------------------------------------------------------------------------------------------------------------
# the line rule, restated: derived files
# ---------------------------------------------------------------------------------------------------------------------

def derive(rest, k):
    """A cohort line's part behind the name -> derived file k's: the position as it is, then dk (tests/text_rules.py: what
    `iss >> pos >> d1 >> ... >> dk` leaves in dk)."""
    ok, pos, q = tr.extract(rest, 0)
    if not ok:
        return rest                                         # no position (or an overflowing one): the same in either file
    return f"{rest[:q]}\t{tr.columns(rest, k)[1][k - 1]}"


def derived_lines(lines, k):
    return [ln if isinstance(ln, str) else (ln[0], derive(ln[1], k)) for ln in lines]


def cohort_lines(name, depths, n, seed, quirks=True, unsorted=False):
    """Data lines (name, rest) of one chromosome with K depth columns (depths: K x n), running past the end; with quirks:
    mixed blanks, '\\r', missing positions, pos < 1, short lines, non-numeric and sign-only tokens mid-line."""
    K = depths.shape[0]
    seps = ["\t", " ", "  ", "\t "]
    out = []
    for pos in range(1, n + 3):
        if quirks and pos % 1009 == 0:
            continue                                        # missing position: stays 0
        d = [int(depths[s, pos - 1]) if pos <= n else 55 + s for s in range(K)]
        sep = seps[pos % 4] if quirks else "\t"
        toks = [str(x) for x in d]
        if quirks and pos % 97 == 0:
            toks = toks[:pos % K]                           # fewer depth columns than K (none at all for some)
        elif quirks and pos % 89 == 0 and K > 2:
            toks[2] = f"{d[2]}abc"                          # column 3 reads 12 of "12abc", columns 4.. read 0
        elif quirks and pos % 83 == 0 and K > 1:
            toks[1] = "- 5"                                 # a sign without digits: columns 2.. read 0
        elif quirks and pos % 79 == 0 and K > 3:
            toks[3] = "+" + toks[3]
        rest = sep.join([str(pos)] + toks) + ("\r" if quirks and pos % 7 == 0 else "")
        out.append((name, rest))
    if quirks:
        mid = len(out) // 2
        out.insert(mid, (name, "0\t99\t98\t97\t96\t95"))     # pos < 1: skipped
        out.insert(mid + 1, (name, "-4 12 13"))
        out.insert(mid + 2, (name, "x 12 13"))               # no position
    if unsorted:                                            # a repeated position: the order-dependent rules are in play
        q = len(out) // 3
        out.insert(q + 1, out[q - 5])
    return out


def sample_depths(hotlib, n, seeds, model=1):
    """K depth arrays of one chromosome (each with its own CNV events) and the chromosome's sequence (the first seed's)."""
    fasta, rows = None, []
    for i, sd in enumerate(seeds):
        _, fa, d = make_case(hotlib, dict(n=n, seed=sd, model=model, n_events=4, gaps=1, max_len=20000, end_n=5000, gap_len=8000))
        fasta = fa if fasta is None else fasta
        rows.append(d)
    return fasta, np.stack(rows)


def cohort_case(hotlib, K=5, unsorted_chrom=None, quirks=True):
    """Three chromosomes with K samples each, an unknown contig and comments, behind a #CHROM POS header."""
    specs = [("chrA", 200_003, 0x7A01), ("chrB", 150_001, 0x7A02), ("chrC", 260_017, 0x7A03)]
    lines = ["#CHROM\tPOS\t" + "\t".join(f"S{s + 1}" for s in range(K)), "# cohort"]
    seqs = []
    for i, (name, n, seed) in enumerate(specs):
        fasta, depths = sample_depths(hotlib, n, [seed + 16 * s for s in range(K)])
        seqs.append((name, fasta))
        lines += cohort_lines(name, depths, n, i, quirks=quirks, unsorted=(name == unsorted_chrom))
        lines += ["# between", ""]
        if i == 0:
            lines += [("chrUn_missing", f"{p}\t7\t8") for p in range(1, 1500)]
    return lines, seqs


def genome_of(path, names, lens, **kw):
    """{name: (depth or None, stats)} of today's genome reader."""
    from rsicnv_amd import api
    out = {}
    with api.GenomeText(str(path), names, lens, **kw) as g:
        for name, ptr, n, st in g:
            out[name] = (None if ptr is None else g.depth(st["slot"]), st)
    return out


def cohort_of(path, names, lens, samples, **kw):
    """{name: ([depth of each sample] or None, stats)} of the cohort reader."""
    from rsicnv_amd import api
    out = {}
    with api.GenomeText(str(path), names, lens, samples=samples, **kw) as g:
        assert g.samples == list(samples)
        for name, ptr, n, st in g:
            if ptr is None:
                out[name] = (None, st)
                continue
            ds = [g.sample_depth(st["slot"], j) for j in range(len(samples))]
            assert np.array_equal(ds[0], g.depth(st["slot"]))
            out[name] = (ds, st)
    return out


def check_against_derived(tmp_path, lines, names, lens, samples, tag, text_seed=1, **kw):
    got = cohort_of(tmp_path / f"{tag}.depth", names, lens, samples, **kw)
    for j, k in enumerate(samples):
        dpath = tmp_path / f"{tag}_derived_{k}.depth"
        dpath.write_text(render(derived_lines(lines, k), text_seed))
        ref = genome_of(dpath, names, lens)
        assert list(got) == list(ref), (k, list(got), list(ref))
        for name, (d, st) in ref.items():
            ds, cst = got[name]
            if d is None:
                assert ds is None
                continue
            assert np.array_equal(ds[j], d), (k, name, int(np.sum(ds[j] != d)))
            for s in STATS:
                assert cst[s] == st[s], (k, name, s, cst[s], st[s])
    return got


# ---------------------------------------------------------------------------------------------------------------------
# CPU: refusals and the ABI
# ---------------------------------------------------------------------------------------------------------------------

def _refused(tmp_path, depth_text, args):
    d = tmp_path / "c.depth"
    d.write_text(depth_text)
    out = tmp_path / "out.txt"
    r = subprocess.run([EXE, "rsi", "-f", str(tmp_path / "ref.fa"), "-d", str(d), "-o", str(out), "-np"] + args,
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 1, (args, r.returncode, r.stderr)
    assert not [p for p in os.listdir(tmp_path) if p.startswith("out.txt")], (args, os.listdir(tmp_path))
    return r.stderr


COHORT3 = "#CHROM\tPOS\ta\tb\tc\nchr1\t1\t30\t31\t32\nchr1\t2\t30\t31\t32\n"


@pytest.mark.parametrize("args,msg", [
    (["-samples", "all", "-c", "chr1"], "without -c"),
    (["-samples", "all", "-b", "x.bam"], "not a BAM file"),
    (["-samples", "all", "-gpus", "2"], "one device"),
    (["-samples", "4"], "not a depth column"),
    (["-samples", "0"], "not a depth column"),
    (["-samples", "2,1,2"], "selected twice"),
    (["-samples", "1,x"], "not a depth column"),
    (["-samples", ""], "-samples"),
], ids=["with_c", "with_b", "gpus2", "k_plus_1", "zero", "duplicate", "not_a_number", "empty"])
def test_samples_refusals(tmp_path, args, msg):
    assert msg in _refused(tmp_path, COHORT3, args)


def test_samples_refuses_a_two_column_file(tmp_path):
    assert "readdepth file and chromosome must be specified together" in _refused(tmp_path, "1\t30\n2\t31\n", ["-samples", "all"])


def test_samples_refuses_more_than_64_columns(tmp_path):
    line = "chr1\t1\t" + "\t".join(["5"] * 65) + "\n"
    assert "more than 64" in _refused(tmp_path, line, ["-samples", "all"])
    assert "at most 64" in _refused(tmp_path, line, ["-samples", ",".join(str(k) for k in range(1, 66))])


def test_samples_in_the_usage():
    u = subprocess.run([EXE], capture_output=True, text=True)
    assert "-samples" in u.stderr and "-d GENOME.depth" in u.stderr


def test_cohort_reader_in_the_abi(hotlib):
    from rsicnv_amd import api
    for sym in ("rsi_genome_text_open_samples", "rsi_genome_text_samples", "rsi_genome_text_max_resident",
                "rsi_genome_text_sample_depth", "rsi_genome_text_copy_sample_depth", "rsi_synth_append_genome_samples"):
        assert sym in api.EXPORTS and hasattr(hotlib, sym)


def test_line_rule_restatement():
    assert derive("7\t1\t2\t3", 2) == "7\t2"
    assert derive("7 12abc 9", 1) == "7\t12" and derive("7 12abc 9", 2) == "7\t0"
    assert derive("7\t- 5\t6", 1) == "7\t0" and derive("7\t- 5\t6", 2) == "7\t0"
    assert derive("7\t1", 3) == "7\t0" and derive("x 1 2", 1) == "x 1 2"


def test_synth_writer_lines(hotlib, tmp_path):
    from rsicnv_amd import api
    lib = api.load_library()
    d = np.array([[1, 2, 3], [4, -5, 6]], dtype=np.int32)
    p = tmp_path / "s.depth"
    assert lib.rsi_synth_append_genome_samples(str(p).encode(), b"chrZ", d.ctypes.data, 2, 3, 0) == 0
    assert p.read_text() == "chrZ\t1\t1\t4\nchrZ\t2\t2\t-5\nchrZ\t3\t3\t6\n"
    pz = tmp_path / "s.depth.gz"
    assert lib.rsi_synth_append_genome_samples(str(pz).encode(), b"chrZ", d.ctypes.data, 2, 3, 1) == 0
    import gzip
    assert gzip.decompress(pz.read_bytes()).decode() == p.read_text()


# ---------------------------------------------------------------------------------------------------------------------
# device: the reader against the derived files
# ---------------------------------------------------------------------------------------------------------------------

def fai_names(seqs):
    return [nm for nm, _ in seqs], [int(s.size) for _, s in seqs]


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_cohort_reader_equals_derived_files(hotlib, tmp_path):
    lines, seqs = cohort_case(hotlib)
    (tmp_path / "cohort.depth").write_text(render(lines, 1))
    names, lens = fai_names(seqs)
    for samples in ([1, 2, 3, 4, 5], [4, 2]):
        got = check_against_derived(tmp_path, lines, names, lens, samples, "cohort")
        assert list(got) == ["chrA", "chrUn_missing", "chrB", "chrC"]
        for name in ("chrA", "chrB", "chrC"):
            assert got[name][1]["fallback"] == 0 and got[name][1]["beyond"] == 3


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_cohort_unsorted_chromosome_falls_back_alone(hotlib, tmp_path):
    lines, seqs = cohort_case(hotlib, K=4, unsorted_chrom="chrB")
    (tmp_path / "cohort.depth").write_text(render(lines, 2))
    names, lens = fai_names(seqs)
    got = check_against_derived(tmp_path, lines, names, lens, [3, 1, 4, 2], "cohort", text_seed=2)
    assert {nm: got[nm][1]["fallback"] for nm in ("chrA", "chrB", "chrC")} == {"chrA": 0, "chrB": 1, "chrC": 0}


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_cohort_geometry_does_not_change_the_depth(tmp_path):
    """360 tiny contigs with 3 samples: 4 KiB chunks and two depth buffers against one chunk and the default buffers."""
    rng = np.random.default_rng(12)
    lines, names, lens = ["#CHROM\tPOS\tx\ty\tz"], [], []
    for i in range(360):
        n = int(rng.integers(200, 2001))
        name = f"ctg{i:04d}"
        depths = rng.integers(0, 90, (3, n)).astype(np.int32)
        names.append(name); lens.append(n)
        lines += cohort_lines(name, depths, n, i, quirks=(i % 3 == 0))
        if i % 17 == 0:
            lines.append("")
    (tmp_path / "tiny.depth").write_text(render(lines, 4))
    base = check_against_derived(tmp_path, lines, names, lens, [1, 2, 3], "tiny", text_seed=4)
    small = cohort_of(tmp_path / "tiny.depth", names, lens, [1, 2, 3], chunk_bytes=4097, max_resident=2)
    assert list(small) == list(base) == names
    for name in names:
        assert all(np.array_equal(a, b) for a, b in zip(small[name][0], base[name][0])), name
        assert all(small[name][1][s] == base[name][1][s] for s in STATS), name


@pytest.mark.gpu
@pytest.mark.timeout(1200)
def test_cohort_compressed_equals_text(hotlib, tmp_path):
    lines, seqs = cohort_case(hotlib, K=3, unsorted_chrom="chrC")
    text = render(lines, 5).encode()
    names, lens = fai_names(seqs)
    (tmp_path / "plain.depth").write_bytes(text)
    ref = cohort_of(tmp_path / "plain.depth", names, lens, [2, 3, 1])
    rng = np.random.default_rng(5)
    forms = {"bgzf_small": bz.bgzf(text, sizes=iter(lambda: int(rng.integers(100, 4001)), None)), "bgzf": bz.bgzf(text),
             "gzip": bz.gzip_members(text, parts=3)}
    for form, data in forms.items():
        p = tmp_path / f"{form}.depth.gz"
        p.write_bytes(data)
        for chunk in (0, 131072):
            got = cohort_of(p, names, lens, [2, 3, 1], chunk_bytes=chunk)
            assert list(got) == list(ref), form
            for name, (ds, st) in ref.items():
                if ds is None:
                    continue
                assert all(np.array_equal(a, b) for a, b in zip(got[name][0], ds)), (form, chunk, name)
                assert all(got[name][1][s] == st[s] for s in STATS), (form, chunk, name)


# ---------------------------------------------------------------------------------------------------------------------
# command line
# ---------------------------------------------------------------------------------------------------------------------

def cli_cohort(hotlib, tmp, K=3, zero=None):
    """Three chromosomes with calls in every sample, a skipped MT contig; zero=(sample, chromosome): that sample's depth is
    0 all along that chromosome.  Returns the FASTA, the cohort file and its lines."""
    specs = [("chrP", 400_007, 0xC31), ("chrQ", 350_019, 0xC32), ("chrR", 300_001, 0xC33)]
    lines, seqs = ["#CHROM\tPOS\t" + "\t".join(f"NA{100 + s}" for s in range(K))], []
    for i, (name, n, seed) in enumerate(specs):
        fasta, depths = sample_depths(hotlib, n, [seed + 16 * s for s in range(K)], model=i % 2)
        depths[:, n - 1] = 0
        if zero is not None and zero[1] == name:
            depths[zero[0] - 1] = 0
        seqs.append((name, fasta))
        lines += cohort_lines(name, depths, n, 200 + i, quirks=False)
        if i == 0:
            lines += [("chrMT", f"{p}\t9\t9\t9") for p in range(1, 500)] + [""]
    fa = os.path.join(tmp, "ref.fa")
    write_fasta(fa, list(reversed(seqs)))
    cohort = os.path.join(tmp, "cohort.depth")
    with open(cohort, "w") as f:
        f.write(render(lines, 7))
    return fa, cohort, lines, [nm for nm, _, _ in specs]


def _cli(args, timeout=900):
    return subprocess.run([EXE, "rsi"] + args, capture_output=True, text=True, timeout=timeout)


def _blocks(path):
    t = open(path + ".log").read().splitlines()
    t = t[next((i for i, l in enumerate(t) if l.startswith("#processing ")), len(t)):]
    return [l for l in t if not l.startswith(("timing:", "output written to"))]


def check_cli_against_derived(tmp, fa, cohort, lines, samples_arg, ks, extra, names=None):
    """`-samples samples_arg` once, then every derived file k as today's genome run: OUT.k == that run's OUT past line 1,
    the same log blocks, line 1 names the sample."""
    out = os.path.join(tmp, "out.txt")
    r = _cli(["-f", fa, "-d", cohort, "-o", out, "-np", "-samples", samples_arg] + extra)
    assert r.returncode == 0, r.stderr[-3000:]
    assert not os.path.exists(out)
    log = open(out + ".log").read()
    for j, k in enumerate(ks):
        assert f"#sample {k}" + (f": {names[j]}" if names else "") + "\n" in log
    for j, k in enumerate(ks):
        dk = os.path.join(tmp, f"derived_{k}.depth")
        with open(dk, "w") as f:
            f.write(render(derived_lines(lines, k), 7))
        ok = os.path.join(tmp, f"one_{k}.txt")
        r1 = _cli(["-f", fa, "-d", dk, "-o", ok, "-np"] + extra)
        assert r1.returncode == 0, r1.stderr[-3000:]
        mine = open(f"{out}.{k}").read().split("\n", 1)
        assert mine[0] == f"#input {cohort} sample {k}" + (f" {names[j]}" if names else ""), mine[0]
        assert mine[1] == open(ok).read().split("\n", 1)[1], k
        assert _blocks(f"{out}.{k}") == _blocks(ok), k
    return out


@pytest.mark.gpu
@pytest.mark.timeout(2400)
@pytest.mark.parametrize("extra", [[], ["-MED", "-m", "51"], ["-NOGC"]], ids=["nb", "med51", "nogc"])
def test_cli_samples_equal_derived_runs(hotlib, tmp_path, extra):
    import oracle
    tmp = str(tmp_path)
    fa, cohort, lines, chroms = cli_cohort(hotlib, tmp)
    out = check_cli_against_derived(tmp, fa, cohort, lines, "all", [1, 2, 3], extra, names=["NA100", "NA101", "NA102"])
    for k in (1, 2, 3):
        assert len([l for l in open(f"{out}.{k}") if not l.startswith("#")]) >= 2, k
    # one worker or four: the same files
    for w in ("1", "4"):
        ow = os.path.join(tmp, f"out_w{w}.txt")
        r = _cli(["-f", fa, "-d", cohort, "-o", ow, "-np", "-samples", "3,1", "-workers", w] + extra)
        assert r.returncode == 0, r.stderr[-3000:]
        for k in (3, 1):
            assert open(f"{ow}.{k}").read() == open(f"{out}.{k}").read(), (w, k)
        assert not os.path.exists(f"{ow}.2")
    # the compiled reference on the per-chromosome slices of each derived file
    if os.path.exists(oracle.REF_BIN):
        for k in (1, 2, 3):
            dl = derived_lines(lines, k)
            theirs = []
            for name in chroms:
                sl = os.path.join(tmp, f"slice_{k}_{name}.txt")
                with open(sl, "w") as f:
                    f.write(slice_text(dl, name))
                o2 = os.path.join(tmp, f"ref_{k}_{name}.txt")
                subprocess.run([oracle.REF_BIN, "rsi", "-f", fa, "-d", sl, "-c", name, "-o", o2, "-np"] + extra, check=True,
                               capture_output=True, timeout=900, cwd=tmp)
                theirs += [l for l in open(o2).read().splitlines() if not l.startswith("#")]
            assert [l for l in open(f"{out}.{k}").read().splitlines() if not l.startswith("#")] == theirs, k


@pytest.mark.gpu
@pytest.mark.timeout(1200)
def test_cli_sample_failure_ends_that_sample_only(hotlib, tmp_path):
    """Sample 2 has no depth at all on chrQ: whatever the library makes of that, OUT.2 and its log are the derived run's,
    and samples 1 and 3 are complete."""
    tmp = str(tmp_path)
    fa, cohort, lines, chroms = cli_cohort(hotlib, tmp, zero=(2, "chrQ"))
    out = check_cli_against_derived(tmp, fa, cohort, lines, "1,2,3", [1, 2, 3], [], names=["NA100", "NA101", "NA102"])
    for k in (1, 3):
        assert [l.split()[1] for l in open(f"{out}.{k}.log") if l.startswith("#processing ")] == chroms, k


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_cli_samples_all_on_a_three_column_file(hotlib, tmp_path):
    tmp = str(tmp_path)
    fa, cohort, lines, chroms = cli_cohort(hotlib, tmp, K=1)
    out = os.path.join(tmp, "out.txt")
    r = _cli(["-f", fa, "-d", cohort, "-o", out, "-np", "-samples", "all"])
    assert r.returncode == 0, r.stderr[-3000:]
    plain = os.path.join(tmp, "plain.txt")
    r = _cli(["-f", fa, "-d", cohort, "-o", plain, "-np"])
    assert r.returncode == 0, r.stderr[-3000:]
    mine, theirs = open(out + ".1").read().split("\n", 1), open(plain).read().split("\n", 1)
    assert mine[0] == f"#input {cohort} sample 1 NA100" and theirs[0] == f"#input {cohort}"
    assert mine[1] == theirs[1]
    assert _blocks(out + ".1") == _blocks(plain)


@pytest.mark.gpu
@pytest.mark.timeout(900)
@pytest.mark.parametrize("form", ["bgzf", "gzip"])
def test_cli_samples_compressed_and_broken(hotlib, tmp_path, form):
    """A compressed cohort file gives its text's OUT.k; one cut short exits 1 and leaves no OUT.k."""
    tmp = str(tmp_path)
    fa, cohort, lines, chroms = cli_cohort(hotlib, tmp)
    text = open(cohort, "rb").read()
    data = bz.bgzf(text) if form == "bgzf" else bz.gzip_members(text, parts=3)
    packed = os.path.join(tmp, "cohort.depth.gz")
    with open(packed, "wb") as f:
        f.write(data)
    o1, o2 = os.path.join(tmp, "o_text.txt"), os.path.join(tmp, "o_packed.txt")
    for src, o in ((cohort, o1), (packed, o2)):
        r = _cli(["-f", fa, "-d", src, "-o", o, "-np", "-samples", "2,3"])
        assert r.returncode == 0, r.stderr[-3000:]
    for k in (2, 3):
        assert open(f"{o1}.{k}").read().split("\n", 1)[1] == open(f"{o2}.{k}").read().split("\n", 1)[1], k
        assert _blocks(f"{o1}.{k}") == _blocks(f"{o2}.{k}"), k
    cut = os.path.join(tmp, "cut.depth.gz")
    with open(cut, "wb") as f:
        f.write(data[:int(len(data) * 0.6)])
    o3 = os.path.join(tmp, "o_cut.txt")
    r = _cli(["-f", fa, "-d", cut, "-o", o3, "-np", "-samples", "all"])
    assert r.returncode == 1 and "offset" in r.stderr, (r.returncode, r.stderr[-2000:])
    assert not [p for p in os.listdir(tmp) if p.startswith("o_cut.txt.") and p != "o_cut.txt.log"], os.listdir(tmp)
