"""`rsicnv rsi ... -track FILE.gz -bintrack FILE.gz -trackindex`: the .tbi files the command line leaves beside its BGZF tracks,
joined from the part files' indexes with each part's offset.  Both answer region queries as a tabix reader makes them; a
plain-text track is refused before any output; without -trackindex nothing changes."""
import glob
import gzip
import os
import subprocess

import numpy as np
import pytest

import bgzf_walk as bw
import tabix_util as tx
from conftest import make_case
from test_genome_text import EXE, chrom_lines, render, rows_of, write_fasta

SPECS = [("chrP", dict(n=300_007, seed=0xD21, model=1, n_events=4, gaps=1, max_len=20000, end_n=5000, gap_len=8000)),
         ("chrQ", dict(n=250_019, seed=0xD22, model=0, n_events=4, gaps=0, max_len=15000, end_n=4000)),
         ("chrR", dict(n=200_003, seed=0xD23, model=0, n_events=3, gaps=0, max_len=15000, end_n=4000))]


def _cli(args, timeout=600):
    return subprocess.run([EXE, "rsi"] + args, capture_output=True, text=True, timeout=timeout)


@pytest.fixture(scope="module")
def genome(hotlib, tmp_path_factory):
    """Three chromosomes in one whole-genome depth file."""
    tmp = str(tmp_path_factory.mktemp("index_cli"))
    lines, seqs = [], []
    for i, (name, kw) in enumerate(SPECS):
        _, fasta, depth = make_case(hotlib, kw)
        seqs.append((name, fasta))
        lines += chrom_lines(name, depth, fasta.size, 300 + i, quirks=False)
    fa = os.path.join(tmp, "ref.fa")
    write_fasta(fa, seqs)
    depth_file = os.path.join(tmp, "genome.depth")
    with open(depth_file, "w") as f:
        f.write(render(lines, 7))
    return dict(tmp=tmp, fa=fa, depth=depth_file)


def test_trackindex_in_the_usage_and_refused_for_a_text_track(tmp_path):
    u = subprocess.run([EXE], capture_output=True, text=True)
    assert "-trackindex" in u.stderr and "FILE.tbi" in u.stderr and "-dindex PATH|none" in u.stderr
    d = tmp_path / "d.txt"
    d.write_text("1\t30\n2\t31\n")
    for extra in (["-track", str(tmp_path / "t.bedgraph")], ["-track", str(tmp_path / "t.gz"), "-trackformat", "text"], ["-bintrack", str(tmp_path / "b.txt")], []):
        r = _cli(["-f", str(tmp_path / "ref.fa"), "-d", str(d), "-c", "chrS", "-o", str(tmp_path / "o.txt"), "-np", "-trackindex"] + extra)
        assert r.returncode != 0 and "-trackindex" in r.stderr and "BGZF" in r.stderr, r.stderr
        assert sorted(os.listdir(tmp_path)) == ["d.txt"]


def test_trackindex_refuses_a_sequence_beyond_the_format(tmp_path):
    d = tmp_path / "d.txt"
    d.write_text("1\t30\n")
    fa = tmp_path / "ref.fa"
    (tmp_path / "ref.fa.fai").write_text(f"chrS\t1000\t6\t60\t61\nchrBig\t{2**29 + 1}\t2000\t60\t61\n")
    r = _cli(["-f", str(fa), "-d", str(d), "-c", "chrBig", "-o", str(tmp_path / "o.txt"), "-np", "-track", str(tmp_path / "t.gz"), "-trackindex"])
    assert r.returncode == 1 and "536870912" in r.stderr and "chrBig" in r.stderr
    assert sorted(os.listdir(tmp_path)) == ["d.txt", "ref.fa.fai"]
    # without -c every sequence of the .fai can be written: the long one is refused all the same, for either kind of input
    for inp in (["-d", str(d)], ["-b", str(tmp_path / "reads.bam")]):
        for extra in (["-track", str(tmp_path / "t.gz")], ["-bintrack", str(tmp_path / "b.bgz")]):
            r = _cli(["-f", str(fa)] + inp + ["-o", str(tmp_path / "o.txt"), "-np", "-trackindex"] + extra)
            assert r.returncode == 1 and "536870912" in r.stderr and "chrBig" in r.stderr, r.stderr
            assert sorted(os.listdir(tmp_path)) == ["d.txt", "ref.fa.fai"]
    # -c names the short one, with or without chr: the long one is not this run's
    for c in ("chrS", "S"):
        r = _cli(["-f", str(fa), "-d", str(d), "-c", c, "-o", str(tmp_path / "o.txt"), "-np", "-track", str(tmp_path / "t.gz"), "-trackindex"])
        assert "536870912" not in r.stderr
    for f in os.listdir(tmp_path):
        if f not in ("d.txt", "ref.fa.fai"):
            os.unlink(tmp_path / f)


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_both_tracks_are_indexed_and_answer_queries(genome):
    g = genome
    tmp = g["tmp"]
    out, track, bins = os.path.join(tmp, "x.txt"), os.path.join(tmp, "t.bedgraph.gz"), os.path.join(tmp, "b.bedgraph.gz")
    r = _cli(["-f", g["fa"], "-d", g["depth"], "-o", out, "-np", "-track", track, "-bintrack", bins, "-trackindex"])
    assert r.returncode == 0, r.stderr[-3000:]
    log = open(out + ".log").read()
    assert log.count(", index: ") == 6 and f"track index written to {track}.tbi" in log and f"bin track index written to {bins}.tbi" in log
    rng = np.random.default_rng(8)
    for path in (track, bins):
        data = open(path, "rb").read()
        text = gzip.decompress(data)
        table = tx.member_table(data)
        bw.check_file(data, text)
        index = tx.parse_index(path + ".tbi")
        assert index["names"] == [s[0] for s in SPECS]
        exp = tx.expected_index(text, table)
        assert tx.resolved(index, table) == {k: dict(chunks=v["chunks"], linear=v["linear"]) for k, v in exp.items()}
        for name, kw in SPECS:
            n = kw["n"]
            regions = [(int(a), int(a) + int(w)) for a, w in zip(rng.integers(0, n, 6), rng.choice([1, 100, 40_000], 6))]
            for beg, end in regions + [(0, 1), (16_383, 16_385), (n - 1, n), (0, n)]:
                lines, touched = tx.query(data, index, name, beg, end, table)
                assert lines == tx.overlapping(text, name, beg, end), (path, name, beg, end)
                assert touched or not lines
    assert not glob.glob(os.path.join(tmp, "*.part.*"))
    # without -trackindex: the same track bytes, and no index
    out2, track2, bins2 = os.path.join(tmp, "y.txt"), os.path.join(tmp, "t2.bedgraph.gz"), os.path.join(tmp, "b2.bedgraph.gz")
    r = _cli(["-f", g["fa"], "-d", g["depth"], "-o", out2, "-np", "-track", track2, "-bintrack", bins2])
    assert r.returncode == 0, r.stderr[-3000:]
    assert open(track2, "rb").read() == open(track, "rb").read() and open(bins2, "rb").read() == open(bins, "rb").read()
    assert rows_of(out2) == rows_of(out) and not glob.glob(os.path.join(tmp, "*2.bedgraph.gz.tbi")) and ", index: " not in open(out2 + ".log").read()
    # one track as text beside an indexed one: the text track has no index, the other has
    out3, track3, bins3 = os.path.join(tmp, "z.txt"), os.path.join(tmp, "t3.bedgraph"), os.path.join(tmp, "b3.bedgraph.gz")
    r = _cli(["-f", g["fa"], "-d", g["depth"], "-o", out3, "-np", "-track", track3, "-bintrack", bins3, "-trackindex"])
    assert r.returncode == 0 and os.path.exists(bins3 + ".tbi") and not os.path.exists(track3 + ".tbi"), r.stderr[-3000:]
    assert open(bins3 + ".tbi", "rb").read() == open(bins + ".tbi", "rb").read()
