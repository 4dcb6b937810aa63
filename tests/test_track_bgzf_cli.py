"""`rsicnv rsi ... -track FILE.gz -bintrack FILE.gz`: BGZF tracks from the command line.  They inflate to exactly the files the
same run writes as text, end in one end-of-file block, go back in through -d (the device inflater: the round trip), follow
-trackformat whatever their names, and with -samples take the rule from FILE, not FILE.k."""
import glob
import os
import subprocess

import numpy as np
import pytest

import bgzf_walk as bw
from bgzf_util import EOF_BLOCK
from conftest import make_case
from test_cohort_depth import sample_depths
from test_genome_text import EXE, chrom_lines, render, rows_of, write_fasta


def _cli(args, timeout=600):
    return subprocess.run([EXE, "rsi"] + args, capture_output=True, text=True, timeout=timeout)


@pytest.fixture(scope="module")
def genome(hotlib, tmp_path_factory):
    """Two chromosomes in one whole-genome depth file, and the plain-text tracks of a run on it."""
    tmp = str(tmp_path_factory.mktemp("bgzf_cli"))
    specs = [("chrP", dict(n=300_007, seed=0xD21, model=1, n_events=4, gaps=1, max_len=20000, end_n=5000, gap_len=8000)),
             ("chrQ", dict(n=250_019, seed=0xD22, model=0, n_events=4, gaps=0, max_len=15000, end_n=4000))]
    lines, seqs = [], []
    for i, (name, kw) in enumerate(specs):
        _, fasta, depth = make_case(hotlib, kw)
        seqs.append((name, fasta))
        lines += chrom_lines(name, depth, fasta.size, 300 + i, quirks=False)
    fa = os.path.join(tmp, "ref.fa")
    write_fasta(fa, seqs)
    depth_file = os.path.join(tmp, "genome.depth")
    with open(depth_file, "w") as f:
        f.write(render(lines, 7))
    out, track, bins = os.path.join(tmp, "plain.txt"), os.path.join(tmp, "plain.bedgraph"), os.path.join(tmp, "plain.ratio.bedgraph")
    r = _cli(["-f", fa, "-d", depth_file, "-o", out, "-np", "-track", track, "-bintrack", bins])
    assert r.returncode == 0, r.stderr[-3000:]
    return dict(tmp=tmp, fa=fa, depth=depth_file, rows=rows_of(out), track=open(track, "rb").read(), bins=open(bins, "rb").read())


def test_trackformat_in_the_usage_and_refused_when_unknown(tmp_path):
    u = subprocess.run([EXE], capture_output=True, text=True)
    assert "-trackformat text|bgzf" in u.stderr and ".gz or .bgz" in u.stderr
    d = tmp_path / "d.txt"
    d.write_text("1\t30\n2\t31\n")
    r = _cli(["-f", str(tmp_path / "ref.fa"), "-d", str(d), "-c", "chrS", "-o", str(tmp_path / "o.txt"), "-np", "-track", str(tmp_path / "t.gz"),
              "-trackformat", "gzip"])
    assert r.returncode != 0 and "text or bgzf" in r.stderr
    assert sorted(os.listdir(tmp_path)) == ["d.txt"]


@pytest.mark.gpu
def test_gz_names_write_bgzf_and_read_back(genome):
    g = genome
    tmp = g["tmp"]
    assert g["rows"] and g["track"].count(b"\n") > 1000 and g["bins"].count(b"\n") > 1000
    out, track, bins = os.path.join(tmp, "z.txt"), os.path.join(tmp, "out.bedgraph.gz"), os.path.join(tmp, "out.ratio.bedgraph.GZ")
    r = _cli(["-f", g["fa"], "-d", g["depth"], "-o", out, "-np", "-track", track, "-bintrack", bins])
    assert r.returncode == 0, r.stderr[-3000:]
    assert rows_of(out) == g["rows"]
    for path, text in ((track, g["track"]), (bins, g["bins"])):
        data = open(path, "rb").read()
        ms = bw.check_file(data, text)                     # the same bytes of text, member by member, one end-of-file block
        assert data.count(EOF_BLOCK) == 1 and len(data) < len(text) // 2
        # a chromosome's part is whole members: chrQ's text starts a member
        assert any(m["text"].startswith(b"chrQ\t") for m in ms)
    assert not glob.glob(os.path.join(tmp, "*.part.*"))
    # the round trip: the track as depth input, inflated on the device
    back = os.path.join(tmp, "back.txt")
    r = _cli(["-f", g["fa"], "-d", track, "-o", back, "-np"])
    assert r.returncode == 0, r.stderr[-3000:]
    assert rows_of(back) == g["rows"]


@pytest.mark.gpu
def test_trackformat_overrides_the_names(genome):
    g = genome
    tmp = g["tmp"]
    out = os.path.join(tmp, "f.txt")
    track, bins = os.path.join(tmp, "as_text.bedgraph.gz"), os.path.join(tmp, "as_text.ratio.bedgraph")
    r = _cli(["-f", g["fa"], "-d", g["depth"], "-o", out, "-np", "-track", track, "-bintrack", bins, "-trackformat", "text"])
    assert r.returncode == 0, r.stderr[-3000:]
    assert open(track, "rb").read() == g["track"] and open(bins, "rb").read() == g["bins"]
    track, bins = os.path.join(tmp, "as_bgzf.bedgraph"), os.path.join(tmp, "as_bgzf.ratio.bedgraph.bgz")
    r = _cli(["-f", g["fa"], "-d", g["depth"], "-o", out, "-np", "-track", track, "-bintrack", bins, "-trackformat", "bgzf"])
    assert r.returncode == 0, r.stderr[-3000:]
    bw.check_file(open(track, "rb").read(), g["track"])
    bw.check_file(open(bins, "rb").read(), g["bins"])


@pytest.mark.gpu
def test_samples_take_the_rule_from_the_name_given(hotlib, tmp_path):
    from rsicnv_amd import api
    lib = api.load_library()
    tmp = str(tmp_path)
    cohort = os.path.join(tmp, "cohort.depth")
    seqs = []
    for name, n, seed in (("chrA", 200_003, 0x7A01), ("chrB", 150_001, 0x7A02)):
        fasta, depths = sample_depths(hotlib, n, [seed, seed + 16])
        depths = np.ascontiguousarray(depths, dtype=np.int32)
        assert lib.rsi_synth_append_genome_samples(cohort.encode(), name.encode(), depths.ctypes.data, 2, n, 0) == 0
        seqs.append((name, fasta))
    fa = os.path.join(tmp, "ref.fa")
    write_fasta(fa, seqs)
    out, plain, packed = os.path.join(tmp, "c.txt"), os.path.join(tmp, "c.bedgraph"), os.path.join(tmp, "c.bedgraph.gz")
    r = _cli(["-f", fa, "-d", cohort, "-o", out, "-np", "-samples", "1,2", "-track", plain])
    assert r.returncode == 0, r.stderr[-3000:]
    r = _cli(["-f", fa, "-d", cohort, "-o", out, "-np", "-samples", "1,2", "-track", packed])
    assert r.returncode == 0, r.stderr[-3000:]
    for k in (1, 2):
        text = open(f"{plain}.{k}", "rb").read()
        assert text.count(b"\n") > 1000
        bw.check_file(open(f"{packed}.{k}", "rb").read(), text)
    assert not os.path.exists(packed) and not glob.glob(os.path.join(tmp, "*.part.*"))
