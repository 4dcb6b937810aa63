"""The depth track through the public interfaces: RsiHot.write_track after a run, and `rsicnv rsi ... -track FILE` with every
kind of input -- byte for byte against the numpy restatement (tests/track_restatement.py) of the depth the run read, and read
back in as bedGraph input."""
import ctypes as C
import glob
import os
import subprocess

import numpy as np
import pytest

import bam_util as bu
import track_restatement as tr
from conftest import make_case
from test_cohort_depth import sample_depths
from test_genome_text import EXE, cli_case, rows_of, write_fasta
from test_hot_extra import _write_case

BAD_ARG = -2
CASE = dict(n=400_007, seed=0xC11, model=1, n_events=5, gaps=1, max_len=20000, end_n=5000, gap_len=8000)


def _cli(args, timeout=600):
    return subprocess.run([EXE, "rsi"] + args, capture_output=True, text=True, timeout=timeout)


def parsed_depth(path, n):
    """A "pos depth" file as the library's text reader stores it."""
    from rsicnv_amd import api
    h = api.RsiHot(0)
    h.load_depth_text(path, n)
    d = h.fetch("depth_in")
    h.close()
    return d


@pytest.fixture(scope="module")
def text_case(hotlib, tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("track"))
    _, fasta, depth = make_case(hotlib, CASE)
    fa, rd = _write_case(tmp, fasta, depth)
    return tmp, fa, rd, fasta, depth


# ---- refusals: before any output file or device work ----

@pytest.mark.parametrize("args,msg", [
    (["-track", "T", "-gpus", "2"], "-gpus"),
    (["-track", "T", "-trackdepth", "gc", "-NOGC"], "-NOGC"),
    (["-track", "T", "-trackdepth", "capped"], "raw or gc"),
])
def test_track_refusals(tmp_path, args, msg):
    d = tmp_path / "d.txt"
    d.write_text("1\t30\n2\t31\n")
    out, track = str(tmp_path / "o.txt"), str(tmp_path / "t.bedgraph")
    args = [track if a == "T" else a for a in args]
    r = _cli(["-f", str(tmp_path / "ref.fa"), "-d", str(d), "-c", "chrS", "-o", out, "-np"] + args)
    assert r.returncode != 0 and msg in r.stderr, r.stderr[-2000:]
    assert sorted(os.listdir(tmp_path)) == ["d.txt"]


def test_track_in_the_usage():
    u = subprocess.run([EXE], capture_output=True, text=True)
    assert "-track FILE" in u.stderr and "-trackdepth raw|gc" in u.stderr
    assert "rsicnv rsi <options> [-b BAMFILE | -d RDFILE -c RNAME ] -f REFFILE" in u.stderr


def test_track_writer_in_the_abi(hotlib):
    from rsicnv_amd import api
    for sym in ("rsi_hot_write_track", "rsi_hot_write_track_device", "rsi_hot_debug_track"):
        assert sym in api.EXPORTS and hasattr(hotlib, sym)
    assert C.sizeof(api.RsiTrackStats) == 7 * 8


# ---- RsiHot.write_track ----

@pytest.mark.gpu
def test_write_track_after_a_text_run(text_case):
    from rsicnv_amd import api
    tmp, fa, rd, fasta, depth = text_case
    h = api.RsiHot(0)
    with pytest.raises(api.RsiError) as ei:               # nothing has run on this context yet
        h.write_track(0, "chrS", os.path.join(tmp, "none.bedgraph"))
    assert ei.value.code == BAD_ARG
    h.run_text(api.make_params(), rd, fasta)
    raw, gc = os.path.join(tmp, "raw.bedgraph"), os.path.join(tmp, "gc.bedgraph")
    st = h.write_track(0, "chrS", raw)
    exp = tr.text(h.fetch("depth_in"), "chrS")
    assert open(raw, "rb").read() == exp
    assert st["n"] == depth.size and st["lines"] == exp.count(b"\n") and st["bytes"] == len(exp) and st["slices"] == 1
    h.write_track("gc", "chrS", gc)
    rd_gc = h.fetch("rd_gc")
    assert open(gc, "rb").read() == tr.text(rd_gc, "chrS")
    assert not np.array_equal(rd_gc, h.fetch("depth_in"))
    # append: the text twice; without: replaced
    h.write_track(0, "chrS", gc, append=True)
    h.write_track(0, "chrS", gc, append=True)
    assert open(gc, "rb").read() == tr.text(rd_gc, "chrS") + exp + exp
    h.write_track(0, "chrS", gc)
    assert open(gc, "rb").read() == exp
    # a directory in the way: write() never happens, the error names the file
    with pytest.raises(api.RsiError) as ei:
        h.write_track(0, "chrS", os.path.join(tmp, "no_such_dir", "t.bedgraph"))
    assert ei.value.code == -6 and "no_such_dir" in str(ei.value)
    # -NOGC leaves no GC-adjusted depth
    h.run_text(api.make_params(gcadjust=0), rd, fasta)
    with pytest.raises(api.RsiError) as ei:
        h.write_track(1, "chrS", gc)
    assert ei.value.code == BAD_ARG
    h.write_track(0, "chrS", raw)
    assert open(raw, "rb").read() == exp
    h.close()


@pytest.mark.gpu
def test_write_track_device_of_any_array():
    import torch
    from rsicnv_amd import api
    import tempfile
    v = (np.arange(70_001) // 7 % 5 - 2).astype(np.int32)
    d = torch.from_numpy(v).to("cuda:0")
    torch.cuda.synchronize()
    h = api.RsiHot(0)
    with tempfile.TemporaryDirectory() as tmp:
        p = os.path.join(tmp, "v.bedgraph")
        st = h.write_track_device(d.data_ptr(), v.size, "any", p)
        assert open(p, "rb").read() == tr.text(v, "any") and st["lines"] == 10_001
        h.write_track_device(0, 0, "any", p)                  # n == 0: nothing
        assert open(p, "rb").read() == b""
    h.close()


# ---- the command line ----

@pytest.mark.gpu
def test_cli_one_chromosome_and_round_trip(text_case):
    tmp, fa, rd, fasta, depth = text_case
    out, track = os.path.join(tmp, "one.txt"), os.path.join(tmp, "t.bedgraph")
    r = _cli(["-f", fa, "-d", rd, "-c", "chrS", "-o", out, "-np", "-track", track])
    assert r.returncode == 0, r.stderr[-3000:]
    d = parsed_depth(rd, depth.size)
    assert open(track, "rb").read() == tr.text(d, "chrS")
    assert not glob.glob(track + ".part.*")
    assert any(l.startswith("track: chrS ") and " lines, " in l and " bytes, " in l for l in open(out + ".log"))
    assert rows_of(out)
    # The text reader never stores the last base (it stops at the first pos >= n), so the raw depth the run read -- and the
    # track holds -- already ends in 0: the bedGraph reader, which drops the last base of the track's last run likewise, rebuilds
    # that array exactly and the rows are the same bytes.
    assert d[-1] == 0
    back = os.path.join(tmp, "back.txt")
    r = _cli(["-f", fa, "-d", track, "-c", "chrS", "-o", back, "-np"])
    assert r.returncode == 0, r.stderr[-3000:]
    assert rows_of(back) == rows_of(out)
    # -trackdepth gc: another array (checked against rd_gc in test_write_track_after_a_text_run), the same rows
    out_gc, track_gc = os.path.join(tmp, "one_gc.txt"), os.path.join(tmp, "t_gc.bedgraph")
    r = _cli(["-f", fa, "-d", rd, "-c", "chrS", "-o", out_gc, "-np", "-track", track_gc, "-trackdepth", "gc"])
    assert r.returncode == 0, r.stderr[-3000:]
    assert rows_of(out_gc) == rows_of(out)
    gc = open(track_gc, "rb").read()
    assert gc != open(track, "rb").read() and tr.expand(gc, "chrS", depth.size).size == depth.size


@pytest.mark.gpu
def test_cli_whole_genome_three_workers(hotlib, tmp_path):
    tmp = str(tmp_path)
    fa, genome, slices = cli_case(hotlib, tmp)
    lens = {l.split("\t")[0]: int(l.split("\t")[1]) for l in open(fa + ".fai")}
    out, track = os.path.join(tmp, "g.txt"), os.path.join(tmp, "g.bedgraph")
    r = _cli(["-f", fa, "-d", genome, "-o", out, "-np", "-workers", "3", "-track", track])
    assert r.returncode == 0, r.stderr[-3000:]
    exp = b"".join(tr.text(parsed_depth(sl, lens[name]), name) for name, sl in slices)   # the file's order, chrMT skipped
    got = open(track, "rb").read()
    assert got == exp
    assert not glob.glob(os.path.join(tmp, "*.part.*"))
    assert len(rows_of(out)) >= 3
    back = os.path.join(tmp, "back.txt")
    r = _cli(["-f", fa, "-d", track, "-o", back, "-np", "-workers", "3"])
    assert r.returncode == 0, r.stderr[-3000:]
    assert rows_of(back) == rows_of(out)


@pytest.mark.gpu
def test_cli_samples_one_track_per_column(hotlib, tmp_path):
    from rsicnv_amd import api
    lib = api.load_library()
    tmp = str(tmp_path)
    cohort = os.path.join(tmp, "cohort.depth")
    seqs, cols = [], {}
    for name, n, seed in (("chrA", 200_003, 0x7A01), ("chrB", 150_001, 0x7A02)):
        fasta, depths = sample_depths(hotlib, n, [seed, seed + 16])
        depths = np.ascontiguousarray(depths, dtype=np.int32)
        assert lib.rsi_synth_append_genome_samples(cohort.encode(), name.encode(), depths.ctypes.data, 2, n, 0) == 0
        seqs.append((name, fasta))
        cols[name] = depths
    fa = os.path.join(tmp, "ref.fa")
    write_fasta(fa, seqs)
    out, track = os.path.join(tmp, "c.txt"), os.path.join(tmp, "c.bedgraph")
    r = _cli(["-f", fa, "-d", cohort, "-o", out, "-np", "-samples", "all", "-track", track])
    assert r.returncode == 0, r.stderr[-3000:]
    for k in (1, 2):
        exp = b""
        for name, _ in seqs:
            d = cols[name][k - 1].copy()
            d[-1] = 0                                         # the reader never stores the last base
            exp += tr.text(d, name)
        assert open(f"{track}.{k}", "rb").read() == exp, k
        assert os.path.exists(f"{out}.{k}")
    assert not os.path.exists(track) and not glob.glob(os.path.join(tmp, "*.part.*"))


@pytest.mark.gpu
def test_cli_bam_track_beside_the_rd_dump(hotlib, tmp_path):
    tmp = str(tmp_path)
    bam, refs, _ = bu.build_golden_bam(tmp)
    seqs = [(chrom, make_case(hotlib, dict(n=n, seed=0xFA + n, model=0, n_events=1, gaps=0, max_len=3000, end_n=1000))[1]) for chrom, n in refs]
    fa = os.path.join(tmp, "ref.fa")
    write_fasta(fa, seqs)
    n = dict(refs)["chrS"]
    plain, out, track = os.path.join(tmp, "plain.txt"), os.path.join(tmp, "with.txt"), os.path.join(tmp, "t.bedgraph")
    r = _cli(["-b", bam, "-f", fa, "-c", "chrS", "-o", plain, "-np", "-s"])
    assert r.returncode == 0 and os.path.exists(plain + ".chrS_rd"), r.stderr[-3000:]
    r = _cli(["-b", bam, "-f", fa, "-c", "chrS", "-o", out, "-np", "-s", "-track", track])
    assert r.returncode == 0, r.stderr[-3000:]
    dump = open(out + ".chrS_rd", "rb").read()
    assert dump == open(plain + ".chrS_rd", "rb").read()      # plain -s: its file and its bytes as before
    rd = np.loadtxt(out + ".chrS_rd", dtype=np.int64)
    assert np.array_equal(rd[:, 0], np.arange(1, n + 1))
    assert np.array_equal(tr.expand(open(track, "rb").read(), "chrS", n), rd[:, 1])
    assert open(track, "rb").read() == tr.text(rd[:, 1], "chrS")
    assert rows_of(out) == rows_of(plain)
