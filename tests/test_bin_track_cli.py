"""The per-bin track through the public interfaces: RsiHot.write_bin_track after a run, and `rsicnv rsi ... -bintrack FILE` with
every kind of input -- byte for byte against the restatement (tests/bin_track_restatement.py) fed with the run's own bin
medians, removed regions, chromosome median and bin size (the parity tests compare those with the oracle)."""
import glob
import os
import subprocess

import numpy as np
import pytest

import bam_util as bu
import bin_track_restatement as bt
import track_restatement as tr
from conftest import make_case, small_cases
from test_cohort_depth import sample_depths
from test_genome_text import EXE, cli_case, rows_of, write_fasta
from test_hot_extra import _write_case

pytestmark = pytest.mark.gpu

BAD_ARG = -2
MANY600 = [(20_000 + 600 * i, 20_020 + 600 * i) for i in range(600)]   # tests/test_exclude_mask.py: more than 512 regions
CASE = dict(n=400_007, seed=0xC11, model=1, n_events=5, gaps=1, max_len=20000, end_n=5000, gap_len=8000)


def _cli(args, timeout=600):
    return subprocess.run([EXE, "rsi"] + args, capture_output=True, text=True, timeout=timeout)


@pytest.fixture(scope="module")
def hot():
    from rsicnv_amd import api
    h = api.RsiHot(0)
    yield h
    h.close()


def expected(hot, res, m, which, name):
    """The restatement's text of the run `hot` holds."""
    med2 = 2 * res.stats["RDmedian"]
    assert med2 == int(med2)
    return bt.text(hot.fetch("binmedint"), m, res.stats["n"], np.asarray(res.noncode).reshape(-1, 2), int(med2), which, name)


def expected_of(hot, depth, fasta, which, name, m=101, exclude=None):
    from rsicnv_amd import api
    res = hot.run(api.make_params(m=m), depth, fasta, exclude=exclude)
    return expected(hot, res, m, which, name), res


@pytest.fixture(scope="module")
def tail7(hotlib):
    kw = next(c[1] for c in small_cases() if c[0] == "poisson_tail7")
    _, fasta, depth = make_case(hotlib, kw)
    return fasta, depth


# ---- RsiHot.write_bin_track ----

@pytest.mark.parametrize("mask", [None, MANY600], ids=["plain", "many600"])
def test_write_bin_track_after_a_run(hot, tail7, tmp_path, mask):
    from rsicnv_amd import api
    fasta, depth = tail7
    res = hot.run(api.make_params(), depth, fasta, exclude=mask)
    assert (res.stats["n_noncode"] > 512) == (mask is not None)
    path = str(tmp_path / "b.bedgraph")
    for which, word in ((0, "median"), (1, "ratio")):
        exp = expected(hot, res, 101, which, "chrS")
        st = hot.write_bin_track(word, "chrS", path)
        got = open(path, "rb").read()
        assert got == exp
        assert st["n"] == res.stats["nbins"] and st["lines"] == exp.count(b"\n") and st["bytes"] == len(exp) and st["slices"] == 1
        assert st["lines"] >= st["n"]
        bt.check_valid(got, depth.size, np.asarray(res.noncode).reshape(-1, 2))
    med = expected(hot, res, 101, 0, "chrS")
    assert np.array_equal(bt.expand_median(med, depth.size, np.asarray(res.noncode).reshape(-1, 2)),
                          np.repeat(hot.fetch("binmedint").astype(np.int64), 101))
    if mask is None:   # append: behind what is there; without: replaced
        hot.write_bin_track(0, "chrS", path)
        hot.write_bin_track(1, "chrT", path, append=True)
        assert open(path, "rb").read() == med + expected(hot, res, 101, 1, "chrT")
        hot.write_bin_track(0, "chrS", path)
        assert open(path, "rb").read() == med


def test_write_bin_track_needs_a_successful_run(tail7, tmp_path):
    from rsicnv_amd import api
    fasta, depth = tail7
    path = str(tmp_path / "b.bedgraph")
    h = api.RsiHot(0)
    try:
        with pytest.raises(api.RsiError) as ei:             # a fresh context
            h.write_bin_track(1, "chrS", path)
        assert ei.value.code == BAD_ARG
        h.run(api.make_params(), depth, fasta)
        h.write_bin_track(1, "chrS", path)
        for bad in (dict(which=2), dict(chrom="a\tb"), dict(chrom="")):
            with pytest.raises(api.RsiError) as ei:
                h.write_bin_track(bad.get("which", 0), bad.get("chrom", "chrS"), path)
            assert ei.value.code == BAD_ARG
        with pytest.raises(api.RsiError):                   # a run that fails: too short for the GC table
            h.run(api.make_params(), depth[:1000], fasta[:1000])
        with pytest.raises(api.RsiError) as ei:
            h.write_bin_track(1, "chrS", path)
        assert ei.value.code == BAD_ARG
        h.run(api.make_params(), depth, fasta)              # and the context goes on
        h.write_bin_track(1, "chrS", path)
    finally:
        h.close()


def test_runs_without_the_call_launch_nothing_new(hot, tail7, tmp_path):
    from rsicnv_amd import api
    fasta, depth = tail7
    p = api.make_params()
    hot.set_timing(True)
    try:
        hot.run(p, depth, fasta)
        before = [k for k, _ in hot.kernel_times()]
        hot.write_bin_track(1, "chrS", str(tmp_path / "b.bedgraph"))
        hot.run(p, depth, fasta)
        after = [k for k, _ in hot.kernel_times()]
    finally:
        hot.set_timing(False)
    assert before == after and "fasta_classify" in before
    assert not [k for k in after if "track" in k]


# ---- the command line ----

@pytest.mark.parametrize("args,msg", [
    (["-bintrack", "T", "-gpus", "2"], "-gpus"),
    (["-bintrack", "T", "-bintrackvalue", "tnb"], "ratio or median"),
    (["-bintrackvalue", "tnb"], "ratio or median"),
    (["-bintrack", "OUT"], "-bintrack"),
    (["-bintrack", "DEPTH"], "-bintrack"),
    (["-bintrack", "T", "-track", "T"], "-bintrack"),
])
def test_bin_track_refusals(tmp_path, args, msg):
    d = tmp_path / "d.txt"
    d.write_text("1\t30\n2\t31\n")
    out = str(tmp_path / "o.txt")
    names = {"T": str(tmp_path / "t.bedgraph"), "OUT": out, "DEPTH": str(d)}
    args = [names.get(a, a) for a in args]
    r = _cli(["-f", str(tmp_path / "ref.fa"), "-d", str(d), "-c", "chrS", "-o", out, "-np"] + args)
    assert r.returncode != 0 and msg in r.stderr, r.stderr[-2000:]
    assert sorted(os.listdir(tmp_path)) == ["d.txt"]
    assert d.read_text() == "1\t30\n2\t31\n"


def test_refusal_for_the_bam_as_bin_track_file(tmp_path):
    bam = tmp_path / "x.bam"
    bam.write_bytes(b"not a bam")
    r = _cli(["-f", str(tmp_path / "ref.fa"), "-b", str(bam), "-o", str(tmp_path / "o.txt"), "-np", "-bintrack", str(bam)])
    assert r.returncode != 0 and "-bintrack" in r.stderr
    assert bam.read_bytes() == b"not a bam" and sorted(os.listdir(tmp_path)) == ["x.bam"]


def test_bin_track_in_the_usage():
    u = subprocess.run([EXE], capture_output=True, text=True)
    assert "-bintrack FILE" in u.stderr and "-bintrackvalue ratio|median" in u.stderr
    assert "-track FILE" in u.stderr and "-trackdepth raw|gc" in u.stderr


@pytest.fixture(scope="module")
def text_case(hotlib, tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("bintrack"))
    _, fasta, depth = make_case(hotlib, CASE)
    fa, rd = _write_case(tmp, fasta, depth)
    return tmp, fa, rd, fasta, depth


def test_cli_one_chromosome_beside_the_depth_track(hot, text_case):
    from rsicnv_amd import api
    tmp, fa, rd, fasta, depth = text_case
    plain, out = os.path.join(tmp, "plain.txt"), os.path.join(tmp, "one.txt")
    track, bins = os.path.join(tmp, "t.bedgraph"), os.path.join(tmp, "bins.bedgraph")
    r = _cli(["-f", fa, "-d", rd, "-c", "chrS", "-o", plain, "-np"])
    assert r.returncode == 0, r.stderr[-3000:]
    r = _cli(["-f", fa, "-d", rd, "-c", "chrS", "-o", out, "-np", "-bintrack", bins, "-track", track])
    assert r.returncode == 0, r.stderr[-3000:]
    assert open(out, "rb").read() == open(plain, "rb").read()          # the output file: the same bytes with and without
    res = hot.run_text(api.make_params(), rd, fasta)
    exp = expected(hot, res, 101, 1, "chrS")                           # ratio is the default
    got = open(bins, "rb").read()
    assert got == exp
    rows = bt.check_valid(got, depth.size, np.asarray(res.noncode).reshape(-1, 2))   # sorted, non-overlapping, no removed base
    assert len(rows) >= res.stats["nbins"]
    assert open(track, "rb").read() == tr.text(hot.fetch("depth_in"), "chrS")
    assert not glob.glob(os.path.join(tmp, "*.part.*"))
    log = open(out + ".log").read().splitlines()
    assert any(l.startswith("bintrack: chrS ") and " lines, " in l and " bytes, " in l and "kernels" in l and "write" in l for l in log)
    assert "bin track written to " + bins in log and "track written to " + track in log


def test_cli_median_value_and_a_mask(hot, text_case):
    from rsicnv_amd import api
    tmp, fa, rd, fasta, depth = text_case
    out, med = os.path.join(tmp, "m.txt"), os.path.join(tmp, "med.bedgraph")
    r = _cli(["-f", fa, "-d", rd, "-c", "chrS", "-o", out, "-np", "-bintrack", med, "-bintrackvalue", "median"])
    assert r.returncode == 0, r.stderr[-3000:]
    res = hot.run_text(api.make_params(), rd, fasta)
    got = open(med, "rb").read()
    assert got == expected(hot, res, 101, 0, "chrS")
    assert np.array_equal(bt.expand_median(got, depth.size, np.asarray(res.noncode).reshape(-1, 2)),   # expands back to the bins
                          np.repeat(hot.fetch("binmedint").astype(np.int64), 101))
    # -x and -m: the mask's regions cut the bins
    bed = os.path.join(tmp, "x.bed")
    with open(bed, "w") as f:
        f.writelines(f"chrS\t{s}\t{e}\n" for s, e in MANY600[:150])
    r = _cli(["-f", fa, "-d", rd, "-c", "chrS", "-o", out, "-np", "-bintrack", med, "-x", bed, "-m", "51"])
    assert r.returncode == 0, r.stderr[-3000:]
    res = hot.run_text(api.make_params(m=51), rd, fasta, exclude=MANY600[:150])
    assert res.stats["n_noncode"] > 100                                # (some of the 150 merge with the N gaps they fall into)
    got = open(med, "rb").read()
    assert got == expected(hot, res, 51, 1, "chrS")
    assert got.count(b"\n") > res.stats["nbins"]                      # some bins are cut


def test_cli_bedgraph_input(hot, text_case):
    from rsicnv_amd import api
    tmp, fa, rd, fasta, depth = text_case
    out, bg, bins = os.path.join(tmp, "bg.txt"), os.path.join(tmp, "in.bedgraph"), os.path.join(tmp, "frombg.bedgraph")
    res = hot.run_text(api.make_params(), rd, fasta)
    exp = expected(hot, res, 101, 1, "chrS")
    with open(bg, "wb") as f:
        f.write(tr.text(hot.fetch("depth_in"), "chrS"))
    r = _cli(["-f", fa, "-d", bg, "-c", "chrS", "-o", out, "-np", "-bintrack", bins])
    assert r.returncode == 0, r.stderr[-3000:]
    assert open(bins, "rb").read() == exp


def test_cli_whole_genome_three_workers(hotlib, tmp_path):
    tmp = str(tmp_path)
    fa, genome, slices = cli_case(hotlib, tmp)
    out, bins = os.path.join(tmp, "g.txt"), os.path.join(tmp, "g.ratio.bedgraph")
    r = _cli(["-f", fa, "-d", genome, "-o", out, "-np", "-workers", "3", "-bintrack", bins])
    assert r.returncode == 0, r.stderr[-3000:]
    got = open(bins, "rb").read()
    exp = b""
    for name, sl in slices:                                            # the file's order (not the .fai's), chrMT skipped
        one = os.path.join(tmp, f"one_{name}.bedgraph")
        r = _cli(["-f", fa, "-d", sl, "-c", name, "-o", os.path.join(tmp, f"one_{name}.txt"), "-np", "-bintrack", one])
        assert r.returncode == 0, r.stderr[-3000:]
        part = open(one, "rb").read()
        assert part and all(l.startswith(name.encode() + b"\t") for l in part.splitlines())
        exp += part
    assert got == exp
    assert not glob.glob(os.path.join(tmp, "*.part.*"))
    assert len(rows_of(out)) >= 3


def test_cli_samples_one_file_per_column(hot, hotlib, tmp_path):
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
    out, bins = os.path.join(tmp, "c.txt"), os.path.join(tmp, "c.bedgraph")
    r = _cli(["-f", fa, "-d", cohort, "-o", out, "-np", "-samples", "all", "-bintrack", bins, "-bintrackvalue", "median"])
    assert r.returncode == 0, r.stderr[-3000:]
    for k in (1, 2):
        exp = b""
        for name, fasta in seqs:
            d = cols[name][k - 1].copy()
            d[-1] = 0                                                  # the reader never stores the last base
            exp += expected_of(hot, d, fasta, 0, name)[0]
        assert open(f"{bins}.{k}", "rb").read() == exp, k
        assert os.path.exists(f"{out}.{k}")
    assert not os.path.exists(bins) and not glob.glob(os.path.join(tmp, "*.part.*"))


def test_cli_bam(hot, hotlib, tmp_path):
    tmp = str(tmp_path)
    bam, refs, _ = bu.build_golden_bam(tmp)
    seqs = [(chrom, make_case(hotlib, dict(n=n, seed=0xFA + n, model=0, n_events=1, gaps=0, max_len=3000, end_n=1000))[1]) for chrom, n in refs]
    fa = os.path.join(tmp, "ref.fa")
    write_fasta(fa, seqs)
    n = dict(refs)["chrS"]
    plain, out, bins = os.path.join(tmp, "plain.txt"), os.path.join(tmp, "with.txt"), os.path.join(tmp, "b.bedgraph")
    r = _cli(["-b", bam, "-f", fa, "-c", "chrS", "-o", plain, "-np"])
    assert r.returncode == 0, r.stderr[-3000:]
    r = _cli(["-b", bam, "-f", fa, "-c", "chrS", "-o", out, "-np", "-s", "-bintrack", bins])
    assert r.returncode == 0, r.stderr[-3000:]
    assert open(out, "rb").read() == open(plain, "rb").read()
    rd = np.loadtxt(out + ".chrS_rd", dtype=np.int64)
    assert rd.shape == (n, 2)
    exp, res = expected_of(hot, rd[:, 1].astype(np.int32), dict(seqs)["chrS"], 1, "chrS")
    got = open(bins, "rb").read()
    assert got == exp and got
    bt.check_valid(got, n, np.asarray(res.noncode).reshape(-1, 2))
