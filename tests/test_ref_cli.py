"""GPU: the command line with the reference read on the device.  `-f ref.fa` (read_fasta's host loop, the default for plain
text) against `-f ref.fa -refread device` and `-f ref.fa.gz` (BGZF, with a .gzi, without one, with -refindex): the output file
and the log's rows are the same byte for byte with every kind of input; the device runs log exactly one "#reference:" line,
the default text run none; what cannot work exits non-zero and says why."""
import os
import shutil
import subprocess

import pytest

import bam_util as bu
from bgzf_util import bgzf, gzip_members
from conftest import make_case
from test_genome_text import EXE, cli_case, write_fasta
from test_ref_host import gzi_of

pytestmark = pytest.mark.gpu

VOLATILE = ("timing:", "#reference:", "#command:", "#reffile:", "track:", "bintrack:")


def run(cwd, args, env=None):
    return subprocess.run([EXE, "rsi"] + args, cwd=cwd, capture_output=True, text=True, timeout=600, env=env)


def log_rows(path):
    return [l for l in open(path).read().splitlines() if not l.startswith(VOLATILE)]


def pack_reference(folder, gzi=True):
    """ref.fa of `folder` as BGZF beside it: ref.fa.gz, its .fai (the text's: offsets are text offsets) and, with gzi, its .gzi."""
    data = bgzf(open(os.path.join(folder, "ref.fa"), "rb").read())
    with open(os.path.join(folder, "ref.fa.gz"), "wb") as f:
        f.write(data)
    shutil.copy(os.path.join(folder, "ref.fa.fai"), os.path.join(folder, "ref.fa.gz.fai"))
    if gzi:
        with open(os.path.join(folder, "ref.fa.gz.gzi"), "wb") as f:
            f.write(gzi_of(data)[0])


@pytest.fixture(scope="module")
def case(hotlib, tmp_path_factory):
    """Three chromosomes of 300 to 400 kb with calls: the whole-genome depth file, its per-chromosome slices, a two-column
    cohort made of it, the reference as text and as BGZF."""
    tmp = str(tmp_path_factory.mktemp("refcli"))
    fa, genome, slices = cli_case(hotlib, tmp)
    pack_reference(tmp)
    with open(genome) as f, open(os.path.join(tmp, "cohort.depth"), "w") as out:
        for line in f:
            t = line.split()
            out.write(f"{t[0]}\t{t[1]}\t{t[2]}\t{2 * int(t[2])}\n" if len(t) == 3 and not line.startswith("#") else line)
    with open(os.path.join(tmp, "mask.bed"), "w") as f:
        f.write("chrP\t100000\t130000\nQ\t5\t10\nchrR\t20000\t21000\n")
    return tmp, slices


def three_ways(tmp, args, outs=("out.txt",), gz_extra=(), row_logs=("out.txt.log",)):
    """The run with -f ref.fa, with -refread device and with -f ref.fa.gz: every file of `outs` and the rows of every log of
    `row_logs` equal the first run's; returns the three main logs."""
    logs, want = [], None
    for tag, ref in (("host", ["-f", "ref.fa"]), ("device", ["-f", "ref.fa", "-refread", "device"]), ("bgzf", ["-f", "ref.fa.gz"] + list(gz_extra))):
        for o in outs:
            if os.path.exists(os.path.join(tmp, o)):
                os.remove(os.path.join(tmp, o))
        r = run(tmp, ref + args + ["-o", "out.txt", "-np"])
        assert r.returncode == 0, (tag, r.stderr[-3000:])
        got = {o: open(os.path.join(tmp, o), "rb").read() for o in outs}
        rows = [log_rows(os.path.join(tmp, l)) for l in row_logs]
        if want is None:
            want = (got, rows)
            assert any(not l.startswith(b"#") for l in got[outs[0]].splitlines()), "no call at all: the case checks nothing"
        assert got == want[0], tag
        assert rows == want[1], tag
        logs.append(open(os.path.join(tmp, "out.txt.log")).read())
    assert logs[0].count("#reference:") == 0
    assert logs[1].count("#reference: text, ") == 1 and logs[1].count("#reference:") == 1
    assert logs[2].count("#reference: BGZF, ") == 1 and logs[2].count("#reference:") == 1
    return logs


def test_one_chromosome_depth_file(case):
    tmp, slices = case
    name, sl = slices[0]
    logs = three_ways(tmp, ["-d", os.path.basename(sl), "-c", name])
    assert "index ref.fa.gz.gzi, 1 sequences" in logs[2]
    line = [l for l in logs[2].splitlines() if l.startswith("#reference:")][0]
    assert "compressed bytes read" in line and "members inflated" in line


def test_whole_genome_depth_file(case):
    tmp, _ = case
    logs = three_ways(tmp, ["-d", "genome.depth"], gz_extra=["-refindex", "none"])
    assert "members walked, 3 sequences" in logs[2]
    assert ", 3 sequences" in logs[1]


def test_cohort_samples(case):
    tmp, _ = case
    logs = three_ways(tmp, ["-d", "cohort.depth", "-samples", "all"], outs=("out.txt.1", "out.txt.2"),
                      row_logs=("out.txt.log", "out.txt.1.log", "out.txt.2.log"))
    assert ", 3 sequences" in logs[2]          # once per chromosome, not once per sample


def test_exclude_and_bin_track(case):
    tmp, _ = case
    shutil.copy(os.path.join(tmp, "ref.fa.gz.gzi"), os.path.join(tmp, "named.gzi"))
    three_ways(tmp, ["-d", "genome.depth", "-x", "mask.bed", "-bintrack", "bins.bedgraph"], outs=("out.txt", "bins.bedgraph"),
               gz_extra=["-refindex", "named.gzi"])


def test_bam(hotlib, tmp_path):
    tmp = str(tmp_path)
    bam, refs, _ = bu.build_golden_bam(tmp)
    seqs = [(chrom, make_case(hotlib, dict(n=n, seed=0xFA + n, model=0, n_events=1, gaps=0, max_len=3000, end_n=1000))[1]) for chrom, n in refs]
    write_fasta(os.path.join(tmp, "ref.fa"), seqs)
    pack_reference(tmp, gzi=False)
    b = os.path.basename(bam)
    logs, want = [], None
    for tag, extra, env in (("host", ["-f", "ref.fa"], None), ("device", ["-f", "ref.fa", "-refread", "device"], None), ("bgzf", ["-f", "ref.fa.gz"], None),
                            ("one", ["-f", "ref.fa.gz", "-c", refs[1][0]], None),
                            ("two_devices", ["-f", "ref.fa.gz", "-gpus", "2", "-workers", "2"], dict(os.environ, RSI_HOT_DEVICE_MAP="0,0"))):
        r = run(tmp, extra + ["-b", b, "-o", f"{tag}.txt", "-np"], env=env)
        assert r.returncode == 0, (tag, r.stderr[-3000:])
        logs.append(open(os.path.join(tmp, f"{tag}.txt.log")).read())
        if tag == "one":
            continue
        got = open(os.path.join(tmp, f"{tag}.txt")).read()
        rows = [l.replace(f"{tag}.txt", "OUT") for l in log_rows(os.path.join(tmp, f"{tag}.txt.log")) if not l.startswith("#output:")]
        if want is None:
            want = (got, rows)
        assert got == want[0], tag
        if tag != "two_devices":           # (the pools' log blocks are the same; stderr's "over 2 device(s)" line is not in the log)
            assert rows == want[1], tag
    assert [l.count("#reference:") for l in logs] == [0, 1, 1, 1, 1]
    assert "members walked, 2 sequences" in logs[2] and "members walked, 1 sequences" in logs[3] and "members walked, 2 sequences" in logs[4]
    want_one = run(tmp, ["-f", "ref.fa", "-c", refs[1][0], "-b", b, "-o", "one_host.txt", "-np"])
    assert want_one.returncode == 0
    assert open(os.path.join(tmp, "one.txt")).read() == open(os.path.join(tmp, "one_host.txt")).read()


def test_refusals(case, tmp_path):
    tmp, slices = case
    name, sl = slices[0]
    args = ["-d", os.path.basename(sl), "-c", name, "-o", "refused.txt", "-np"]
    r = run(tmp, ["-f", "ref.fa.gz", "-refread", "host"] + args)
    assert r.returncode != 0 and "-refread host" in r.stderr and "BGZF" in r.stderr
    r = run(tmp, ["-f", "ref.fa", "-refread", "gpu"] + args)
    assert r.returncode != 0 and "expected device or host" in r.stderr
    r = run(tmp, ["-f", "ref.fa", "-refindex", "ref.fa.gz.gzi"] + args)
    assert r.returncode != 0 and "-refindex" in r.stderr
    r = run(tmp, ["-f", "ref.fa.gz", "-refindex", "nowhere.gzi"] + args)
    assert r.returncode != 0 and "nowhere.gzi" in r.stderr
    plain = os.path.join(tmp, "plain.fa.gz")
    with open(plain, "wb") as f:
        f.write(gzip_members(open(os.path.join(tmp, "ref.fa"), "rb").read()))
    shutil.copy(os.path.join(tmp, "ref.fa.fai"), plain + ".fai")
    for extra in ([], ["-refread", "host"], ["-refread", "device"]):
        r = run(tmp, ["-f", "plain.fa.gz"] + extra + args)
        assert r.returncode != 0 and "bgzip" in r.stderr, r.stderr[-2000:]
    assert not os.path.exists(os.path.join(tmp, "refused.txt"))
    # a .fai that does not fit the file: the run stops with the sequence's name, and no rows
    lines = open(os.path.join(tmp, "ref.fa.fai")).read().splitlines()
    bad = [l.split("\t") for l in lines]
    for row in bad:
        row[2] = str(int(row[2]) - 1)
    shutil.copy(os.path.join(tmp, "ref.fa"), tmp_path / "bad.fa")
    (tmp_path / "bad.fa.fai").write_text("".join("\t".join(row) + "\n" for row in bad))
    r = run(tmp, ["-f", str(tmp_path / "bad.fa"), "-refread", "device"] + args)
    assert f"reference {name}" in r.stderr and "does not fit" in r.stderr, r.stderr[-2000:]
    assert not os.path.exists(os.path.join(tmp, "refused.txt"))


def test_usage_names_the_options():
    u = subprocess.run([EXE], capture_output=True, text=True)
    assert "-refread device|host" in u.stderr and "-refindex PATH|none" in u.stderr
