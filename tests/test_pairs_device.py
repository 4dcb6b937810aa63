"""GPU: the RP / Q0 annotation from the pair table an armed BAM load keeps in HBM.  The two debug hooks on every
case of pairs_cases against the restatement's integers; the table of a mixed BAM, in both read modes, against the table
computed from the written records; the whole path on bam_util's 12 Mb recipe against rsi_result_annotate_bam on the same
result, and the command line's rows under -pairs device against -pairs host; the two refusals; and an unarmed context, which
has no table."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import bam_util as bu
import pairs_cases as pc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "rsicnv_amd", "bin", "rsicnv")
SMALL = 65536
ARRAYS = ("pairs_pos", "pairs_rend", "pairs_mpos", "pairs_isize", "pairs_info")


@pytest.fixture(scope="module")
def hot(hotlib):
    from rsicnv_amd import api
    h = api.RsiHot(0)
    yield h
    h.close()


SAMPLE = dict(pc.sample_cases(), **pc.count_cases())
ANNOTATE = pc.annotate_cases()


@pytest.mark.parametrize("name", list(SAMPLE))
def test_sample_hook(hot, name):
    _, table, tid_len = SAMPLE[name]
    assert hot.debug_pair_sample(table, tid_len) == pc.sample_expected(table, tid_len)


@pytest.mark.parametrize("name", list(ANNOTATE))
def test_annotate_hook(hot, name):
    _, table, calls, mean, sd = ANNOTATE[name]
    rp, qa, qq = hot.debug_pair_annotate(table, [c[0] for c in calls], [c[1] for c in calls], [c[2] for c in calls], mean, sd)
    assert list(zip(rp.tolist(), qa.tolist(), qq.tolist())) == pc.annotate_expected(table, calls, mean, sd)


def test_annotate_hook_refuses_an_unsorted_table(hot):
    from rsicnv_amd import api
    _, table, calls, mean, sd = ANNOTATE["whole_table"]
    swapped = tuple(np.concatenate([a[1:2], a[0:1], a[2:]]) for a in table)
    with pytest.raises(api.RsiError) as e:
        hot.debug_pair_annotate(swapped, [calls[0][0]], [calls[0][1]], [0], mean, sd)
    assert api.STATUS_NAMES[e.value.code] == "RSI_ERR_UNSUPPORTED" and "not sorted" in str(e.value)


def armed_table(hot, bam, chrom, mode, chunk=0):
    hot.set_bam_read(mode, chunk_bytes=chunk)
    hot.set_bam_pairs(True)
    try:
        hot.load_depth_bam(bam, chrom)
        return tuple(hot.fetch(a).copy() for a in ARRAYS), hot.pairs_stats()
    finally:
        hot.set_bam_read("host")
        hot.set_bam_pairs(False)


def test_table(hot, tmp_path):
    """About 3000 records of chrS with mixed CIGARs, unmapped-with-tid reads, secondaries and duplicates (bam_util.synth_reads), mates
    on this, another and no chromosome; BGZF blocks cut at 4093 bytes, so records straddle every seam of the 64 KiB chunks."""
    rng = np.random.default_rng(0x7AB1E)
    refs = [("chrA", 50_000), ("chrS", 37_001), ("chrT", 9_000)]
    recs = []
    for t, (_, n) in enumerate(refs):
        for r in bu.synth_reads(n, coverage=8.0, seed=0x51 + t):
            b = bytearray(r)
            b[4:8] = struct.pack("<i", t)
            b[24:36] = struct.pack("<iii", int(rng.choice([-1, 0, 1, 1, 1, 2])), int(rng.integers(-1, n)), int(rng.integers(-70000, 70000)))
            recs.append(bytes(b))
    bam = str(tmp_path / "mixed.bam")
    bu.write_bam(bam, refs, recs, block=4093, straddle=True)
    want = pc.table_from_bytes(recs, 1)
    assert 2500 < len(want[0]) < 3500 and len({int(v) >> 24 & 3 for v in want[4]}) == 3
    tables = {}
    for mode in ("host", "device"):
        got, st = armed_table(hot, bam, "chrS", mode, SMALL)
        for name, g, w in zip(ARRAYS, got, want):
            assert np.array_equal(g.astype(np.int64) & 0xffffffff, w & 0xffffffff), (mode, name)
        assert st["records"] == len(want[0]) and st["table_bytes"] == 20 * len(want[0]) and st["maxspan"] == int(np.max(want[1] - want[0]))
        tables[mode] = got
    assert hot.bam_read_stats()["mode"] == "device" and hot.bam_read_stats()["chunks"] >= 2
    assert all(np.array_equal(a, b) for a, b in zip(tables["host"], tables["device"]))


@pytest.fixture(scope="module")
def config1(hotlib, tmp_path_factory):
    """bam_util's 12 Mb recipe (test_bam_depth.test_bam_12mb_rows_against_reference_binary): soft-clipped reads, mapq-0 reads and
    discordant pairs around the events, the sample window at 10 Mb populated."""
    from conftest import make_case
    from test_genome_text import write_fasta
    tmp = str(tmp_path_factory.mktemp("config1"))
    n = 12_000_017
    plan, fasta, depth = make_case(hotlib, dict(n=n, seed=0x5EED0001, model=0, mean=14.0, n_events=5, gaps=1, max_len=20000, end_n=10000, gap_len=30000))
    recs = bu.paired_reads_following_depth(depth, n, seed=11, events=plan["events"], clipped=0.3, q0=0.05)
    bam = os.path.join(tmp, "c1.bam")
    bu.write_bam(bam, [("chrS", n)], recs)
    pc.write_bai(bam, recs, 1)
    write_fasta(os.path.join(tmp, "ref.fa"), [("chrS", fasta)])
    return tmp, bam, fasta


@pytest.mark.parametrize("mode", ["host", "device"])
def test_whole_path_against_the_host_annotation(hot, config1, mode):
    from rsicnv_amd import api
    _, bam, fasta = config1
    hot.set_bam_read(mode)
    hot.set_bam_pairs(True)
    try:
        res = hot.run_bam(api.make_params(), bam, "chrS", fasta)
        assert all(p == (-1, -1.0) for p in res.pairs())
        hot.annotate_device(res)
        dev, dev_rows = res.pairs(), res.format_rows("chrS")
        st = hot.pairs_stats()
        res.annotate_bam(bam, "chrS")
        host, host_rows = res.pairs(), res.format_rows("chrS")
    finally:
        hot.set_bam_read("host")
        hot.set_bam_pairs(False)
    assert len(dev) >= 2 and dev == host and dev_rows == host_rows         # ints, and doubles bit for bit
    assert any(rp > 0 for rp, _ in dev) and any(q0 > 0 for _, q0 in dev), "vacuous: no supporting pair, or no mapq-0 read, in any call"
    assert st["records"] == res.bam_stats["on_chrom"] and st["calls"] == len(dev) and st["examined"] > 0
    assert st["sample_count"] > 2 and st["isize"] > 0 and st["isize_sd"] > 0 and st["sample_stop"] >= st["sample_count"] - 1


def cli(tmp, tag, bam, extra, chrom="chrS"):
    r = subprocess.run([EXE, "rsi", "-b", bam, "-f", "ref.fa", "-c", chrom, "-o", tag + ".txt", "-np"] + extra, cwd=tmp, capture_output=True, text=True,
                       timeout=600)
    out = os.path.join(tmp, tag + ".txt")
    return r, (open(out).read() if os.path.exists(out) else ""), (open(out + ".log").read() if os.path.exists(out + ".log") else "")


def data_rows(text):
    return [ln for ln in text.splitlines() if not ln.startswith("#")]


def test_command_line_rows(config1):
    tmp, bam, _ = config1
    rh, host, hlog = cli(tmp, "host", bam, [])
    assert rh.returncode == 0 and "#pairs:" not in hlog, rh.stderr[-2000:]               # unarmed: no line, and the default is host
    rows = data_rows(host)
    assert len(rows) >= 2 and any(not r.split("\t")[7].startswith("RP=0;") for r in rows) and any(not r.split("\t")[7].endswith("Q0=0") for r in rows)
    for tag, extra in (("dev_host", ["-pairs", "device"]), ("dev_dev", ["-pairs", "device", "-bamread", "device"])):
        r, dev, log = cli(tmp, tag, bam, extra)
        assert r.returncode == 0, r.stderr[-2000:]
        assert dev.replace(tag + ".txt", "host.txt") == host, tag
        assert log.count("#pairs: ") == 1 and "annotation failed" not in log
    rx, explicit, xlog = cli(tmp, "explicit", bam, ["-pairs", "host"])
    assert rx.returncode == 0 and explicit.replace("explicit.txt", "host.txt") == host and "#pairs:" not in xlog
    r, _, _ = cli(tmp, "bad", bam, ["-pairs", "gpu"])
    assert r.returncode != 0 and "device or host" in r.stderr and not os.path.exists(os.path.join(tmp, "bad.txt"))
    u = subprocess.run([EXE], capture_output=True, text=True, timeout=60)
    assert "-pairs device|host" in u.stderr + u.stdout


def test_command_line_all_chromosomes_in_pools(hotlib, tmp_path):
    """Without -c, and with -gpus 2 -workers 2 (both logical devices on the one GPU): every worker's context is armed, each
    chromosome is annotated from the table of its own load."""
    from conftest import make_case
    from test_genome_text import write_fasta
    tmp = str(tmp_path)
    bam, refs, recs = bu.build_golden_bam(tmp)
    pc.write_bai(bam, recs, len(refs))
    write_fasta(os.path.join(tmp, "ref.fa"), [(chrom, make_case(hotlib, dict(n=n, seed=0xFA + n, model=0, n_events=1, gaps=0, max_len=3000, end_n=1000))[1])
                                              for chrom, n in refs])
    two = dict(os.environ, RSI_HOT_DEVICE_MAP="0,0")
    outs = {}
    for tag, extra, env in (("host", [], None), ("dev", ["-pairs", "device"], None), ("pool", ["-pairs", "device", "-gpus", "2", "-workers", "2"], two),
                            ("pool_dev", ["-pairs", "device", "-bamread", "device", "-gpus", "2", "-workers", "2"], two)):
        r = subprocess.run([EXE, "rsi", "-b", bam, "-f", "ref.fa", "-o", tag + ".txt", "-np"] + extra, cwd=tmp, capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0, (tag, r.stderr[-2000:])
        outs[tag] = open(os.path.join(tmp, tag + ".txt")).read().replace(tag + ".txt", "OUT")
        log = open(os.path.join(tmp, tag + ".txt.log")).read()
        assert log.count("#pairs: ") == (0 if tag == "host" else len(refs)) and "annotation failed" not in log
    assert outs["dev"] == outs["host"] and outs["pool"] == outs["host"] and outs["pool_dev"] == outs["host"]


def test_refusals_from_the_command_line(hotlib, tmp_path):
    """A BAM whose positions go back once, and one with a record whose CIGAR count overruns its block_size: the annotation is
    refused, the log says why, and the rows carry -1 / -1 as after a failed host pass."""
    from conftest import make_case
    from test_genome_text import write_fasta
    tmp = str(tmp_path)
    n = 1_000_003
    _, fasta, depth = make_case(hotlib, dict(n=n, seed=0xBA5, model=0, n_events=6, gaps=1, max_len=30000, end_n=8000, gap_len=20000))
    write_fasta(os.path.join(tmp, "ref.fa"), [("chrS", fasta)])
    recs = bu.paired_reads_following_depth(depth, n)
    k = len(recs) // 2
    assert recs[k][8:12] != recs[k + 1][8:12] or recs[k + 2][8:12] != recs[k + 1][8:12]
    unsorted = recs[:k] + [recs[k + 2], recs[k + 1], recs[k]] + recs[k + 3:]
    many_cig = bytearray(recs[k]); many_cig[16:18] = struct.pack("<H", 60000)
    overrun = recs[:k] + [bytes(many_cig)] + recs[k + 1:]
    for tag, records, words in (("unsorted", unsorted, "BAM not sorted by position"), ("overrun", overrun, "malformed BAM record (name / CIGAR overrun the record)")):
        bam = os.path.join(tmp, tag + ".bam")
        bu.write_bam(bam, [("chrS", n)], records)
        r, text, log = cli(tmp, tag, bam, ["-pairs", "device"])
        assert r.returncode == 0, r.stderr[-2000:]
        assert "RP / Q0 annotation failed: " + words in log, log[-1500:]
        rows = data_rows(text)
        assert rows and all(row.split("\t")[7] == "RP=-1;Q0=-1" for row in rows)


def test_unarmed(hot, tmp_path):
    from rsicnv_amd import api
    from conftest import make_case
    bam, refs, _ = bu.build_golden_bam(str(tmp_path))
    chrom, n = refs[1]
    _, fasta, _ = make_case(api.load_library(), dict(n=n, seed=0xFA + n, model=0, n_events=1, gaps=0, max_len=3000, end_n=1000))
    res = hot.run_bam(api.make_params(), bam, chrom, fasta)
    st = hot.pairs_stats()
    assert st["records"] == 0 and st["table_bytes"] == 0
    with pytest.raises(KeyError):
        hot.fetch("pairs_pos")
    with pytest.raises(api.RsiError) as e:
        hot.annotate_device(res)
    assert api.STATUS_NAMES[e.value.code] == "RSI_ERR_BAD_ARG" and "not armed" in str(e.value)
    # an armed load of another chromosome does not serve this result either
    hot.set_bam_pairs(True)
    try:
        hot.load_depth_bam(bam, refs[0][0])
        assert hot.pairs_stats()["records"] > 0
        with pytest.raises(api.RsiError):
            hot.annotate_device(res)
    finally:
        hot.set_bam_pairs(False)
    hot.load_depth_bam(bam, chrom)                                       # the next load, unarmed, drops the table
    assert hot.pairs_stats()["records"] == 0


def test_abi(hotlib):
    from rsicnv_amd import api
    hdr = open(os.path.join(ROOT, "include", "rsi_hot.h")).read()
    for sym in ("rsi_hot_set_bam_pairs", "rsi_result_annotate_device", "rsi_hot_last_pairs_stats", "rsi_hot_debug_pair_sample",
                "rsi_hot_debug_pair_annotate"):
        assert re.search(r"\b" + sym + r"\(", hdr) and sym in api.EXPORTS and hasattr(hotlib, sym)
    body = re.search(r"typedef struct rsi_pairs_stats \{(.*?)\} rsi_pairs_stats;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    size = 0
    for decl in body.split(";"):
        t = decl.split()
        if t:
            size += {"int32_t": 4, "int64_t": 8, "double": 8}[t[0]] * (decl.count(",") + 1)
    assert C.sizeof(api.RsiPairsStats) == size == 7 * 8 + 2 * 4 + 2 * 8 + 3 * 8
