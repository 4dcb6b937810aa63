"""GPU: a BAM read on the device (`set_bam_read("device")`) -- BGZF members inflated there, records found there by
guess / walk / stitch, the same pileup kernel -- against the host mode on the same files: the depth, and the stats that do not
describe a mode's own chunks, must be equal on every file; on the golden BAM the depth is also the reference's.  Small chunks
(65 536 bytes) put a seam and a carried record between every two members; the crafted streams of bam_walk_cases put record
starts, segment seams and look-alike bytes together.  Errors leave the context usable."""
import ctypes as C
import os
import re
import struct
import subprocess
import zlib

import numpy as np
import pytest

import bam_util as bu
import bam_walk_cases as bw

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "bam_small.npz")
EXE = os.path.join(ROOT, "rsicnv_amd", "bin", "rsicnv")
SAME = ("n", "tid", "indexed", "records", "on_chrom", "used", "runs", "malformed")
SMALL = 65536


def bgzf_blocks(raw):
    """(file offset, block size, inflated bytes) of every BGZF block of a file written by bam_util."""
    out, p = [], 0
    while p < len(raw):
        bsize = struct.unpack_from("<H", raw, p + 16)[0] + 1
        out.append((p, bsize, zlib.decompress(raw[p + 18:p + bsize - 8], -15)))
        p += bsize
    return out


def write_min_bai(bam, nref):
    """A .bai that holds what the loader takes from one: per reference one bin with one chunk that begins at the virtual offset
    of the reference's first read (no bin for a reference without reads)."""
    blocks = bgzf_blocks(open(bam, "rb").read())
    text = b"".join(b[2] for b in blocks)
    starts = np.cumsum([0] + [len(b[2]) for b in blocks])
    p = 8 + struct.unpack_from("<i", text, 4)[0]
    for _ in range(struct.unpack_from("<i", text, p)[0]):
        p += 4 + struct.unpack_from("<i", text, p + 4)[0] + 4
    p += 4
    first = {}
    while p + 8 <= len(text):
        bs, tid = struct.unpack_from("<ii", text, p)
        if tid >= 0 and tid not in first:
            k = int(np.searchsorted(starts, p, side="right")) - 1
            first[tid] = (blocks[k][0] << 16) | (p - int(starts[k]))
        p += 4 + bs
    with open(bam + ".bai", "wb") as f:
        f.write(b"BAI\1" + struct.pack("<i", nref))
        for t in range(nref):
            if t in first:
                f.write(struct.pack("<iIiQQ", 1, 4681, 1, first[t], len(open(bam, "rb").read()) << 16))
            else:
                f.write(struct.pack("<i", 0))
            f.write(struct.pack("<i", 0))
    return first


@pytest.fixture(scope="module")
def hot(hotlib):
    from rsicnv_amd import api
    h = api.RsiHot(0)
    yield h
    h.close()


def load(hot, bam, chrom, mode, chunk=0, **kw):
    hot.set_bam_read(mode, chunk_bytes=chunk)
    try:
        st = hot.load_depth_bam(bam, chrom, **kw)
        return st, hot.fetch("depth_in").copy(), hot.bam_read_stats()
    finally:
        hot.set_bam_read("host")


def same_as_host(hot, bam, chrom, chunk=0, **kw):
    """Both modes on one file: equal depth, equal stats; returns (stats, depth, read stats) of the device mode."""
    hs, hd, hr = load(hot, bam, chrom, "host", **kw)
    ds, dd, dr = load(hot, bam, chrom, "device", chunk, **kw)
    assert hr["mode"] == "host" and hr["chunks"] == 0 and dr["mode"] == "device"
    assert {k: ds[k] for k in SAME} == {k: hs[k] for k in SAME}
    assert np.array_equal(dd, hd), int(np.sum(dd != hd))
    assert dr["guessed"] + dr["rewalked"] + dr["passed"] <= dr["segments"]
    return ds, dd, dr


@pytest.fixture(scope="module")
def golden(tmp_path_factory):
    plain, indexed = str(tmp_path_factory.mktemp("plain")), str(tmp_path_factory.mktemp("indexed"))
    bam, refs, recs = bu.build_golden_bam(plain)
    bam_i, _, _ = bu.build_golden_bam(indexed)
    first = write_min_bai(bam_i, len(refs))
    assert sorted(first) == [0, 1] and first[1] & 0xffff     # chrS begins inside a block: the index start is a mid-block offset
    return {False: bam, True: bam_i}, refs, recs


@pytest.mark.parametrize("chunk", [0, SMALL])
@pytest.mark.parametrize("indexed", [False, True])
def test_golden_bam(hot, golden, indexed, chunk):
    bams, refs, recs = golden
    g = np.load(GOLDEN)
    for t, (chrom, n) in enumerate(refs):
        st, depth, rs = same_as_host(hot, bams[indexed], chrom, chunk)
        assert st["indexed"] == int(indexed) and st["n"] == n and st["tid"] == t
        assert np.array_equal(depth, g[f"{chrom}_q0_Q13"])
        if not indexed:
            assert {k: st[k] for k in ("records", "on_chrom")} == bu.walk_counts(recs, t)
        assert rs["members"] > 0 and rs["segments"] > 0 and rs["guessed"] > 0
        assert (rs["chunks"] > 10) == (chunk == SMALL)


def test_other_filters_too(hot, golden):
    bams, refs, _ = golden
    g = np.load(GOLDEN)
    for chrom, _ in refs:
        _, depth, _ = same_as_host(hot, bams[False], chrom, SMALL, minq=20, min_baseq=0)
        assert np.array_equal(depth, g[f"{chrom}_q20_Q0"])


@pytest.mark.parametrize("block", [777, 4093, 60000])
def test_records_that_straddle_blocks(hot, golden, tmp_path, block):
    _, refs, recs = golden
    g = np.load(GOLDEN)
    bam = str(tmp_path / "straddle.bam")
    bu.write_bam(bam, refs, recs, block=block, straddle=True)
    for chunk in (0, SMALL):
        for chrom, _ in refs:
            _, depth, _ = same_as_host(hot, bam, chrom, chunk)
            assert np.array_equal(depth, g[f"{chrom}_q0_Q13"])


CASES = bw.cases()


@pytest.mark.parametrize("name", [k for k in CASES if k != "bad_chain"])
def test_crafted_streams(hot, tmp_path, name):
    refs, recs, tid = CASES[name]
    bam = str(tmp_path / (name + ".bam"))
    bu.write_bam(bam, refs, recs)
    chrom = refs[tid][0]
    want, seen, _, _ = bw.serial_walk(b"".join(recs), 0, tid)
    for chunk in (0, SMALL):
        st, _, rs = same_as_host(hot, bam, chrom, chunk)
        assert (st["records"], st["on_chrom"]) == (seen, len(want))
        if name == "decoys":
            assert rs["rewalked"] >= 1                       # the verify path ran on the device too
        if name == "long_record" and chunk == 0:
            assert rs["passed"] >= 2


def test_a_record_carried_over_several_chunks(hot, tmp_path):
    recs = bw.plain_reads(50, 0) + [bw.read_of_size(150_000, 0, 400)] + bw.plain_reads(300, 0, pos0=500, seed=3)
    bam = str(tmp_path / "long.bam")
    bu.write_bam(bam, bw.REFS, recs)
    st, depth, rs = same_as_host(hot, bam, "chrA", SMALL)
    assert st["on_chrom"] == len(recs) and rs["chunks"] >= 3 and rs["passed"] >= 5
    assert depth[400] > 0


def test_malformed_records_are_skipped_not_followed(hot, golden, tmp_path):
    """The four crafted records of test_bam_depth's test of the same name, read on the device."""
    _, refs, recs = golden
    chrom, n = refs[0]
    clean = [r for r in recs if struct.unpack("<i", r[4:8])[0] == 0]
    q = bytes([30] * 50)
    neg = bu.encode_read(0, -1, 60, 0, [("M", 50)], 50, q)
    long_seq = bytearray(bu.encode_read(0, 1000, 60, 0, [("M", 50)], 50, q)); long_seq[20:24] = struct.pack("<i", 1 << 20)
    many_cig = bytearray(bu.encode_read(0, 2000, 60, 0, [("M", 50)], 50, q)); many_cig[16:18] = struct.pack("<H", 60000)
    cig_long = bu.encode_read(0, 3000, 60, 0, [("M", 80)], 50, q)
    merged = sorted(clean + [bytes(long_seq), bytes(many_cig), cig_long], key=lambda r: struct.unpack("<i", r[8:12])[0])
    bad, good = str(tmp_path / "bad.bam"), str(tmp_path / "good.bam")
    bu.write_bam(bad, refs, [neg] + merged)
    bu.write_bam(good, refs, clean)
    _, want, _ = load(hot, good, chrom, "device")
    want[3000:3050] += 1
    for chunk in (0, SMALL):
        st, got, _ = same_as_host(hot, bad, chrom, chunk)
        assert st["malformed"] == 2
        assert np.array_equal(got, want)


def expect_error(hot, bam, chrom, code_name, *words, mode="device", chunk=SMALL):
    from rsicnv_amd import api
    with pytest.raises(api.RsiError) as e:
        load(hot, bam, chrom, mode, chunk)
    assert api.STATUS_NAMES[e.value.code] == code_name, str(e.value)
    for w in words:
        assert w in str(e.value), str(e.value)


def test_errors_leave_the_context_usable(hot, golden, tmp_path):
    bams, refs, recs = golden
    good = bams[False]
    g = np.load(GOLDEN)

    def still_good():
        _, depth, _ = load(hot, good, "chrA", "device", SMALL)
        assert np.array_equal(depth, g["chrA_q0_Q13"])

    raw = bytearray(open(good, "rb").read())
    blocks = bgzf_blocks(bytes(raw))
    off, bsize, _ = blocks[len(blocks) // 2]
    # one flipped payload byte in a middle member: the decoder or the CRC32 catches it, the message names the member
    flipped = bytearray(raw)
    flipped[off + 18 + (bsize - 26) // 2] ^= 0x10
    p = str(tmp_path / "crc.bam")
    open(p, "wb").write(flipped)
    expect_error(hot, p, "chrS", "RSI_ERR_BAD_ARG", f"file offset {off} ", "is bad: ")
    still_good()
    # the file cut at two thirds: inside a member
    p = str(tmp_path / "cut.bam")
    open(p, "wb").write(raw[:len(raw) * 2 // 3])
    assert not any(b[0] == len(raw) * 2 // 3 for b in blocks)
    expect_error(hot, p, "chrS", "RSI_ERR_BAD_ARG", "BGZF block")
    still_good()
    # block_size 31 on the chain
    refs_c, recs_c, tid = CASES["bad_chain"]
    p = str(tmp_path / "bad_chain.bam")
    bu.write_bam(p, refs_c, recs_c)
    for chunk in (0, SMALL):
        expect_error(hot, p, refs_c[tid][0], "RSI_ERR_BAD_ARG", "malformed BAM record", chunk=chunk)
    expect_error(hot, p, refs_c[tid][0], "RSI_ERR_BAD_ARG", "malformed BAM record", mode="host")
    still_good()
    # not a BGZF file
    p = str(tmp_path / "text.bam")
    open(p, "wb").write(b"chrA\t1\t5\n" * 100)
    expect_error(hot, p, "chrA", "RSI_ERR_BAD_ARG")
    still_good()
    # a chromosome with no reads: all-zero depth, no error
    p = str(tmp_path / "empty.bam")
    bu.write_bam(p, refs + [("chrEmpty", 50_000)], recs)
    st, depth, _ = same_as_host(hot, p, "chrEmpty", SMALL)
    assert st["on_chrom"] == 0 and depth.shape == (50_000,) and not depth.any()
    still_good()


def test_bad_member_message_names_the_block_and_the_file(hot, tmp_path):
    """A small BAM of several members, the CRC32 of a middle one flipped: the whole message of the device read."""
    from rsicnv_amd import api
    refs = [("chrT", 3000)]
    p = str(tmp_path / "crc_small.bam")
    bu.write_bam(p, refs, bu.synth_reads(3000, coverage=2.0, seed=5), block=2000)
    raw = bytearray(open(p, "rb").read())
    blocks = bgzf_blocks(bytes(raw))
    assert len(blocks) >= 5                             # header, three members of reads at least, the end-of-file block
    off, bsize, _ = blocks[2]
    raw[off + bsize - 8] ^= 0x10
    open(p, "wb").write(raw)
    with pytest.raises(api.RsiError) as e:
        load(hot, p, "chrT", "device", SMALL)
    assert str(e.value) == f"RSI_ERR_BAD_ARG: BGZF: the block at file offset {off} of {p} is bad: CRC32 mismatch"


def test_set_bam_read_arguments(hot):
    from rsicnv_amd import api
    for bad in (2, -1):
        with pytest.raises(api.RsiError):
            hot.set_bam_read(bad)
    with pytest.raises(ValueError):
        hot.set_bam_read("gpu")
    hot.set_bam_read("device")
    hot.set_bam_read(0)
    assert api.BAM_SEGMENT == bw.SEG


def test_abi(hotlib):
    from rsicnv_amd import api
    hdr = open(os.path.join(ROOT, "include", "rsi_hot.h")).read()
    for sym in ("rsi_hot_set_bam_read", "rsi_hot_last_bam_read_stats"):
        assert re.search(r"\b" + sym + r"\(", hdr) and sym in api.EXPORTS and hasattr(hotlib, sym)
    body = re.search(r"typedef struct rsi_bam_read_stats \{(.*?)\} rsi_bam_read_stats;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    size = 0
    for decl in body.split(";"):
        t = decl.split()
        if t:
            size += {"int32_t": 4, "int64_t": 8, "double": 8}[t[0]] * (decl.count(",") + 1)
    assert C.sizeof(api.RsiBamReadStats) == size == 2 * 4 + 6 * 8 + 3 * 8
    assert "RSI_BAM_READ_HOST = 0" in hdr and "RSI_BAM_READ_DEVICE = 1" in hdr


VOLATILE = ("timing:", "#command:", "#output:", "#bam:")


def log_rows(path, tag):
    return [l.replace(tag, "OUT") for l in open(path).read().splitlines() if not l.startswith(VOLATILE)]


def test_command_line(hotlib, golden, tmp_path):
    from conftest import make_case
    from test_genome_text import write_fasta
    bams, refs, _ = golden
    tmp = str(tmp_path)
    seqs = [(chrom, make_case(hotlib, dict(n=n, seed=0xFA + n, model=0, n_events=1, gaps=0, max_len=3000, end_n=1000))[1]) for chrom, n in refs]
    write_fasta(os.path.join(tmp, "ref.fa"), seqs)

    def run(tag, extra, env=None):
        r = subprocess.run([EXE, "rsi", "-b", bams[False], "-f", "ref.fa", "-o", tag + ".txt", "-np"] + extra, cwd=tmp, capture_output=True, text=True,
                           timeout=300, env=env)
        return r, os.path.join(tmp, tag + ".txt")

    two = dict(os.environ, RSI_HOT_DEVICE_MAP="0,0")
    for name, extra, env in (("all", [], None), ("two", ["-gpus", "2", "-workers", "2"], two), ("one", ["-c", refs[1][0]], None)):
        rh, host = run(name + "_host", extra, env)
        rd, dev = run(name + "_dev", extra + ["-bamread", "device"], env)
        assert rh.returncode == 0 and rd.returncode == 0, (name, rh.stderr[-2000:], rd.stderr[-2000:])
        assert open(dev, "rb").read() == open(host, "rb").read(), name
        hlog, dlog = open(host + ".log").read(), open(dev + ".log").read()
        nchrom = 1 if name == "one" else len(refs)
        assert hlog.count("#bam:") == 0 and dlog.count("#bam: read on the device, ") == nchrom
        assert log_rows(host + ".log", name + "_host.txt") == log_rows(dev + ".log", name + "_dev.txt")
    # -bamread host is the default, spelled out
    rx, explicit = run("explicit", ["-bamread", "host"])
    assert rx.returncode == 0 and open(explicit, "rb").read() == open(os.path.join(tmp, "all_host.txt"), "rb").read()
    assert "#bam:" not in open(explicit + ".log").read()
    # what cannot work
    r, _ = run("x", ["-bamread", "gpu"])
    assert r.returncode != 0 and "device or host" in r.stderr
    r = subprocess.run([EXE, "rsi", "-d", "x.depth", "-c", "chrA", "-f", "ref.fa", "-o", "y.txt", "-np", "-bamread", "device"], cwd=tmp,
                       capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "-bamread" in r.stderr and "-b BAMFILE" in r.stderr
    u = subprocess.run([EXE], capture_output=True, text=True, timeout=60)
    assert "-bamread device|host" in u.stderr + u.stdout
