"""GPU: the BAM pileup (host record walk, k_bam_depth, the scan kernels) on the inputs of bam_edge_cases.py -- long reads
that span BGZF blocks, odd CIGARs, quality patterns, chromosome ends and scan-tile edges, a pile deeper than 16 bits --
against the depth the real reference produced (tests/golden/bam_edges.npz) and, for the counts and the records the
reference has no answer for, against the run-by-run restatement (bam_util.depth_rules_counts), which
test_bam_edge_rules.py pins to the same golden file on the CPU."""
import functools
import os
import shutil
import struct

import numpy as np
import pytest

import bam_edge_cases as ec
import bam_util as bu

pytestmark = pytest.mark.gpu

GOLDEN_SMALL = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bam_small.npz")


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("bam_edges"))


@pytest.fixture(scope="module")
def ctx(hotlib):
    """One context for the whole module: every load leaves it to the next one as it is."""
    from rsicnv_amd import api
    h = api.RsiHot(0)
    yield h
    h.close()


@functools.lru_cache(maxsize=None)
def _ruler(name, tid, n, q, Q):
    c = ec.case(name)
    rd, counts = bu.depth_rules_counts(c.records, tid, n, minq=q, min_baseq=Q)
    rd.setflags(write=False)
    return rd, dict(counts, **bu.walk_counts(c.records, tid))


def _want(c, key, chrom, n):
    return ec.golden_depth(f"edges/{chrom}/q0_Q13" if c.name == "edges_desc" else key, n)


def _explain(got, want, records, tid):
    """The first position at which the depth differs and the reads that could have put a base there."""
    bad = np.flatnonzero(got != want)
    p = int(bad[0])
    cover = []
    for rec in records:
        rtid, pos0, l_nm, _mq, _bin, n_cig, flag, l_seq = struct.unpack_from("<iiBBHHHi", rec, 4)
        if rtid != tid or pos0 > p: continue
        ops = [(c & 0xf, c >> 4) for c in struct.unpack_from(f"<{n_cig}I", rec, 36 + l_nm)]
        if pos0 + sum(l for _, l in ops) > p:
            cig = "".join(f"{l}{bu.CIGAR_OPS[op] if op < 9 else '?'}" for op, l in ops[:12]) + ("..." if n_cig > 12 else "")
            cover.append(f"{rec[36:36 + l_nm - 1].decode()}@{pos0} flag {flag:#x} l_seq {l_seq} {n_cig} ops {cig}")
    return f"{bad.size} positions differ, the first at {p}: got {int(got[p])}, want {int(want[p])}; reads there: " + "; ".join(cover[:6])


def _check_load(h, c, bam, indexed=False):
    for key, t, chrom, n, q, Q in c.keys():
        st = h.load_depth_bam(bam, chrom, minq=q, min_baseq=Q)
        got = h.fetch("depth_in")
        rule, counts = _ruler(c.name, t, n, q, Q)
        want = _want(c, key, chrom, n) if c.golden or c.name == "edges_desc" else rule
        assert st["n"] == n == got.size and st["tid"] == t and st["indexed"] == int(indexed)
        print(key, {k: st[k] for k in ("records", "on_chrom", "used", "runs", "malformed")}, "max depth", int(got.max()) if n else 0)
        assert np.array_equal(got, want), (key, bam, _explain(got, want, c.records, t))
        assert np.array_equal(rule, want), key           # the two rulers agree (CPU-tested; here it guards the test's own wiring)
        assert (st["used"], st["runs"], st["on_chrom"], st["malformed"]) == (counts["used"], counts["runs"], counts["on_chrom"], 0), (key, st, counts)
        if not indexed:                                  # an indexed load starts at the reference's first record, not the file's
            assert st["records"] == counts["records"], (key, st, counts)


LOADS = [(name, layout) for name in ec.ALL_CASES for layout in ec.case(name).layouts]


@pytest.mark.parametrize("name,layout", LOADS, ids=[f"{n}-{l[0]}" for n, l in LOADS])
def test_depth_and_counts_match_reference(ctx, workdir, name, layout):
    """Every reference and (minq, min_baseq) setting of the case: depth equal to the reference's (for outside_reference:
    to the library's documented contract, cut at the read's end / count nothing / ignore the op), and used, runs,
    on_chrom and records equal to an independent count."""
    c = ec.case(name)
    _check_load(ctx, c, c.write(workdir, layout))


def test_long_reads_block_layouts_agree(ctx, workdir):
    """Records that begin where htslib would put them, at fixed 60 000-byte cuts, and at 4093-byte cuts (one record over
    dozens of blocks, most blocks without a record start): the same depth and counts from all three files."""
    c = ec.case("long_reads")
    for chrom, _ in c.refs:
        seen = []
        for layout in c.layouts:
            st = ctx.load_depth_bam(c.write(workdir, layout), chrom)
            seen.append((ctx.fetch("depth_in"), [st[k] for k in ("records", "on_chrom", "used", "runs", "malformed")]))
        for d, s in seen[1:]:
            assert np.array_equal(d, seen[0][0]) and s == seen[0][1], (chrom, s, seen[0][1])


def _bai_first_offset(path, tid):
    """The smallest chunk start the index holds for reference `tid` (the .bai layout of the SAM specification)."""
    raw = open(path, "rb").read()
    assert raw[:4] == b"BAI\1"
    p, first = 8, None
    for r in range(struct.unpack_from("<i", raw, 4)[0]):
        n_bin = struct.unpack_from("<i", raw, p)[0]; p += 4
        for _ in range(n_bin):
            b, n_chunk = struct.unpack_from("<Ii", raw, p); p += 8
            for k in range(n_chunk):
                beg = struct.unpack_from("<Q", raw, p + 16 * k)[0]
                if r == tid and b != 37450: first = beg if first is None else min(first, beg)
            p += 16 * n_chunk
        p += 4 + 8 * struct.unpack_from("<i", raw, p)[0]
    return first


def test_indexed_load_of_long_reads(ctx, workdir):
    """With a .bai the load starts at the index's first offset for the reference: for chrL that is the middle of the
    block the small chromosome in front of it half fills."""
    import ctypes
    import oracle
    libref = os.path.join(os.path.dirname(oracle.REF_BIN), "libref.so")
    if not os.path.exists(libref):
        pytest.skip("no compiled reference to build the .bai with")
    c = ec.case("long_reads")
    d = os.path.join(workdir, "indexed"); os.makedirs(d, exist_ok=True)
    bam = shutil.copy(c.write(workdir), os.path.join(d, "long_reads.bam"))
    L = ctypes.CDLL(libref)
    L.bam_index_build.argtypes = [ctypes.c_char_p]
    assert L.bam_index_build(os.fsencode(bam)) == 0
    off = _bai_first_offset(bam + ".bai", 1)
    assert off is not None and off & 0xffff, "chrL's first record should lie inside a block"
    _check_load(ctx, c, bam, indexed=True)


@pytest.mark.parametrize("first", ["edges", "edges_desc"])
def test_edges_in_both_orders_on_one_context(hotlib, workdir, first):
    """References of 1 to 1 048 577 bases, ascending and descending, on one context: a short reference after a long one
    finds the difference array cleared beyond its own n + 1, and the scan's tile and pass edges (4096 elements, 256
    tiles) all occur: 4095 / 4096 / 4097 and 256 * 4096 - 1 / + 0 / + 1."""
    from rsicnv_amd import api
    h = api.RsiHot(0)
    for name in (first, "edges_desc" if first == "edges" else "edges", first):
        c = ec.case(name)
        _check_load(h, c, c.write(workdir))
    h.close()


def test_stack_exact_and_through_the_caller(ctx, hotlib, workdir):
    """70 000 identical reads on one spot and 300 beside it: exactly 70 000 / 70 300 / 300.  Then the same pile inside a
    400 kb chromosome at 30x through run_bam: depth as counted here, and calls and the compacted depth equal to those from
    the fetched depth as an array -- a depth beyond 16 bits takes the escape paths of the stages behind the pileup."""
    from conftest import make_case, calls_equal
    from rsicnv_amd import api
    c = ec.case("stack")
    ctx.load_depth_bam(c.write(workdir), "chrK")
    rd = ctx.fetch("depth_in")
    assert (rd[4000:4030] == 70_000).all() and (rd[4030:4050] == 70_300).all() and (rd[4050:4080] == 300).all()
    assert not rd[:4000].any() and not rd[4080:].any()

    n, at = 400_009, 200_000
    rng = np.random.default_rng(0x57AC)
    pos = np.sort(rng.integers(1, n - 100, n * 30 // 100))
    pos = pos[~((pos >= 100_000) & (pos < 112_000) & (rng.random(pos.size) < 0.5))]         # a loss to call
    pos = np.sort(np.concatenate([pos, rng.integers(300_000, 309_000, 2_700)]))             # and a gain
    body = bu.encode_read(0, 0, 60, 0, [("M", 100)], 100, bytes([30] * 100))
    plain = [body[:8] + struct.pack("<i", p) + body[12:14] + struct.pack("<H", bu.reg2bin(p, p + 100)) + body[16:] for p in pos.tolist()]
    k = int(np.searchsorted(pos, at))
    recs = plain[:k] + ec.stack_records(0, at) + plain[k:]
    bam = os.path.join(workdir, "stack_400k.bam")
    bu.write_bam(bam, [("chrK", n)], recs)
    diff = np.zeros(n + 1, dtype=np.int64)
    np.add.at(diff, pos, 1); np.add.at(diff, pos + 100, -1)
    diff[at] += ec.STACK_DEEP; diff[at + 50] -= ec.STACK_DEEP; diff[at + 30] += ec.STACK_NEXT; diff[at + 80] -= ec.STACK_NEXT
    want = np.cumsum(diff[:n]).astype(np.int32)
    _, fasta, _ = make_case(hotlib, dict(n=n, seed=0x57AD, model=0, n_events=1, gaps=1, max_len=5000, end_n=3000, gap_len=6000))
    res = ctx.run_bam(api.make_params(), bam, "chrK", fasta)
    assert res.bam_stats["used"] == res.bam_stats["runs"] == res.bam_stats["on_chrom"] == res.bam_stats["records"] == len(recs)
    got = ctx.fetch("depth_in")
    assert np.array_equal(got, want), int(np.flatnonzero(got != want)[0])
    assert got.max() >= 70_300
    calls, concat = res.calls("calls"), ctx.fetch("rd_concat")
    res_arr = ctx.run(api.make_params(), got, fasta)
    ok, why = calls_equal(calls, res_arr.calls("calls"), rtol=0)
    assert ok, why
    assert len(calls) >= 2
    assert np.array_equal(concat, ctx.fetch("rd_concat"))


def test_context_still_reproduces_the_small_golden(ctx, tmp_path):
    """Last in the file: after everything above, the shared context gives the 100-base golden depth as before."""
    g = np.load(GOLDEN_SMALL)
    bam, refs, _ = bu.build_golden_bam(str(tmp_path))
    chrom, n = refs[0]
    st = ctx.load_depth_bam(bam, chrom, minq=20, min_baseq=0)
    assert st["n"] == n and np.array_equal(ctx.fetch("depth_in"), g[f"{chrom}_q20_Q0"])
