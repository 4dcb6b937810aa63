"""CPU: the Python restatements of the reference's pileup rules (bam_util.depth_rules, base by base, and
bam_util.depth_rules_counts, run by run) against the depth the real reference produced for every case of
bam_edge_cases.py (tests/golden/bam_edges.npz, tools/make_golden_bam.py edges), and the BAM writer they share.

The reference binary got through every case of the five in-reference groups, the references of 1 and 15 bases included
(its annotation pass fails on chromosomes this short, after the dump, as bam_util.reference_depth_dump describes)."""
import hashlib
import struct
import zlib

import numpy as np
import pytest

import bam_edge_cases as ec
import bam_util as bu


def test_golden_bam_bytes_unchanged(tmp_path):
    """The writer learnt to split records over many blocks; the file behind bam_small.npz must not have moved by a byte
    (the digest is that of the file the writer produced before that change)."""
    path, _, _ = bu.build_golden_bam(str(tmp_path))
    assert hashlib.sha256(open(path, "rb").read()).hexdigest() == "635bd33ccc40b61d90d0f062ffae1b8558c000d24f4ee21d0672006e5a8d873a"


def _blocks(path):
    raw, p, out = open(path, "rb").read(), 0, []
    while p < len(raw):
        bsize = struct.unpack_from("<H", raw, p + 16)[0] + 1
        data = zlib.decompress(raw[p + 18:p + bsize - 8], -15)
        assert len(data) == struct.unpack_from("<I", raw, p + bsize - 4)[0] <= bu.BGZF_MAX_PAYLOAD
        out.append(data)
        p += bsize
    assert p == len(raw)
    return out


@pytest.mark.parametrize("layout", ec.case("long_reads").layouts, ids=lambda l: l[0])
def test_writer_splits_records_longer_than_a_block(tmp_path, layout):
    """Every block is a legal BGZF block, the blocks together are the header and the records byte for byte, and the
    file does hold what it was made for: blocks in which no record starts, and records that span more than two."""
    c = ec.case("long_reads")
    blocks = _blocks(c.write(str(tmp_path), layout))
    assert blocks[-1] == b"" and b"".join(blocks[1:]) == b"".join(c.records)
    starts, p = set(), 0
    for r in c.records:
        starts.add(p); p += len(r)
    edges = np.cumsum([0] + [len(b) for b in blocks[1:-1]])
    no_start = sum(1 for a, b in zip(edges[:-1], edges[1:]) if not any(a <= s < b for s in starts))
    assert no_start >= 3
    assert max(len(r) for r in c.records) > 2 * bu.BGZF_MAX_PAYLOAD
    if layout is ec.HTS:       # htslib's way: a record that fits a block is never split
        pos = 0
        for r in c.records:
            if len(r) <= layout[1]["block"]:
                k = int(np.searchsorted(edges, pos, side="right")) - 1
                assert pos + len(r) <= edges[k + 1], "a short record was split"
            pos += len(r)


def test_golden_holds_every_in_reference_case():
    g = ec._golden()
    want = {key + s for name in ec.IN_REFERENCE for key, *_ in ec.case(name).keys() for s in (":n", ":at", ":val")}
    assert set(g.files) == want
    assert not ec.case("outside_reference").golden and all(ec.case(name).golden for name in ec.IN_REFERENCE)


@pytest.mark.parametrize("name", ec.IN_REFERENCE)
def test_python_rules_match_reference_golden_edges(name):
    """Both restatements equal the reference's depth on every reference and setting of the case.  (`stack` only run by
    run: base by base its 70 300 reads would take the seconds the rest of the suite does not have.)"""
    c = ec.case(name)
    for key, t, chrom, n, q, Q in c.keys():
        want = ec.golden_depth(key, n)
        rd, counts = bu.depth_rules_counts(c.records, t, n, minq=q, min_baseq=Q)
        assert np.array_equal(rd, want), (key, int(np.flatnonzero(rd != want)[0]))
        if name != "stack":
            assert np.array_equal(bu.depth_rules(c.records, t, n, minq=q, min_baseq=Q), want), key
        assert counts["used"] <= bu.walk_counts(c.records, t)["on_chrom"]


def test_stack_depth_is_exact():
    c = ec.case("stack")
    rd = ec.golden_depth("stack/chrK/q0_Q13", 8_209)
    assert (rd[4000:4030] == 70_000).all() and (rd[4030:4050] == 70_300).all() and (rd[4050:4080] == 300).all()
    assert not rd[:4000].any() and not rd[4080:].any()
    _, counts = bu.depth_rules_counts(c.records, 0, 8_209)
    assert counts == {"used": 70_300, "runs": 70_300}


def test_edges_in_either_order_are_the_same_reads():
    a, b = ec.case("edges"), ec.case("edges_desc")
    assert [r[0] for r in b.refs] == [r[0] for r in a.refs][::-1]
    for t, (chrom, n) in enumerate(b.refs):
        rd, _ = bu.depth_rules_counts(b.records, t, n)
        assert np.array_equal(rd, ec.golden_depth(f"edges/{chrom}/q0_Q13", n)), chrom


def test_counts_of_the_run_restatement_by_hand():
    """used / runs on reads small enough to count on paper."""
    q = bytes([30, 30, 5, 30, 5, 5, 30, 30, 30, 5])
    R = lambda pos, cig, L=10, flag=0, mapq=60: bu.encode_read(0, pos, mapq, flag, cig, L, q[:L])
    n = 1000
    assert bu.read_runs(R(10, [("M", 10)]), 0, n) == [(10, 12), (13, 14), (16, 19)]
    assert bu.read_runs(R(10, [("M", 10)]), 0, n, min_baseq=0) == [(10, 20)]
    assert bu.read_runs(R(10, [("M", 10)]), 0, n, min_baseq=31) == []                       # used, but no run
    assert bu.read_runs(R(10, [("=", 4), ("M", 6)]), 0, n) == [(10, 12), (13, 14), (12, 15)]    # '=' does not move the position
    assert bu.read_runs(R(10, [("M", 4), ("S", 2), ("M", 4)]), 0, n) == [(10, 12), (13, 14), (16, 19)]   # S after the anchor does
    assert bu.read_runs(R(10, [("S", 2), ("M", 8)]), 0, n) == [(11, 12), (14, 17)]            # S before the anchor does not
    assert bu.read_runs(R(995, [("M", 10)]), 0, n) == [(995, 997), (998, 999)]                # cut at n
    assert bu.read_runs(R(998, [("M", 10)]), 0, n) == [(998, 1000)]                           # the run's end is n itself
    assert bu.read_runs(R(1000, [("M", 10)]), 0, n) == []
    assert bu.read_runs(R(10, [("M", 20)]), 0, n, min_baseq=0) == [(10, 20)]                  # cut at the read's end
    assert bu.read_runs(R(10, [("M", 5), (9, 3), ("M", 5)]), 0, n, min_baseq=0) == [(10, 15), (15, 20)]   # op code 9: ignored
    assert bu.read_runs(R(10, [("M", 10)], L=0), 0, n) == []
    for filtered in (R(0, [("M", 10)]), R(10, [("M", 10)], flag=0x100), R(10, [("M", 10)], flag=0x400), R(10, [("S", 4), ("I", 6)]),
                     R(10, [(9, 4), ("N", 6)])):
        assert bu.read_runs(filtered, 0, n) is None
    assert bu.read_runs(R(10, [("M", 10)], mapq=59), 0, n, minq=60) is None and bu.read_runs(R(10, [("M", 10)]), 1, n) is None
    recs = [R(10, [("M", 10)]), R(10, [("M", 10)]), R(12, [("S", 4), ("I", 6)]), R(995, [("M", 10)]), bu.encode_read(1, 5, 60, 0, [("M", 10)], 10, q)]
    rd, counts = bu.depth_rules_counts(recs, 0, n)
    assert counts == {"used": 3, "runs": 8} and rd.sum() == 2 * 6 + 3
    assert bu.walk_counts(recs + recs, 0) == {"records": 5, "on_chrom": 4}


def test_outside_reference_contract_by_hand():
    """The three families the reference has no answer for, against numbers worked out on paper: qualities are 4 at every
    7th base of the read (not counted at min_baseq 13) and 30 elsewhere."""
    c = ec.case("outside_reference")
    rd, counts = bu.depth_rules_counts(c.records, 0, 10_007)
    rd0, counts0 = bu.depth_rules_counts(c.records, 0, 10_007, min_baseq=0)
    assert counts["used"] == counts0["used"] == 12                                # all but the record of op codes 11, 13, 14 alone
    assert rd0[100:150].all() and not rd0[150:200].any()                         # 80M on 50 bases
    assert rd0[300:330].all() and rd0[330:340].all() and not rd0[340:400].any()  # 30M 10I 30M on 50: the second M keeps 10 bases
    assert (rd0[500:520] == 3).sum() == 10 and (rd0[500:520] == 2).sum() == 10   # three 20= at one position: 20 + 20 + 10
    assert rd0[700:740].all() and not rd0[740:760].any() and rd0[760:780].all() and not rd0[780:800].any()   # 40M 20D 40M on 60
    assert not rd0[900:1100].any()                                               # 60S 40M on 50: the clip uses the read up
    assert rd0[10_007 - 30:].all()
    assert not rd0[1100:1400].any()                                              # l_seq = 0
    assert rd0[1500:1540].all() and not rd0[1540:1560].any()                     # 20M (9) 20M: the unknown op moves nothing
    assert rd0[1700:1730].all() and rd0[1900:1910].all() and (rd0[1910:1920] == 2).all() and not rd0[1920:1930].any()
    assert not rd0[2100:2200].any()
    assert rd0.sum() == 50 + 40 + 50 + 60 + 0 + 30 + 0 + 0 + 40 + 30 + 30 + 0 + 50
    assert rd[100:150].tolist() == [0 if i % 7 == 0 else 1 for i in range(50)]
    assert rd[330:340].tolist() == [0 if i % 7 == 0 else 1 for i in range(40, 50)]   # the bases behind the insertion
    assert counts0["runs"] == 1 + 2 + 3 + 2 + 1 + 2 + 1 + 3 + 1 and counts["runs"] > counts0["runs"]
