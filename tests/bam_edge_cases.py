"""The BAM inputs on which the pileup is tested beyond 100-base reads: long reads that span BGZF blocks, a CIGAR zoo,
quality patterns that split every op into runs, chromosome ends and scan-tile edges, a pile deeper than 16 bits, and
three families of records on which the reference itself has no defined behaviour.  Everything is deterministic.

A case gives its references, its records in coordinate order, the BGZF layouts it is written in and the
(minq, min_baseq) settings it is run under.  tools/make_golden_bam.py runs the reference on every case with
`golden=True` and stores its depth in tests/golden/bam_edges.npz; the tests read it back with golden_depth()."""
import functools
import os
import struct

import numpy as np

import bam_util as bu

GOLDEN_EDGES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bam_edges.npz")
SCAN_TILE = 4096            # elements per tile of the device scan; 256 tile sums per pass of its offsets kernel

HTS = ("hts", dict(block=60000))
STRADDLE_60000 = ("straddle60000", dict(block=60000, straddle=True))
STRADDLE_4093 = ("straddle4093", dict(block=4093, straddle=True))


class Case:
    def __init__(self, name, refs, records, settings, layouts=(HTS,), golden=True):
        self.name, self.refs, self.settings, self.layouts, self.golden = name, refs, list(settings), list(layouts), golden
        # coordinate order: by reference, then position (stable, so equal positions keep the order they were made in)
        self.records = sorted(records, key=lambda r: struct.unpack_from("<ii", r, 4))

    def write(self, workdir, layout=HTS):
        path = os.path.join(workdir, f"{self.name}_{layout[0]}.bam")
        if not os.path.exists(path):
            bu.write_bam(path, self.refs, self.records, **layout[1])
        return path

    def keys(self):
        """(golden key, tid, chrom, n, minq, min_baseq) for every reference and setting."""
        return [(f"{self.name}/{chrom}/q{q}_Q{Q}", t, chrom, n, q, Q)
                for t, (chrom, n) in enumerate(self.refs) for q, Q in self.settings]


def _qual(rng, L, lo=2, hi=41, ff=0):
    q = rng.integers(lo, hi, L).astype(np.uint8)
    for _ in range(ff):                                   # stretches of 0xff ("no quality"): they pass every threshold up to 255
        a = int(rng.integers(0, max(1, L)))
        q[a:a + int(rng.integers(1, 500))] = 0xff
    return q.tobytes()


def _qlen(cig):
    return sum(l for op, l in cig if op in ("M", "I", "S", "=", "X"))


def _long_reads():
    rng = np.random.default_rng(0x10A6)
    n = 300_007
    refs = [("chrP", 5_003), ("chrL", n)]                 # the small one in front: chrL's first record lies inside a block
    recs = [bu.encode_read(0, int(p), 40, 0, [("M", 100)], 100, _qual(rng, 100), name=b"p%d" % i)
            for i, p in enumerate(np.sort(rng.integers(1, 4_950, 30)))]
    lens = {"M": 40, "I": 6, "D": 12, "N": 300, "S": 20, "=": 30, "X": 3, "P": 4}
    ops, w = list(lens), np.array([30, 8, 8, 2, 3, 30, 12, 3], dtype=np.float64)
    for i in range(40):
        L = int(rng.integers(8_000, 30_001))
        cig = [("S", 7), ("=", 25), ("M", 10), ("X", 2), ("M", 31)] if i % 2 else [("M", 12)]   # M right after '=' and after X
        have = _qlen(cig)
        while have < L:
            op = ops[int(rng.choice(len(ops), p=w / w.sum()))]
            if op == cig[-1][0]:
                continue
            l = int(rng.integers(1, lens[op] + 1))
            if op in "MIS=X":
                l = min(l, L - have)
                have += l
            cig.append((op, l))
        assert _qlen(cig) == L and len(cig) < 65536
        pos = int(rng.integers(1, n - 2_000))             # the late ones run over the chromosome's end
        recs.append(bu.encode_read(1, pos, int(rng.integers(0, 61)), int(rng.choice([0, 0, 0, 0x10, 0x800, 0x400])), cig, L,
                                   _qual(rng, L, ff=int(rng.integers(0, 4))), name=b"L%d" % i))
    recs.append(bu.encode_read(1, 100_000, 60, 0, [("M", 1), ("D", 1)] * 30_000, 30_000, _qual(rng, 30_000, ff=2), name=b"md"))
    recs.append(bu.encode_read(1, 200_000, 60, 0, [("=", 1)] * 30_000, 30_000, _qual(rng, 30_000, ff=2), name=b"eq"))
    return Case("long_reads", refs, recs, [(0, 13), (30, 0)], layouts=(HTS, STRADDLE_60000, STRADDLE_4093))


ZOO_FLAGS = (0x4, 0x10, 0x100, 0x400, 0x800, 0x200)


def _cigar_zoo():
    rng = np.random.default_rng(0x200)
    n = 50_021
    fixed = [
        [("=", 30), ("M", 40)], [("X", 3), ("M", 60)], [("=", 10), ("X", 1), ("=", 10), ("M", 30), ("=", 20)],   # M after '=' / X: overlapping runs
        [("D", 9), ("M", 50)], [("D", 4), ("=", 40), ("D", 3), ("M", 20)],                                    # D as the anchor
        [("N", 30), ("P", 2), ("I", 4), ("H", 6), ("S", 8), ("M", 50)], [("H", 3), ("S", 5), ("I", 2), ("N", 7), ("=", 33)],
        [("P", 1), ("N", 5), ("D", 2), ("M", 44)], [("S", 9), ("I", 9), ("X", 2), ("M", 30)],
        [("M", 30), ("S", 12), ("M", 30)], [("=", 20), ("S", 5), ("=", 20), ("S", 5), ("M", 20)],               # S after the anchor does move the position
        [("M", 0), ("M", 40)], [("S", 0), ("M", 35), ("D", 0), ("M", 35)], [("I", 0), ("=", 0), ("N", 10), ("M", 31)],
        [("M", 25), ("I", 0), ("M", 25)], [("D", 0), ("S", 10), ("M", 40)], [("X", 0), ("M", 50), ("N", 0), ("=", 10)],   # zero-length ops
        [("M", 20), ("P", 3), ("M", 20)], [("P", 5), ("M", 40), ("P", 0)], [("=", 15), ("P", 2), ("=", 15), ("P", 9), ("M", 15)],
        [("S", 10), ("I", 5)], [("N", 20)], [("H", 5), ("P", 2)], [("I", 30), ("S", 3), ("N", 9), ("H", 2)],   # no anchor at all
    ]
    lens = {"M": 40, "I": 8, "D": 10, "N": 60, "S": 12, "H": 6, "P": 4, "=": 40, "X": 3}
    cigs = list(fixed)
    while len(cigs) < 420:
        cig = [(op, int(rng.integers(0, lens[op] + 1))) for op in rng.choice(list("ISHNP"), int(rng.integers(0, 4)))]
        if rng.random() < 0.95:
            a = str(rng.choice(list("MD=X")))
            cig.append((a, int(rng.integers(0 if rng.random() < 0.1 else 1, lens[a] + 1))))
            for op in rng.choice(list("MIDNSHP=X"), int(rng.integers(0, 9)), p=[.3, .08, .08, .05, .08, .03, .05, .25, .08]):
                cig.append((str(op), int(rng.integers(0 if rng.random() < 0.1 else 1, lens[str(op)] + 1))))
            if _qlen(cig) < 30:
                cig.append((str(rng.choice(list("M="))), int(rng.integers(30, 150)) - _qlen(cig)))
        cigs.append([(str(op), l) for op, l in cig])
    pos = np.sort(rng.integers(1, n + 40, len(cigs)))
    pos[:3] = [0, 1, 1]                                   # position 0 is skipped by the reference
    pos[-4:] = [n - 40, n - 1, n, n + 30]
    order = rng.permutation(len(cigs))
    recs = []
    for i, p in enumerate(pos.tolist()):
        cig = cigs[int(order[i])]
        r = rng.random()
        flag = 0 if r < 0.6 else int(rng.choice(ZOO_FLAGS)) if r < 0.85 else int(np.bitwise_or.reduce(rng.choice(ZOO_FLAGS, 3)))
        L = _qlen(cig)
        recs.append(bu.encode_read(0, p, int(rng.integers(0, 61)), flag, cig, L, _qual(rng, L, lo=0, hi=46, ff=int(rng.random() < 0.1)), name=b"z%d" % i))
    return Case("cigar_zoo", [("chrZ", n)], recs, [(0, 13), (20, 0)])


def _quality_runs():
    n = 20_011
    alt = lambda a, b: bytes([a if i % 2 == 0 else b for i in range(100)])
    one = lambda i, v=3: bytes([v if k == i else 30 for k in range(100)])
    quals = [alt(12, 13), alt(13, 12), alt(0, 255), alt(40, 41), alt(41, 42), alt(14, 0), one(0), one(99), one(0, 0), one(99, 0),
             one(50), bytes([30] * 100), bytes([0] * 100), bytes([255] * 100), bytes([41] * 100), bytes([12] * 50 + [13] * 50)]
    recs, k = [], 0
    for mapq in (0, 59, 60, 61, 254, 255):                # around the minq settings below
        for q in quals:
            recs.append(bu.encode_read(0, 1 + 37 * k, mapq, 0, [("M", 100)] if k % 3 else [("=", 40), ("M", 60)], 100, q, name=b"q%d" % k))
            k += 1
    for j, low in enumerate((48, 49, 50)):                # base 49 of a read at n-50 lands on n-1: a low base just before it, on it, past it
        for mapq in (60, 255):
            recs.append(bu.encode_read(0, n - 50, mapq, 0, [("M", 100)], 100, one(low), name=b"e%d" % j))
    for mapq in (60, 255):
        recs.append(bu.encode_read(0, n - 100, mapq, 0, [("M", 100)], 100, one(99), name=b"l"))      # ends on n-1 with a low last base
        recs.append(bu.encode_read(0, n - 100, mapq, 0, [("M", 100)], 100, alt(12, 13), name=b"a"))  # ... with a run of one base there
        recs.append(bu.encode_read(0, n - 99, mapq, 0, [("M", 100)], 100, alt(13, 12), name=b"b"))   # the base on n-1 is the last one counted
    return Case("quality_runs", [("chrQ", n)], recs, [(0, 13), (0, 0), (0, 41), (0, 256), (60, 0), (61, 0), (255, 0)])


EDGE_LENGTHS = (1, 15, 4095, 4096, 4097, 1_048_575, 1_048_576, 1_048_577)


def _edge_reads(rng, tid, n):
    """Reads around the end of a reference of n bases and across every scan-tile boundary in it."""
    out = []
    def add(pos0, L, name):
        if pos0 >= 0 and L >= 1:
            q = bytearray([30] * L)
            if L > 4 and rng.random() < 0.3: q[int(rng.integers(0, L))] = 5
            out.append(bu.encode_read(tid, int(pos0), 50, 0, [("M", L)], L, bytes(q), name=name))
    for last in (n - 3, n - 2, n - 1, n, n + 98):         # last base of the read: the -1 lands on diff[n-1], diff[n], or is cut
        L = min(100, last)                                # keeps pos0 >= 1 on the short references
        add(last - L + 1, L, b"end%d" % (last - n))
    add(0, 10, b"zero")                                   # skipped: pos == 0
    add(n - 1, 60, b"startlast")
    add(n, 60, b"startpast")
    add(n + 7, 60, b"startpast7")
    # 0 to 3 reads across every tile boundary: the carry into a tile (the depth at its first base) is 0, 1, 2 or 3, and a
    # tile in which more reads end than start has a negative sum
    for b in range(SCAN_TILE, n + 1, SCAN_TILE):
        for _ in range(int(rng.integers(0, 4))):
            add(b - int(rng.integers(1, 100)), 100, b"t")
    for _ in range(min(n // 50, 40)):
        add(int(rng.integers(1, n)), 100, b"s")
    return out


def _edges(descending=False):
    lengths = EDGE_LENGTHS[::-1] if descending else EDGE_LENGTHS
    refs = [(f"e{n}", n) for n in lengths]
    recs = []
    for tid, (_, n) in enumerate(refs):
        recs += _edge_reads(np.random.default_rng(0xED6E + n), tid, n)     # the same reads whichever place the reference has
    return Case("edges_desc" if descending else "edges", refs, recs, [(0, 13)], golden=not descending)


STACK_DEEP, STACK_NEXT = 70_000, 300


def stack_records(tid, pos0):
    q = bytes([30] * 50)
    return ([bu.encode_read(tid, pos0, 60, 0, [("M", 50)], 50, q, name=b"k")] * STACK_DEEP
            + [bu.encode_read(tid, pos0 + 30, 60, 0, [("M", 50)], 50, q, name=b"j")] * STACK_NEXT)


def _stack():
    return Case("stack", [("chrK", 8_209)], stack_records(0, 4_000), [(0, 13)])


def _outside_reference():
    """Records on which the reference reads past its own buffers; the library's contract is the ruler (bam_util.read_runs)."""
    n = 10_007
    q = lambda L: bytes([30 if i % 7 else 4 for i in range(L)])
    R = lambda pos, cig, L, name: bu.encode_read(0, pos, 60, 0, cig, L, q(L), name=name)
    recs = [
        # a CIGAR longer than the read: cut at the read's last base
        R(100, [("M", 80)], 50, b"long1"), R(300, [("M", 30), ("I", 10), ("M", 30)], 50, b"long2"), R(500, [("=", 20)] * 3, 50, b"long3"),
        R(700, [("M", 40), ("D", 20), ("M", 40)], 60, b"long4"), R(900, [("S", 60), ("M", 40)], 50, b"long5"), R(n - 30, [("M", 80)], 50, b"long6"),
        # no sequence at all, with M ops: counts nothing, but is a used read
        R(1_100, [("M", 50)], 0, b"noseq1"), R(1_300, [("S", 10), ("M", 40)], 0, b"noseq2"),
        # op codes 9-15: not an anchor, no count, no move of either position
        R(1_500, [("M", 20), (9, 10), ("M", 20)], 40, b"op9"), R(1_700, [(12, 5), ("M", 30)], 30, b"op12"),
        R(1_900, [("M", 10), (15, 7), ("=", 10), (10, 3), ("M", 10)], 30, b"op15"), R(2_100, [(11, 4), (13, 9), (14, 1)], 0, b"op11"),
        R(2_300, [("M", 50)], 50, b"plain"),
    ]
    return Case("outside_reference", [("chrO", n)], recs, [(0, 13), (0, 0)], golden=False)


@functools.lru_cache(maxsize=None)
def case(name):
    return {"long_reads": _long_reads, "cigar_zoo": _cigar_zoo, "quality_runs": _quality_runs, "edges": _edges,
            "edges_desc": lambda: _edges(descending=True), "stack": _stack, "outside_reference": _outside_reference}[name]()


IN_REFERENCE = ("long_reads", "cigar_zoo", "quality_runs", "edges", "stack")
ALL_CASES = IN_REFERENCE + ("outside_reference",)


# ---- the golden file: a depth array as the positions where it changes and the values it takes there ----
def pack_depth(rd):
    rd = np.asarray(rd, dtype=np.int32)
    at = np.flatnonzero(np.diff(rd, prepend=np.int32(0))).astype(np.int32)
    return at, rd[at]


def unpack_depth(at, val, n):
    d = np.zeros(n + 1, dtype=np.int32)
    d[at] = np.diff(val, prepend=np.int32(0))
    return np.cumsum(d[:n], dtype=np.int32)


@functools.lru_cache(maxsize=None)
def _golden():
    return np.load(GOLDEN_EDGES)


def golden_depth(key, n):
    g = _golden()
    assert int(g[key + ":n"]) == n, key
    return unpack_depth(g[key + ":at"], g[key + ":val"], n)
