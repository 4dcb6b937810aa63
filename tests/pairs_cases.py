"""Cases for the read-pair annotation on the device: pair tables and call spans, with a Python restatement of
pairrd.cpp's two routines (the insert-size sample of bam_rd_pr_stats as cnv_stat uses it, and cnv_stat's per-call counts) for
the expected values.  The restatement walks the table serially with the reference's own variables; it shares nothing with
bam_pairs_core.h.  A case is either a list of reads (Read tuples: a BAM can be written from them, and table_of() gives their
table) or, for the sizes no small file reaches, the five arrays directly."""
import struct
from collections import namedtuple

import numpy as np

import bam_util as bu

TID = 1                                   # the chromosome of every case: tid 0 and 2 exist, so mtid 0 / 2 / -1 all mean something
TILE = 1024                               # kernels.h, kPairSampleTile
SAMPLE_BEG, SAMPLE_END = 10_000_000, 349_250_621
Read = namedtuple("Read", "pos cigar mapq flag mtid mpos isize")
M2 = [("M", 40), ("S", 10)]               # two operations, 40 reference bases


def refs(tid_len):
    return [("chr0", 1000), ("chrP", int(tid_len)), ("chr2", 1000)]


def encode(reads):
    return [bu.encode_read(TID, r.pos, r.mapq, r.flag, r.cigar, 50, bytes([30] * 50), name=b"q%d" % i, mtid=r.mtid, mpos=r.mpos, tlen=r.isize)
            for i, r in enumerate(reads)]


def rend_of(r):
    return r.pos + sum(l for op, l in r.cigar if op in ("M", "D", "N")) if r.cigar else r.pos + 1


def info_of(mapq, flag, ncig, mtid, tid=TID):
    return mapq | (flag << 8) | (min(ncig, 2) << 24) | (int(mtid != tid and mtid > 0) << 26) | (int(mtid == tid) << 27)


def table_of(reads):
    """(pos, rend, mpos, isize, info) as int64 arrays (info < 2^32)."""
    cols = [[r.pos for r in reads], [rend_of(r) for r in reads], [r.mpos for r in reads], [r.isize for r in reads],
            [info_of(r.mapq, r.flag, len(r.cigar), r.mtid) for r in reads]]
    return tuple(np.array(c, dtype=np.int64) for c in cols)


def table_from_bytes(records, tid):
    """The table of the encoded records of `tid`, decoded from their bytes (for files whose reads were not made here)."""
    rows = []
    for rec in records:
        rtid, pos, l_nm, mapq, _bin, n_cig, flag, _l_seq, mtid, mpos, isize = struct.unpack_from("<iiBBHHHiiii", rec, 4)
        if rtid != tid:
            continue
        ops = struct.unpack_from(f"<{n_cig}I", rec, 36 + l_nm)
        rend = pos + sum(c >> 4 for c in ops if (c & 0xf) in (0, 2, 3)) if n_cig else pos + 1
        rows.append((pos, rend, mpos, isize, info_of(mapq, flag, n_cig, mtid, tid)))
    return tuple(np.array(c, dtype=np.int64) for c in zip(*rows)) if rows else tuple(np.zeros(0, dtype=np.int64) for _ in range(5))


# ---------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------

def wrap32(v):
    v &= 0xffffffff
    return v - (1 << 32) if v & 0x80000000 else v


def sample_expected(table, tid_len):
    """bam_rd_pr_stats' sampling loop (pairrd.cpp:136-175) over the reads bam_fetch(10000000, 349250621) yields:
    [proper pairs, sum |isize|, sum of int * int, the index of the read it stopped at among those it looked at (-1: none)]."""
    pos, rend, _mpos, isize, info = (a.tolist() for a in table)
    count, pos_start, pos_end = 0, 0, -10000
    c = a = q = 0
    j = -1
    for i in range(len(pos)):
        if not (rend[i] > SAMPLE_BEG and pos[i] < SAMPLE_END):
            continue
        flag = (info[i] >> 8) & 0xffff
        if (info[i] >> 26) & 1 or flag & 0x100 or flag & 0x400:
            continue
        j += 1
        if flag & 0x2 and (info[i] >> 27) & 1:
            c += 1; a += abs(isize[i]); q += wrap32(isize[i] * isize[i])
        if pos[i] >= tid_len:
            break
        if (rend[i] if (info[i] >> 24) & 3 else pos[i]) >= tid_len:       # bam_calend of a read without CIGAR is its pos
            break
        if pos[i] > pos_end + 1000:
            count, pos_start = 0, pos[i]
        pos_end = pos[i]
        count += 1
        if count > 1000000 or pos_end - pos_start > 1000000:
            break
    return [c, a, q, j]


def isize_expected(sums):
    """bamstat_st's isize / isize_sd (ints) from the sums; -1 / -1 with fewer than three pairs."""
    c, a, q = float(sums[0]), float(sums[1]), float(sums[2])
    if not c > 2:
        return -1, -1
    mean = a / c
    return int(mean), int(np.sqrt((q - c * mean * mean) / c))


EXITS = ("ncigar", "matetid", "strand", "del_near", "del_noverlap", "del_close", "del_half_len", "del_half_span", "del_rp",
         "dup_far", "dup_close", "dup_half_len", "dup_half_span", "dup_rp", "other_type")


def annotate_expected(table, calls, mean, sd, exits=None):
    """cnv_stat's loop (pairrd.cpp:640-745) per call, over the reads bam_fetch(p1e, p2e) yields: [(rp, q0_all, q0_q0)].
    exits: a set that collects the name of every way a read left the visitor."""
    pos, rend, mpos, _isize, info = (a.tolist() for a in table)
    out = []
    DIS = 1000
    note = (lambda e: exits.add(e)) if exits is not None else (lambda e: None)
    for start, end, typ in calls:
        beg, end = (end, start) if start > end else (start, end)
        LEN = end - beg + 1
        DIS = min(max(DIS, LEN), 5000)
        p1e, p2e = max(beg - DIS, 1), end + DIS
        q0_all = q0_q0 = rp = 0
        for i in range(len(pos)):
            if pos[i] >= p2e:
                break
            if not (rend[i] > p1e and pos[i] < p2e):
                continue
            if (info[i] >> 24) & 3 < 2:
                note("ncigar"); continue
            if rend[i] > beg and pos[i] < end:
                q0_all += 1
                if info[i] & 0xff == 0:
                    q0_q0 += 1
            if (info[i] >> 26) & 1:
                note("matetid"); continue
            flag = (info[i] >> 8) & 0xffff
            if bool(flag & 0x10) == bool(flag & 0x20):
                note("strand"); continue
            r1, r2 = rend[i], mpos[i]
            if typ == 0:
                if r2 - r1 < mean + sd * 3:
                    note("del_near"); continue
                overlap = min(r2, end) - max(r1, beg)
                if overlap < 0:
                    note("del_noverlap"); continue
                if abs(r1 - beg) + abs(r2 - end) < mean + sd * 3:
                    rp += 1; note("del_close"); continue
                if overlap < LEN * 0.5:
                    note("del_half_len"); continue
                if overlap < (r2 - r1) * 0.5:
                    note("del_half_span"); continue
                rp += 1; note("del_rp")
            elif typ == 1:
                if r2 - r1 > mean - sd * 3:
                    note("dup_far"); continue
                if abs(r1 - beg) + abs(r2 - end) < mean + sd * 3:
                    rp += 1; note("dup_close"); continue
                if r1 > r2:
                    r1, r2 = r2, r1
                overlap = min(r2, end) - max(r1, beg)
                if overlap < LEN * 0.5:
                    note("dup_half_len"); continue
                if overlap < (r2 - r1) * 0.5:
                    note("dup_half_span"); continue
                rp += 1; note("dup_rp")
            else:
                note("other_type")
        out.append((rp, q0_all, q0_q0))
    return out


def q0_of(q0_all, q0_q0):
    return q0_q0 / (q0_all + 0.00001)


# ---------------------------------------------------------------------------------------------------------------------
# sample cases: name -> (reads or None, table, tid_len)
# ---------------------------------------------------------------------------------------------------------------------

PROPER = 0x1 | 0x2 | 0x20


def pair(pos, isize=300, flag=PROPER, cigar=M2, mapq=30, mtid=TID):
    return Read(pos, cigar, mapq, flag, mtid, pos + 250, isize)


def run_of(pos0, n, step=10, **kw):
    return [pair(pos0 + step * k, isize=280 + (k * 7) % 50, **kw) for k in range(n)]


WRAPPING = (70000, -70000) + (100,) * 30     # 70000 * 70000 wraps to 605 032 704 in 32 bits: the variance stays positive


def sample_cases():
    B = SAMPLE_BEG
    big = 40_000_000
    c = {}
    c["two_pairs"] = (run_of(B + 100, 2), big)
    c["three_pairs"] = (run_of(B + 100, 3), big)
    c["all_before"] = (run_of(B - 5000, 30), big)
    c["straddle_by_rend"] = ([pair(B - 39, 311), pair(B - 40, 999)][::-1] + run_of(B + 5, 5), big)     # rend B + 1 counts, rend B does not
    c["gap_1000"] = (run_of(B + 100, 5, 100) + run_of(B + 500 + 1000, 5, 100), big)
    c["gap_1001"] = (run_of(B + 100, 5, 100) + run_of(B + 500 + 1001, 5, 100), big)
    # a span of exactly 1 000 000 goes on, 1 000 001 stops: steps of 1000 never open a new stretch
    c["span_1000000"] = ([pair(B + 100 + 1000 * k, 300 + k % 9) for k in range(1001)] + run_of(B + 100 + 1_000_000 + 500, 4), big)
    c["span_1000001"] = ([pair(B + 100 + 1000 * k, 300 + k % 9) for k in range(1000)] + [pair(B + 100 + 999_500, 351), pair(B + 100 + 1_000_001, 350)]
                         + run_of(B + 100 + 1_000_600, 4), big)
    n = B + 50_000
    c["stop_by_pos"] = (run_of(n - 200, 10, 10) + [pair(n, 400), pair(n + 5, 500)], n)
    c["stop_by_rend"] = (run_of(n - 200, 10, 10) + [pair(n - 40, 410), pair(n - 30, 510)], n)           # rend == n stops
    c["no_cigar_at_the_end"] = (run_of(n - 200, 10, 10) + [pair(n - 1, 420, cigar=[]), pair(n - 1, 520)], n)   # calend n - 1: goes on; the next one stops
    skip = [pair(B + 3000, 777, flag=PROPER | 0x100), pair(B + 3001, 778, flag=PROPER | 0x400), pair(B + 3002, 779, mtid=2)]
    c["passed_over_on_a_boundary"] = (run_of(B + 100, 5, 100) + skip + run_of(B + 3003, 5, 100), big)
    c["mate_not_elsewhere"] = (run_of(B + 100, 4) + [pair(B + 200, 501, mtid=0), pair(B + 210, 502, mtid=-1), pair(B + 220, 503, flag=0x1 | 0x20)], big)
    c["square_wraps"] = ([pair(B + 100 + k, i) for k, i in enumerate(WRAPPING)], big)
    c["negative_isize"] = ([pair(B + 100 + k, -300 - k) for k in range(7)], big)
    c["n0"] = ([], big)
    c["n1"] = (run_of(B + 100, 1), big)
    for d in (-1, 0, 1):
        c[f"tile{d:+d}"] = (run_of(B + 100, TILE + d, 3), big)
    # a passed-over read in the last entry of a tile and one in the first of the next, a boundary right behind them
    seam = run_of(B + 100, TILE - 1, 2) + [pair(B + 2200, 1, flag=PROPER | 0x400), pair(B + 2201, 2, mtid=2)] + run_of(B + 2146 + 1001, 40, 2)
    c["passed_over_on_a_seam"] = (seam, big)
    # the stop in the last entry of tile 0, and in the first entry of tile 1
    c["stop_last_of_tile"] = (run_of(n - 3 * TILE, TILE - 1, 2) + [pair(n + 1, 600)] + run_of(n + 2, 30, 1), n)
    c["stop_first_of_tile"] = (run_of(n - 3 * TILE, TILE, 2) + [pair(n + 1, 600)] + run_of(n + 2, 30, 1), n)
    out = {}
    for name, (reads, tid_len) in c.items():
        out[name] = (reads, table_of(reads) if reads else tuple(np.zeros(0, dtype=np.int64) for _ in range(5)), tid_len)
    return out


def count_cases():
    """count reaching 1 000 000 (goes on) and 1 000 001 (stops): tables only -- no file is written for them."""
    out = {}
    for name, n in (("count_1000000", 1_000_000), ("count_1000001", 1_000_002)):
        k = np.arange(n, dtype=np.int64)
        pos = SAMPLE_BEG + 100 + k // 2
        isize = 250 + (k * 13) % 101
        info = np.full(n, info_of(30, PROPER, 2, TID), dtype=np.int64)
        out[name] = (None, (pos, pos + 40, pos + 250, isize, info), 40_000_000)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# annotation cases: name -> (reads, table, calls [(start, end, type)], mean, sd)
# ---------------------------------------------------------------------------------------------------------------------

FR, RF, FF, RR = 0x1 | 0x20, 0x1 | 0x10, 0x1, 0x1 | 0x10 | 0x20
A_OFF = [-700, -361, -360, -359, -181, -180, -179, -1, 0, 1, 250, 499, 500, 501, 640, 641, 999, 1000, 1001, 1010, 1400]
B_OFF = [-1400, -1001, -1000, -999, -761, -760, -759, -641, -640, -639, -501, -500, -499, -1, 0, 1, 179, 180, 181, 359, 360, 361, 400, 700]


def by_pos(reads):
    return sorted(reads, key=lambda r: r.pos)


def grid(beg, end, flag=FR, cigar=M2):
    """Reads whose end (r1) and mate position (r2) lie at every pair of offsets from the call's two edges."""
    return by_pos([Read(beg + a - 40, cigar, 30 if (a + b) % 3 else 0, flag, TID, end + b, 0) for a in A_OFF for b in B_OFF])


def annotate_cases():
    c = {}
    beg, end = 50_000, 51_000            # LEN 1001; with mean 300, sd 20: far = 360, near = 240
    g = grid(beg, end)
    c["grid_del_dup"] = (g, [(beg, end, 0), (beg, end, 1), (beg, end, 2)], 300, 20)
    c["grid_even_len"] = (grid(beg, end + 1), [(beg, end + 1, 0), (beg, end + 1, 1)], 300, 20)
    c["grid_no_sample"] = (g, [(beg, end, 0), (beg, end, 1)], -1, -1)
    c["grid_swapped_call"] = (g, [(end, beg, 0), (end, beg, 1)], 300, 20)           # start > end
    c["strands"] = (by_pos(grid(beg, end, RF)[::7] + grid(beg, end, FF)[::11] + grid(beg, end, RR)[::13]), [(beg, end, 0), (beg, end, 1)], 300, 20)
    one = [("M", 40)]
    c["cigar_classes"] = (by_pos(grid(beg, end, cigar=[])[::9] + grid(beg, end, cigar=one)[::9] + grid(beg, end)[::9]), [(beg, end, 0), (beg, end, 1)], 300, 20)
    mates = [Read(beg + 10 * k, M2, 0 if k % 2 else 20, FR, mt, end + 400, 0) for k, mt in enumerate((TID, 0, -1, 2, 2, 0, -1, TID))]
    c["mate_elsewhere"] = (mates, [(beg, end, 0), (beg, end, 1)], 300, 20)
    # rend == beg and rend == beg + 1; pos == end - 1 and pos == end (Q0 counts reads overlapping [beg, end) only)
    edge = [Read(beg - 40, M2, 0, FR, TID, end, 0), Read(beg - 39, M2, 0, FR, TID, end, 0), Read(end - 1, M2, 0, FR, TID, end, 0), Read(end, M2, 0, FR, TID, end, 0)]
    c["q0_edges"] = (edge, [(beg, end, 0)], 300, 20)
    low = by_pos([Read(p, M2, 0 if p % 2 else 9, FR, TID, p + 700, 0) for p in (0, 1, 2, 5, 30, 400, 900, 1100, 2500)] + [Read(0, M2, 3, FR, TID, 900, 0)])
    c["p1e_clamped"] = (low, [(300, 800, 0), (300, 800, 1)], 300, 20)
    # DIS carries over: the 10-base call behind the 6000-base one reads 5000 bases either side, in front of it 1000
    far_reads = by_pos([Read(200_000 + d, M2, 0, FR, TID, 200_000 + d + 500, 0) for d in (-5100, -5039, -5038, -4000, -1041, -1039, -1038, 0, 5, 9, 10, 1008, 1009, 4000, 5008, 5009, 5010)]
                       + [Read(100_000 + d, M2, 1, FR, TID, 106_500, 0) for d in (-5039, -5038, 0, 3000, 5999, 6000, 10_998, 10_999)])
    c["dis_long_then_short"] = (far_reads, [(100_000, 105_999, 0), (200_000, 200_009, 0)], 300, 20)
    c["dis_short_then_long"] = (far_reads, [(200_000, 200_009, 0), (100_000, 105_999, 0)], 300, 20)
    c["dis_short_first"] = (by_pos(far_reads), [(100_000, 100_009, 1), (200_000, 200_009, 0), (100_000, 105_999, 0)], 300, 20)
    # one read with a 200 000-base N sets maxspan: it reaches calls whose window begins far behind its pos
    spanning = by_pos(run_plain(300_000, 50, 37) + [Read(300_500, [("M", 20), ("N", 200_000), ("M", 20)], 0, FR, TID, 501_500, 0)] + run_plain(500_000, 50, 37))
    c["long_span"] = (spanning, [(500_200, 500_900, 0), (400_000, 400_100, 1), (300_100, 300_900, 0)], 300, 20)
    c["empty_window"] = (run_plain(300_000, 20, 37), [(700_000, 700_500, 0), (10, 20, 1)], 300, 20)
    c["no_reads"] = ([], [(700_000, 700_500, 0)], 300, 20)
    c["whole_table"] = (run_plain(600_000, 120, 61), [(600_000, 607_400, 0), (600_000, 607_400, 1)], 300, 20)
    for k in (1, 63, 64, 65, 257):
        c[f"in_range_{k}"] = (run_plain(800_000, k, 3), [(800_000, 800_000 + 3 * k + 50, 0), (800_000, 800_000 + 3 * k + 50, 1)], 300, 20)
    rng = np.random.default_rng(0x9A125)
    many = run_plain(1_000_000, 4000, 25)
    calls = []
    for k in range(300):
        s = int(rng.integers(999_000, 1_101_000)); ln = int(rng.choice([5, 80, 900, 4000, 7000]))
        calls.append((s, s + ln, int(rng.integers(0, 3))))
    c["calls_300"] = (many, calls, 300, 20)
    return {name: (reads, table_of(reads) if reads else tuple(np.zeros(0, dtype=np.int64) for _ in range(5)), calls, mean, sd)
            for name, (reads, calls, mean, sd) in c.items()}


def run_plain(pos0, n, step):
    """n reads from pos0 on, every strand pairing, mapq 0 now and then, mates at mixed distances on either side."""
    flags = (FR, RF, FR, FF, FR, RR)
    return [Read(pos0 + step * k, M2 if k % 5 else [("M", 40)], 0 if k % 4 == 0 else 17, flags[k % 6], TID if k % 9 else 2,
                 pos0 + step * k + (-1) ** k * (150 + (k * 53) % 1700), 0) for k in range(n)]


# ---------------------------------------------------------------------------------------------------------------------
# a .bai for a BAM written by bam_util.write_bam
# ---------------------------------------------------------------------------------------------------------------------

def write_bai(bam, records, nref):
    """BAM.bai with what the host annotation takes from one: per reference one bin whose chunk begins at its first read, and the
    linear index (per 16 384-base window the virtual offset of the first read that overlaps it).  records: the encoded reads of
    the file, in its order (write_bam without `straddle` keeps the header in a block of its own: the reads start block 1)."""
    raw = open(bam, "rb").read()
    coffs, usize = [], []
    p = 0
    while p < len(raw):
        bsize = struct.unpack_from("<H", raw, p + 16)[0] + 1
        coffs.append(p); usize.append(struct.unpack_from("<I", raw, p + bsize - 4)[0])
        p += bsize
    ustart = np.cumsum([0] + usize[1:])                        # inflated offset, behind the header's block, at which block k + 1 starts
    lens = np.fromiter((len(r) for r in records), dtype=np.int64, count=len(records))
    at = np.concatenate([[0], np.cumsum(lens)[:-1]]) if len(records) else np.zeros(0, dtype=np.int64)
    blk = np.searchsorted(ustart, at, side="right") - 1
    voff = (np.array(coffs[1:], dtype=np.int64)[blk] << 16) | (at - ustart[blk]) if len(records) else at
    first, linear = {}, {}
    for k, rec in enumerate(records):
        tid, pos, l_nm, _mq, _bin, n_cig = struct.unpack_from("<iiBBHH", rec, 4)
        if tid < 0:
            continue
        end = pos + sum(c >> 4 for c in struct.unpack_from(f"<{n_cig}I", rec, 36 + l_nm) if (c & 0xf) in (0, 2, 3)) if n_cig else pos + 1
        v = int(voff[k])
        first.setdefault(tid, v)
        lin = linear.setdefault(tid, {})
        for w in range(max(pos, 0) >> 14, (max(end, pos + 1) - 1 >> 14) + 1):
            lin.setdefault(w, v)
    with open(bam + ".bai", "wb") as f:
        f.write(b"BAI\1" + struct.pack("<i", nref))
        for t in range(nref):
            if t in first:
                f.write(struct.pack("<iIiQQ", 1, 4681, 1, first[t], len(raw) << 16))
                nw = max(linear[t]) + 1
                f.write(struct.pack("<i", nw) + struct.pack(f"<{nw}Q", *[linear[t].get(w, 0) for w in range(nw)]))
            else:
                f.write(struct.pack("<ii", 0, 0))


def write_case_bam(path, reads, tid_len):
    recs = encode(reads)
    bu.write_bam(path, refs(tid_len), recs, block=20000)
    write_bai(path, recs, 3)
    return recs
