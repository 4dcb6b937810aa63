"""Cases for `rsicnv pin` and `rsicnv stat`, with a Python restatement of the reference's three routines for the
expected values: the depth sample of bam_rd_pr_stats, one breakpoint's window of get_rds_stats, and the scoring loop of
optimize_resolution (pairrd.cpp), walked serially with the reference's own variables; cnv_stat's counts come from pairs_cases'
restatement with DIS carried through the list here.  It shares nothing with bam_pin_core.h.  A case is a list of reads (a BAM is
written from them; tables_of() gives their pair table and CIGAR pool), a CNV list as text, and -m.  Every case's chromosome has
10 100 000 bases, its reads lie near 10.0 Mb (the sample) and near the breakpoints, so a case takes well under a second.
tests/golden/pin_edges.npz holds what the reference binary makes of the same files (tools/make_golden_pin.py)."""
import math
from collections import namedtuple

import numpy as np

import bam_util as bu
import pairs_cases as pc

TID = pc.TID
TID_LEN = 10_100_000
CHROM = "chrP"
NO_CHROM = "chrZ"                         # a name the BAM header lacks: the reference segfaults on such a line
SAMPLE_BEG, SAMPLE_END = pc.SAMPLE_BEG, pc.SAMPLE_END
RDC_SIZE = 1_001_000
OPS = bu.CIGAR_OPS
DEL, DUP, UNKNOWN = 0, 1, 2

PRead = namedtuple("PRead", "pos cigar flag mtid lq mapq mpos isize", defaults=(0, TID, None, 30, 0, 0))
Case = namedtuple("Case", "reads cnv m")


def lq_of(r):
    return r.lq if r.lq is not None else sum(l for op, l in r.cigar if op in ("M", "I", "S", "=", "X"))


def encode(reads, tid=TID):
    """The reads as records of chromosome `tid`; a mate on the read's own chromosome (mtid == TID) goes with it."""
    return [bu.encode_read(tid, r.pos, r.mapq, r.flag, r.cigar, lq_of(r), bytes([30] * lq_of(r)), name=b"p%d" % i, mtid=tid if r.mtid == TID else r.mtid,
                           mpos=r.mpos, tlen=r.isize) for i, r in enumerate(reads)]


def write_case_bam(path, reads):
    recs = encode(reads)
    bu.write_bam(path, pc.refs(TID_LEN), recs, block=20000)
    return recs


def words_of(cigar):
    return [(l << 4) | OPS.index(op) for op, l in cigar]


def tables_of(reads):
    """The pair table (pairs_cases.table_of) and the kept CIGARs: lq, coff, pool with pool[0] = 0 (the empty CIGAR) in front."""
    table = pc.table_of([pc.Read(r.pos, r.cigar, r.mapq, r.flag, r.mtid, r.mpos, r.isize) for r in reads])
    pool, coff = [0], []
    for r in reads:
        coff.append(len(pool))
        pool += [len(r.cigar)] + words_of(r.cigar)
    return table, (np.array([lq_of(r) for r in reads], dtype=np.int64), np.array(coff, dtype=np.int64), np.array(pool, dtype=np.int64))


def cigars_from_bytes(records, tid):
    """lq, and per read its CIGAR words, decoded from encoded records (for files whose reads were not made here)."""
    import struct
    lq, cigs = [], []
    for rec in records:
        rtid, _pos, l_nm, _mq, _bin, n_cig, _flag, l_seq = struct.unpack_from("<iiBBHHHi", rec, 4)
        if rtid == tid:
            lq.append(l_seq); cigs.append(list(struct.unpack_from(f"<{n_cig}I", rec, 36 + l_nm)))
    return lq, cigs


# ---------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------

def calend(r):
    return r.pos + sum(l for op, l in r.cigar if op in ("M", "D", "N"))


def iter_query(reads, beg, end):
    """bam_iter_query + bam_iter_read over a sorted file: a negative beg queries from 0."""
    beg = max(beg, 0)
    for r in reads:
        if r.pos >= end:
            break
        if (calend(r) if r.cigar else r.pos + 1) > beg:
            yield r


def passed_over(r):
    return (r.mtid != TID and r.mtid > 0) or r.flag & 0x100 or r.flag & 0x400


def resolve_cigar_pos(r):
    """samfunctions.cpp:38: (op, nop, cop) of every operation, cop 1-based; [] without an anchor."""
    ops = [op for op, _ in r.cigar]
    anchor = next((k for k, op in enumerate(ops) if op in "MD=X"), -1)
    if anchor < 0:
        return []
    cop = [0] * len(ops)
    end = r.pos + 1
    for k in range(anchor, len(ops)):
        cop[k] = end
        if ops[k] in "MDNS":
            end += r.cigar[k][1]
    end = r.pos + 1
    for k in range(anchor - 1, -1, -1):
        if ops[k] in "MDNS":
            end -= r.cigar[k][1]
        cop[k] = end
    return [(ops[k], r.cigar[k][1], cop[k]) for k in range(len(ops))]


def sample_restated(reads, tid_len=TID_LEN):
    """bam_rd_pr_stats(ref, 10000000, 349250621): dict with l_qseq, rd, rd_sd, drd, drd_sd (what it returns), pos_start, pos_end,
    count, grows (the array would have been expanded), and the last stretch's rd / drd arrays from pos_start on."""
    count, pos_start, pos_end, offset, l_qseq_sum = 0, 0, -10000, 0, 0.0
    RDC = np.zeros(RDC_SIZE, dtype=np.int64)
    grows = False
    for r in iter_query(reads, SAMPLE_BEG, SAMPLE_END):
        if passed_over(r):
            continue
        read_pos_end = calend(r)
        if r.pos >= tid_len or read_pos_end >= tid_len:
            break
        if r.pos > pos_end + 1000:
            count, pos_start, offset, pos_end, l_qseq_sum = 0, r.pos, r.pos, r.pos, 0.0
        if read_pos_end - offset > RDC_SIZE - 100:
            grows = True
        pos_end = r.pos
        l_qseq_sum += lq_of(r)
        count += 1
        if count > 1000000 or pos_end - pos_start > 1000000:
            break
        for op, nop, cop in resolve_cigar_pos(r):
            if op not in "M=":
                continue
            p1 = cop - 1
            a, b = p1 - offset, min(p1 + nop, tid_len) - offset
            if a < b and not grows:
                RDC[a:b] += 1
    if count == 0:
        return {"count": 0}
    l_qseq = int(l_qseq_sum / count + 0.5)
    out = {"count": count, "pos_start": pos_start, "pos_end": pos_end, "grows": grows, "l_qseq": l_qseq}
    if grows or l_qseq < 1:
        return out
    q = l_qseq // 4
    length = pos_end - pos_start
    drd = np.zeros(max(length, 1), dtype=np.int64)
    rdmean = drdmean = 0.0
    rd = [int(v) for v in RDC[:max(length, 1) + q + 1]]
    for k in range(q, length - q):                                        # k - offset, offset == pos_start
        dsum0 = sum(rd[k - q:k]); dsum1 = sum(rd[k:k + q])
        drd[k] = int((dsum1 - dsum0) * 4 / l_qseq)                        # C's int division: toward zero
        rdmean += rd[k]; drdmean += int(drd[k])
    n = length - l_qseq // 2
    rdmean = rdmean / n if n else math.nan
    drdmean = drdmean / n if n else math.nan
    drdsd = rdsd = 0.0
    for k in range(q, length - q):
        drdsd += (drdmean - int(drd[k])) * (drdmean - int(drd[k]))
        rdsd += (rdmean - rd[k]) * (rdmean - rd[k])
    with np.errstate(all="ignore"):
        out.update(rd=rdmean, drd=drdmean, drd_sd=float(np.sqrt(np.float64(drdsd) / n)) if n else math.nan,
                   rd_sd=float(np.sqrt(np.float64(rdsd) / n)) if n else math.nan)
    out["rd_array"] = np.array(rd[:max(length, 1)], dtype=np.int64); out["drd_array"] = drd
    return out


def window_restated(reads, bp, r_len, l_qseq, tid_len=TID_LEN):
    """get_rds_stats for one breakpoint: rd, drd, s_beg, s_end over ipos 0 .. 2 r_len."""
    beg, end = bp - r_len, bp + r_len
    size = 2 * r_len + 1
    rd, s_beg, s_end, drd = ([0] * size for _ in range(4))
    for r in iter_query(reads, beg, end):
        if passed_over(r):
            continue
        read_pos_end = calend(r)
        if r.pos >= tid_len or read_pos_end >= tid_len:
            continue
        if len(r.cigar) > 1:
            ipos = r.pos + 1 - beg
            if r.cigar[0][0] not in "MD=X" and 0 <= ipos <= 2 * r_len:
                s_beg[ipos] += 1
            ipos = read_pos_end + 1 - beg
            if r.cigar[-1][0] not in "MD=X" and 0 <= ipos <= 2 * r_len:
                s_end[ipos] += 1
        for op, nop, cop in resolve_cigar_pos(r):
            if op not in "M=":
                continue
            for p1 in range(cop - 1, cop - 1 + nop):
                ipos = p1 + 1 - beg
                if 0 <= ipos <= 2 * r_len:
                    rd[ipos] += 1
    q = l_qseq // 4
    for k in range(q, size - q):
        dsum0 = float(sum(rd[max(k - q, 0):k])); dsum1 = float(sum(rd[k:min(k + q, size)]))
        drd[k] = int((dsum1 - dsum0) * 4 / l_qseq)
    return rd, drd, s_beg, s_end


def fdiv(a, b):
    """a / b as IEEE doubles divide (Python raises on a zero divisor)."""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def pin_restated(reads, calls, m, sample, tid_len=TID_LEN):
    """optimize_resolution over calls = [(start, end, type)] of one chromosome: [(start, end, sc1, sc2)].  sample: sample_restated's."""
    out = []
    for start, end, type_ in calls:
        if abs(end - start) < 800 or type_ == UNKNOWN:
            out.append((start, end, 0, 0))
            continue
        drd_sd, l_qseq = sample["drd_sd"], sample["l_qseq"]
        r_len = max(50, max(m, l_qseq))
        res = []
        for bp, five in ((start, type_ == DEL), (end, type_ == DUP)):
            rd, drd, s_beg, s_end = window_restated(reads, bp, r_len, l_qseq, tid_len)
            score_max, i_score_max = 0.0, -1
            for i in range(len(rd)):
                score = fdiv(-drd[i], drd_sd) + 3.0 * s_end[i] if five else fdiv(drd[i], drd_sd) + 3.0 * s_beg[i]
                if score > score_max:
                    i_score_max, score_max = i, score
            clips = (s_end if five else s_beg)[i_score_max] if i_score_max >= 0 else 0
            res.append((bp - len(rd) // 2 + i_score_max if clips >= 2 else bp, clips))
        out.append((res[0][0], res[1][0], res[0][1], res[1][1]))
    return out


def cnv_type(field):
    f, t = field.lower(), UNKNOWN
    for word, ty in (("del", DEL), ("loss", DEL), ("dup", DUP), ("gain", DUP), ("add", DUP)):
        if word in f:
            t = ty
    return t


def read_cnvlist(text, names):
    """read_cnvlist (loaddata.cpp:606): [(line, cells, tid, start, end, type)] of the accepted lines."""
    def atoi(s):
        import re
        m_ = re.match(r"\s*[+-]?\d+", s)
        return int(m_.group()) if m_ else 0
    out = []
    for line in text.split("\n"):
        if len(line) < 5 or line[0] == "#":
            continue
        cell = line.split()
        if len(cell) < 4:
            continue
        out.append((line, cell, names.index(cell[0]) if cell[0] in names else -1, atoi(cell[1]), atoi(cell[2]), cnv_type(cell[3])))
    return out


def stat_windows(calls):
    """cnv_stat's (beg, end, p1e, p2e) per call, DIS carried through the list."""
    DIS, out = 1000, []
    for start, end, _ in calls:
        beg, end = min(start, end), max(start, end)
        DIS = min(max(DIS, end - beg + 1), 5000)
        out.append((beg, end, max(beg - DIS, 1), end + DIS))
    return out


def stat_restated(table, calls, windows, isize, isize_sd):
    """cnv_stat's counts for the calls of one chromosome with their windows given: [(rp, q0)]."""
    pos, rend, mpos, _isize, info = (a.tolist() for a in table)
    out = []
    for (start, end, type_), (beg, end_, p1e, p2e) in zip(calls, windows):
        LEN = end_ - beg + 1
        q0_all = q0_q0 = rp = 0
        for i in range(len(pos)):
            if not (rend[i] > p1e and pos[i] < p2e) or (info[i] >> 24) & 3 < 2:
                continue
            if rend[i] > beg and pos[i] < end_:
                q0_all += 1
                q0_q0 += (info[i] & 0xff) == 0
            flag = (info[i] >> 8) & 0xffff
            if (info[i] >> 26) & 1 or bool(flag & 0x10) == bool(flag & 0x20):
                continue
            r1, r2 = rend[i], mpos[i]
            far = isize + isize_sd * 3
            if type_ == DEL:
                if r2 - r1 < far: continue
                overlap = min(r2, end_) - max(r1, beg)
                if overlap < 0: continue
                if abs(r1 - beg) + abs(r2 - end_) < far: rp += 1; continue
                if overlap < LEN * 0.5 or overlap < (r2 - r1) * 0.5: continue
                rp += 1
            elif type_ == DUP:
                if r2 - r1 > isize - isize_sd * 3: continue
                if abs(r1 - beg) + abs(r2 - end_) < far: rp += 1; continue
                if r1 > r2: r1, r2 = r2, r1
                overlap = min(r2, end_) - max(r1, beg)
                if overlap < LEN * 0.5 or overlap < (r2 - r1) * 0.5: continue
                rp += 1
        out.append((rp, q0_q0 / (q0_all + 0.00001)))
    return out


def expected(case):
    """What `pin` and `stat` make of a one-chromosome case: (sample, [(start, end, sc1, sc2)], [(rp, q0)]) over its accepted lines."""
    lines = read_cnvlist(case.cnv, [n for n, _ in pc.refs(TID_LEN)])
    calls = [(s, e, t) for _, _, tid, s, e, t in lines if tid >= 0]
    reads = case.reads
    sample = sample_restated(reads)
    pins = pin_restated(reads, calls, case.m, sample) if any(abs(e - s) >= 800 for s, e, _ in calls) else [(s, e, 0, 0) for s, e, _ in calls]
    table, _ = tables_of(reads)
    isize = pc.isize_expected(pc.sample_expected(table, TID_LEN))
    return sample, pins, stat_restated(table, calls, stat_windows(calls), *isize)


# ---------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------
M100 = [("M", 100)]
PAIR = 0x1 | 0x2 | 0x20


def by_pos(reads):
    return sorted(reads, key=lambda r: r.pos)


def background(lo=10_000_000, n=1500, step=10, cigar=M100, lq=None, thin=7):
    """The sample's stretch: a read every `step` bases, every thin-th left out so that the depth steps; proper pairs, so that stat
    has an insert size."""
    return [PRead(lo + step * k, cigar, PAIR, TID, lq, 30, lo + step * k + 200, 300 + k % 9) for k in range(n) if k % thin]


def flank_left(edge, n=60, step=4, cigar=M100):
    """reads ending at or before `edge` (0-based, exclusive)"""
    span = sum(l for op, l in cigar if op in "MDN")
    return [PRead(edge - span - step * k, cigar) for k in range(n)]


def flank_right(edge, n=60, step=4, cigar=M100):
    return [PRead(edge + step * k, cigar) for k in range(n)]


def clipped_end(rend, k, cigar=(("M", 60), ("S", 40))):
    span = sum(l for op, l in cigar if op in "MDN")
    return [PRead(rend - span, list(cigar), mapq=0 if i == 0 else 30) for i in range(k)]


def clipped_beg(pos, k, cigar=(("S", 40), ("M", 60))):
    return [PRead(pos, list(cigar)) for _ in range(k)]


def deletion(a, b, ka=3, kb=3):
    """depth on both sides of [a, b), ka reads clipped at a, kb at b, and two pairs that span it (RP)"""
    span = [PRead(a - 150 - 10 * i, [("M", 90), ("S", 10)], 0x1 | 0x20, TID, None, 30, b + 60 + 10 * i, b - a + 400) for i in range(2)]
    return flank_left(a) + clipped_end(a, ka) + flank_right(b) + clipped_beg(b, kb) + span


def duplication(a, b, ka=3, kb=3):
    """more depth inside [a, b) than outside, reads clipped in front at a and behind at b"""
    inside = [PRead(p, M100) for p in range(a, a + 300, 4)] + [PRead(p, M100) for p in range(b - 400, b - 100, 4)]
    return flank_left(a, n=20, step=12) + clipped_beg(a, ka) + inside + clipped_end(b, kb) + flank_right(b, n=20, step=12)


def line(start, end, type_="DEL", chrom=CHROM, rest="x\t7"):
    return f"{chrom}\t{start}\t{end}\t{type_}\t{rest}"


def cases():
    c = {}
    bg = background()
    A, B = 2_000_040, 2_010_020
    # the issue's example: bin-resolution breakpoints 41 and 21 bases off, a short call, every spelling of the type
    c["types"] = Case(by_pos(bg + deletion(A, B) + duplication(3_000_000, 3_005_000) + deletion(4_000_000, 4_000_799) + deletion(5_000_000, 5_000_800)),
                      "\n".join(["#CHROM\tSTART\tEND\tTYPE", line(2_000_000, 2_010_000), line(2_000_100, 2_000_601), line(3_000_030, 3_004_990, "DUP"),
                                 line(2_000_000, 2_010_000, "copy_loss"), line(3_000_030, 3_004_990, "Gain"), line(2_000_000, 2_010_000, "inversion"),
                                 line(2_000_000, 2_010_000, "addel"), "short", "chrP\t1\t2", line(4_000_010, 4_000_809), line(5_000_010, 5_000_810),
                                 line(2_010_000, 2_000_000), line(60, 2_010_000), line(2_000_000, 2_010_000, chrom=NO_CHROM)]), 101)
    # reads at the window's first and last base: window of the first breakpoint 1_999_899 .. 2_000_101 (beg = bp - r_len, 0-based use)
    bp = 2_000_000
    beg, end = bp - 101, bp + 101
    edge = []
    for e in (beg - 1, beg, beg + 1):
        edge += [PRead(e - 100, M100), PRead(e - 60, [("M", 60), ("S", 40)]), PRead(e - 60, [("M", 60), ("S", 40)])]
    edge += [PRead(end - 1, M100), PRead(end, M100), PRead(end - 1, [("S", 40), ("M", 60)]), PRead(end, [("S", 40), ("M", 60)])]
    edge += [PRead(beg - 1, [("S", 99), ("M", 1)]), PRead(beg - 1, [("S", 99), ("M", 1)])]
    c["window_edges"] = Case(by_pos(bg + edge + flank_right(2_010_020) + clipped_beg(2_010_020, 2)), line(bp, 2_010_000), 101)
    # every operation first and last; 0 and 1 operations; '=' and X; an S inside
    ops = []
    for k, op in enumerate("SHINPMD=X"):
        first = [(op, 5), ("M", 95)]
        last = [("M", 95), (op, 5)]
        ops += [PRead(bp - 40 + 2 * k, first, lq=100), PRead(bp - 40 + 2 * k, first, lq=100), PRead(bp - 130 + 2 * k, last, lq=100), PRead(bp - 130 + 2 * k, last, lq=100)]
    ops += [PRead(bp - 10, [], lq=100), PRead(bp - 10, [("S", 100)]), PRead(bp - 9, [("M", 100)]), PRead(bp - 8, [("=", 50), ("X", 2), ("=", 48)]),
            PRead(bp - 7, [("M", 30), ("S", 10), ("M", 60)]), PRead(bp - 7, [("M", 30), ("S", 10), ("M", 60)])]
    c["operations"] = Case(by_pos(bg + ops + flank_left(bp - 140, n=30) + flank_right(2_010_020) + clipped_beg(2_010_020, 3)),
                           line(bp, 2_010_000) + "\n" + line(bp, 2_010_000, "DUP"), 101)
    # the filters: every one of these reads would add a clip at the breakpoint
    clip = [("M", 60), ("S", 40)]
    filt = [PRead(A - 60, clip, flag=0x100), PRead(A - 60, clip, flag=0x400), PRead(A - 60, clip, mtid=2), PRead(A - 60, clip, mtid=2),
            PRead(A - 60, clip, mtid=0), PRead(A - 60, clip, mtid=-1)]
    c["filters"] = Case(by_pos(bg + flank_left(A) + filt + flank_right(B) + clipped_beg(B, 1)), line(2_000_000, 2_010_000), 101)
    # reads at the chromosome's end: pos or rend at tid_len
    E = TID_LEN
    tail = [PRead(E - 160 - 3 * k, M100) for k in range(30)] + [PRead(E - 100, clip), PRead(E - 100, clip), PRead(E - 60, clip), PRead(E - 60, clip),
                                                                 PRead(E - 61, clip), PRead(E - 61, clip), PRead(E - 61, clip)]
    c["chromosome_end"] = Case(by_pos(bg + flank_right(B) + clipped_beg(B, 2) + tail), line(B - 20, E - 10, "DUP"), 101)
    # scores: two equal maxima (the first wins), clip counts 1 and 2, a window without depth (best score 0: nothing taken)
    tie = clipped_end(A, 2) + clipped_end(A + 30, 2)
    c["ties"] = Case(by_pos(bg + tie + clipped_beg(B, 1) + clipped_beg(B + 10, 2)), line(2_000_000, 2_010_000) + "\n" + line(6_000_000, 6_010_000), 101)
    # a depth step the wrong way round at a DEL's start (drd above 0 there), clips all the same
    c["negative_drd"] = Case(by_pos(bg + flank_right(A, n=80, step=2) + clipped_end(A, 2) + flank_left(B, n=80, step=2) + clipped_beg(B, 2)),
                             line(2_000_000, 2_010_000), 101)
    # a sample whose depth hardly steps: drd_sd small
    c["flat_sample"] = Case(by_pos(background(thin=1500) + deletion(A, B)), line(2_000_000, 2_010_000), 101)
    c["m301"] = Case(by_pos(bg + deletion(A, B)), line(2_000_000, 2_010_000) + "\n" + line(2_000_250, 2_009_800), 301)
    for name, cig, lq in (("lq99", [("M", 99)], None), ("lq101", [("M", 101)], None)):
        c[name] = Case(by_pos(background(cigar=cig) + deletion(A, B)), line(2_000_000, 2_010_000), 101)
    half = background(n=1501)
    half = [r._replace(cigar=[("M", 101)]) if k % 2 else r for k, r in enumerate(half)]
    assert len(half) % 2 == 0                                      # as many of 100 as of 101 bases: the mean ends in .5
    c["lq_mean_half"] = Case(by_pos(half + deletion(A, B)), line(2_000_000, 2_010_000), 101)
    # the iterator's first read starts before 10 Mb; a second stretch after a gap of more than 1000 leaves the first one's counts
    c["first_before_10mb"] = Case(by_pos(background(lo=9_999_950) + deletion(A, B)), line(2_000_000, 2_010_000), 101)
    c["restart"] = Case(by_pos(background(n=900) + background(lo=10_012_000, n=400, step=6, thin=5) + deletion(A, B)), line(2_000_000, 2_010_000), 101)
    return c


def limit_cases():
    """What the device refuses: (reads, the reason's words, chromosome length).  No golden: the reference's behaviour there is not
    defined.  A read 1 000 900 bases behind its stretch's start needs a chromosome longer than the other cases'."""
    bg = background()
    return {"no_sample": (by_pos(deletion(2_000_040, 2_010_020)), "no read from position 10000000", TID_LEN),
            "grows": (by_pos(bg + [PRead(10_014_000, [("M", 50), ("N", 1_000_000), ("M", 50)])]), "1000900 bases", 12_000_000)}


def stat_two_chromosomes():
    """Two chromosomes for `stat`: the first one's 10 001-base call raises DIS to 5000 for the second one's 401-base call (1000
    when DIS starts again), so that call's window holds the reads up to 5000 bases off.  cnv_stat's rules let no read that far
    from a call change its RP or Q0 (a supporting pair overlaps half of its own span), so the windows themselves and the number of
    table entries the device looks at are what shows the carry; the rows only show that nothing else changed.Returns (refs, reads -- both chromosomes hold the same ones --, cnv text)."""
    refs = [("chrA", TID_LEN), ("chrP", TID_LEN)]
    far = [PRead(3_000_000 - 4000 + 300 * k, [("M", 90), ("S", 10)], 0x1 | 0x20, TID, None, 30, 3_000_000 - 3700 + 300 * k, 400) for k in range(10)]
    cnv = "\n".join([line(2_000_000, 2_010_000, chrom="chrA"), line(3_000_000, 3_000_400, chrom="chrP"), line(3_000_000, 3_000_400, chrom="chrA")])
    return refs, by_pos(background() + deletion(2_000_040, 2_010_020) + deletion(3_000_000, 3_000_400) + far), cnv
