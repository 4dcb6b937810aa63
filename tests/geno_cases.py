"""`rsicnv geno`: seeded cases and a plain Python restatement -- the statistic (sort, index by the ranks), the
region mapping, the flanks, the formatted field.  Shared by test_geno_host.py (CPU), test_geno_device.py (GPU) and
tools/make_golden_geno.py.

A case is an array of values, the storages it runs in (1: bytes, 4: int32) and a list of jobs, each six half-open ranges' ends
(lo, hi, flo0, fhi0, flo1, fhi1): the body [lo, hi) and the two pieces of the flank.

WIDE_SPAN names the cases in which some range's max - min reaches 10^6: the compiled reference allocates one counter per unit
of span, so tests/golden/geno_edges.npz leaves those cases out and they are checked against the restatement alone.  They are the
only ones: every other case is in the golden file, range by range."""
import collections

import numpy as np

TILE = 256                       # values per tile through the hook: seams inside arrays of a few thousand values
GOLDEN_SPAN = 10 ** 6
WIDE_SPAN = ("span_0_and_2p30", "batch_wide_3000")

Case = collections.namedtuple("Case", "depth storages jobs")


# ---------------------------------------------------------------------------------------------------------------------
# the statistic
# ---------------------------------------------------------------------------------------------------------------------

def ranks(n):
    """0-based indices into the sorted values: lower quartile, median, upper quartile (partition_stat_tp with dy = 1)."""
    return [max(n // 4, 1) - 1, max(n // 2, 1) - 1, max(3 * n // 4, 1) - 1]


def quantiles(values):
    s = np.sort(np.asarray(values, dtype=np.int64))
    return [int(s[r]) for r in ranks(s.size)] if s.size else [0, 0, 0]


def record(depth, job):
    """Every field of rsi_geno_record for one job, chrom_median excepted: a dict of Python ints and lists."""
    lo, hi, a0, b0, a1, b1 = job
    body = np.asarray(depth[lo:hi], dtype=np.int64)
    flank = np.concatenate([np.asarray(depth[a0:b0], dtype=np.int64), np.asarray(depth[a1:b1], dtype=np.int64)])
    return dict(n_body=int(body.size), n_flank=int(flank.size), body_min=int(body.min()) if body.size else 0, body_max=int(body.max()) if body.size else 0,
                body_sum=int(body.sum()), flank_sum=int(flank.sum()), body_q=quantiles(body), flank_q=quantiles(flank))


def record_of(row):
    """The same dict from one element of a GENO_RECORD array."""
    return dict(n_body=int(row["n_body"]), n_flank=int(row["n_flank"]), body_min=int(row["body_min"]), body_max=int(row["body_max"]),
                body_sum=int(row["body_sum"]), flank_sum=int(row["flank_sum"]), body_q=[int(v) for v in row["body_q"]],
                flank_q=[int(v) for v in row["flank_q"]])


# ---------------------------------------------------------------------------------------------------------------------
# regions
# ---------------------------------------------------------------------------------------------------------------------

def kept_before(x, pairs):
    """Kept bases in front of the 0-based reference position x; pairs: inclusive (start, end), sorted, disjoint."""
    return x - sum(min(e + 1, x) - s for s, e in pairs if s < x)


def map_line(start, end, n, pairs):
    """START / END, 1-based inclusive -> the half-open compacted interval (a, b); (0, 0) for a line outside [1, n]."""
    if start > end:
        start, end = end, start
    if end < 1 or start > n:
        return 0, 0
    start, end = max(start, 1), min(end, n)
    return kept_before(start - 1, pairs), kept_before(end, pairs)


def line_job(a, b, m, ncompact):
    F = max(b - a, m)
    return (a, b, max(0, a - F), a, b, max(b, min(ncompact, b + F)))


def tiles_of(jobs, tile):
    """(job index, offset, length) in the order the kernels' table has them: job 2 i the body of line i, 2 i + 1 its flank."""
    out = []
    for i, (lo, hi, a0, b0, a1, b1) in enumerate(jobs):
        for j, (a, b) in ((2 * i, (lo, hi)), (2 * i + 1, (a0, b0)), (2 * i + 1, (a1, b1))):
            out += [(j, p, min(tile, b - p)) for p in range(a, b, tile)]
    return out


def field(rec, chrom_median, ploidy=2.0):
    """The text a line gets, from a record() dict."""
    has, med = rec["n_body"] > 0, float(rec["body_q"][1])
    ok = has and chrom_median > 0
    return ("CN=" + ("%.2f" % (med / chrom_median * ploidy) if ok else "NA") + ";RATIO=" + ("%.3f" % (med / chrom_median) if ok else "NA") +
            ";MED=" + ("%g" % med if has else "NA") + ";FLANK=" + ("%g" % float(rec["flank_q"][1]) if rec["n_flank"] > 0 else "NA") +
            ";CHR=%g;N=%d" % (chrom_median, rec["n_body"]))


# the mapping's own cases: (name, n, removed pairs, start, end, expected (a, b)); two removed regions [100, 199] and [300, 349]
MAP_N, MAP_PAIRS = 1000, [(100, 199), (300, 349)]
MAP_CASES = [
    ("inside_removed", 120, 180, (100, 100)),             # N = 0
    ("straddles_one", 91, 210, (90, 110)),
    ("straddles_both", 50, 400, (49, 250)),
    ("starts_on_edge", 101, 250, (100, 150)),             # base 101 is the region's first
    ("ends_on_edge_first_removed", 50, 101, (49, 100)),
    ("ends_on_last_removed", 50, 200, (49, 100)),
    ("starts_behind_region", 201, 210, (100, 110)),
    ("base_1", 1, 1, (0, 1)),
    ("base_n", 1000, 1000, (849, 850)),
    ("swapped", 210, 91, (90, 110)),
    ("beyond_n", 990, 5000, (839, 850)),
    ("wholly_beyond_n", 1001, 2000, (0, 0)),
    ("from_zero", 0, 10, (0, 10)),
    ("negative", -50, -10, (0, 0)),
    ("whole", 1, 1000, (0, 850)),
]


# ---------------------------------------------------------------------------------------------------------------------
# the kernels' cases
# ---------------------------------------------------------------------------------------------------------------------

def _flanked(lo, hi, n, f):
    return (lo, hi, max(0, lo - f), lo, hi, min(n, hi + f))


def cases():
    rng = np.random.default_rng(0x6E0)
    out = {}
    n = 4096
    base = rng.poisson(30, n).astype(np.int64)
    base[::97] = 255                                                       # the byte range's top value
    base[1000:1100] = 0
    # lengths 1 .. 8 at several offsets (aligned and not), flanks of 3
    out["short_lengths"] = Case(base, (1, 4), [_flanked(o, o + k, n, 3) for k in (1, 2, 3, 4, 5, 7, 8) for o in (0, 1, 2, 3, 255, 256, 1001, n - k)])
    flat = np.full(600, 17, dtype=np.int64)
    out["all_equal"] = Case(flat, (1, 4), [_flanked(0, 600, 600, 0), _flanked(5, 6, 600, 4), _flanked(10, 18, 600, 8), _flanked(100, 400, 600, 300)])
    # ties: 8 values whose run of 5s ends exactly on the rank n/4 = 2, n/2 = 4, 3n/4 = 6, or one short of it
    ties = np.array([5, 5, 9, 9, 9, 9, 9, 9,  5, 9, 9, 9, 9, 9, 9, 9,  5, 5, 5, 5, 9, 9, 9, 9,  5, 5, 5, 9, 9, 9, 9, 9,
                     5, 5, 5, 5, 5, 5, 9, 9,  5, 5, 5, 5, 5, 9, 9, 9,  9, 5, 9, 5, 9, 5, 9, 5], dtype=np.int64)
    out["ties_on_ranks"] = Case(ties, (1, 4), [_flanked(o, o + 8, ties.size, 8) for o in range(0, ties.size - 7, 8)] +
                                [_flanked(o, o + k, ties.size, 0) for o in (0, 8, 16) for k in (3, 5, 7)])
    # tile seams: tile - 1, tile, tile + 1 values, at aligned and unaligned offsets, and flanks that cross seams
    out["tile_seams"] = Case(base, (1, 4), [_flanked(o, o + k, n, f) for k in (TILE - 1, TILE, TILE + 1, 2 * TILE, 2 * TILE + 1) for o, f in ((0, 0), (3, 300), (TILE, TILE), (1001, 513))])
    big = rng.poisson(40, 8192).astype(np.int64)
    out["whole_array"] = Case(big, (1, 4), [(0, 8192, 0, 0, 8192, 8192), (0, 8192, 0, 0, 0, 0), (1, 8191, 0, 1, 8191, 8192)])
    # empty left flank, empty right flank, both empty, an empty body with a flank, nothing at all
    out["empty_flanks"] = Case(base, (1, 4), [(0, 50, 0, 0, 50, 100), (n - 50, n, n - 100, n - 50, n, n), (0, n, 0, 0, n, n), (70, 70, 60, 70, 70, 80),
                                              (9, 9, 9, 9, 9, 9), (500, 900, 500, 500, 900, 900)])
    out["overlapping_and_duplicate"] = Case(base, (1, 4), [_flanked(100, 700, n, 600), _flanked(100, 700, n, 600), _flanked(300, 1000, n, 200),
                                                           _flanked(0, n, n, 0), _flanked(100, 700, n, 600), (650, 660, 100, 700, 300, 1000)])
    out["no_jobs"] = Case(base, (1, 4), [])
    out["one_job"] = Case(base, (1, 4), [_flanked(2000, 2300, n, 300)])
    lo = rng.integers(0, n - 40, 3000)
    ln = rng.integers(1, 41, 3000)
    out["batch_3000"] = Case(base, (1, 4), [_flanked(int(a), int(a + k), n, int(max(k, 11))) for a, k in zip(lo, ln)])
    # int32 alone: values around 16 bits, a narrow band at 2^30, and 0 beside 2^30 (the multi-pass road)
    v16 = rng.choice(np.array([0, 1, 65535, 65536, 65537, 40000], dtype=np.int64), 3000)
    out["around_65536"] = Case(v16, (4,), [_flanked(o, o + k, 3000, k) for o, k in ((0, 3000), (10, 7), (500, 257), (1000, 1024), (2990, 10))])
    band = (1 << 30) + rng.integers(-900, 900, 3000)
    out["band_at_2p30"] = Case(band, (4,), [_flanked(o, o + k, 3000, k) for o, k in ((0, 3000), (10, 8), (500, 255), (1000, 1025))])
    wide = rng.poisson(30, 3000).astype(np.int64)
    wide[::3] = (1 << 30) + rng.integers(0, 5000, wide[::3].size)
    wide[7::50] = (1 << 31) - 1
    wide[1::50] = 0
    out["span_0_and_2p30"] = Case(wide, (4,), [_flanked(o, o + k, 3000, k) for o, k in ((0, 3000), (0, 4), (9, 3), (500, 257), (1000, 1024), (2000, 5))] +
                                  [(0, 2, 0, 0, 2, 2)])
    out["batch_wide_3000"] = Case(wide, (4,), [_flanked(int(a) % 2950, int(a) % 2950 + int(k), 3000, int(k)) for a, k in zip(lo, ln)])
    for name, c in out.items():
        assert c.depth.size <= 8192 and c.depth.min() >= 0 and c.depth.max() < 1 << 31
        assert 1 not in c.storages or c.depth.max() <= 255, name
        for j in c.jobs:
            assert all(0 <= a <= b <= c.depth.size for a, b in zip(j[0::2], j[1::2])), (name, j)
    return out


def is_wide(case):
    """Some range of the case spans 10^6 or more: beyond what the compiled reference can be asked."""
    for lo, hi, a0, b0, a1, b1 in case.jobs:
        for v in (case.depth[lo:hi], np.concatenate([case.depth[a0:b0], case.depth[a1:b1]])):
            if v.size and int(v.max()) - int(v.min()) >= GOLDEN_SPAN:
                return True
    return False


def golden_ranges(case):
    """The value sets the golden file stores for a case: per job the body's and the flank's (None for an empty one)."""
    out = []
    for lo, hi, a0, b0, a1, b1 in case.jobs:
        for v in (case.depth[lo:hi], np.concatenate([case.depth[a0:b0], case.depth[a1:b1]])):
            out.append(np.ascontiguousarray(v, dtype=np.int32) if v.size else None)
    return out
