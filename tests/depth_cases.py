"""`rsicnv depth` restated in numpy and plain Python, and the seeded cases the CPU and GPU tests share: the summary,
the 65536-bin distribution with its cap, window and region records, and the exact text of every file under the rounding rule
(two decimals, half up, in integers)."""
import numpy as np

BINS = 65536
SPLIT = 512          # kernels.h, kDepthSplit: depths below it are counted in LDS
SPAN = 1000          # values per workgroup the summary hook is given: small, and no multiple of anything
WSPAN = 100          # bases per workgroup the window hook is given
TILE = 256           # values per tile the region hook is given
I32MAX = (1 << 31) - 1


# ---- the rounding rule ----
def hundredths(S, L):
    """100 a + h: a = S // L, r = S % L, h = (200 r + L) // (2 L), a hundred of them carrying into a; 0 for L <= 0 or S <= 0."""
    S, L = int(S), int(L)
    if L <= 0 or S <= 0:
        return 0
    a, r = divmod(S, L)
    return 100 * a + (200 * r + L) // (2 * L)


def fixed2(S, L):
    q = hundredths(S, L)
    return f"{q // 100}.{q % 100:02d}"


# ---- records ----
def summary(d):
    d = np.asarray(d, dtype=np.int64)
    if d.size == 0:
        return dict(n=0, sum=0, over=0, negative=0, min=0, max=0)
    return dict(n=int(d.size), sum=int(d.sum()), over=int((d > BINS - 1).sum()), negative=0, min=int(d.min()), max=int(d.max()))


def dist(d):
    d = np.asarray(d, dtype=np.int64)
    return np.bincount(np.minimum(d, BINS - 1), minlength=BINS).astype(np.int64)


def windows(n, W):
    W = min(W, n) if n > 0 else W
    return [(k * W, min(n, (k + 1) * W)) for k in range(-(-n // W))] if n > 0 else []


def clip(s, e, n):
    a, b = max(s, 0), min(e, n)
    return (a, b) if b > a else (0, 0)


def written(s, e, n):
    a, b = clip(s, e, n)
    return (a, b) if b > a else (s, e)


def region_record(d, s, e):
    a, b = clip(s, e, len(d))
    if b <= a:
        return (0, 0, 0, 0)
    v = np.asarray(d[a:b], dtype=np.int64)
    return (b - a, int(v.sum()), int(v.min()), int(v.max()))


def record_of(row):
    return (int(row["n"]), int(row["sum"]), int(row["min"]), int(row["max"]))


# ---- text ----
def line(name, s, e, S, pos0=0):
    return f"{name}\t{s + pos0}\t{e + pos0}\t{fixed2(S, e - s)}\n"


def window_text(name, d, W, pos0=0):
    d = np.asarray(d, dtype=np.int64)
    return "".join(line(name, s, e, int(d[s:e].sum()), pos0) for s, e in windows(d.size, W))


def region_text(name, d, regions, pos0=0):
    out = []
    for s, e in regions:
        ws, we = written(s, e, len(d))
        out.append(line(name, ws, we, region_record(d, s, e)[1], pos0))
    return "".join(out)


def summary_text(chroms):
    """chroms: (name, depth array) in order -> PREFIX.mosdepth.summary.txt"""
    rows = [(name,) + tuple(summary(d)[k] for k in ("n", "sum", "min", "max")) for name, d in chroms]
    live = [r for r in rows if r[1] > 0]
    rows.append(("total", sum(r[1] for r in live), sum(r[2] for r in live), min((r[3] for r in live), default=0), max((r[4] for r in live), default=0)))
    return "chrom\tlength\tbases\tmean\tmin\tmax\n" + "".join(f"{nm}\t{n}\t{S}\t{fixed2(S, n)}\t{lo}\t{hi}\n" for nm, n, S, lo, hi in rows)


def dist_lines(name, bins, n, top):
    if n <= 0:
        return ""
    at_least = np.cumsum(bins[::-1])[::-1]
    return "".join(f"{name}\t{k}\t{fixed2(int(at_least[k]), n)}\n" for k in range(min(max(top, 0), BINS - 1), -1, -1))


def dist_text(chroms):
    """PREFIX.mosdepth.global.dist.txt: per chromosome, then total"""
    out, total, n, top = [], np.zeros(BINS, dtype=np.int64), 0, 0
    for name, d in chroms:
        b = dist(d)
        out.append(dist_lines(name, b, len(d), int(np.max(d, initial=0))))
        total += b
        n += len(d)
        top = max(top, int(np.max(d, initial=0)))
    return "".join(out) + dist_lines("total", total, n, top)


# ---- the seeded cases ----
LENGTHS = (0, 1, 2, 63, 64, 65, 255, 256, 257, SPAN - 1, SPAN, SPAN + 1)


def value_cases():
    """name -> int32 array; every one has 3 * SPAN + 17 values (more than one workgroup of the hook's span, the last one short)."""
    n = 3 * SPAN + 17
    rng = np.random.default_rng(0xDE9)
    c = {}
    c["all_zero"] = np.zeros(n, dtype=np.int32)
    c["all_equal_30"] = np.full(n, 30, dtype=np.int32)                 # every lane adds to one value's counters
    c["poisson_30"] = rng.poisson(30, n).astype(np.int32)
    c["around_split"] = rng.choice([SPLIT - 1, SPLIT, SPLIT + 1], n).astype(np.int32)
    c["all_split"] = np.full(n, SPLIT, dtype=np.int32)                 # every lane adds to one global bin
    c["around_65535"] = rng.choice([0, 65534, 65535, 65536, 70000], n).astype(np.int32)
    c["int32_max_beside_0"] = np.where(rng.random(n) < 0.5, I32MAX, 0).astype(np.int32)   # sums pass 2^32
    c["runs"] = np.repeat(rng.integers(0, 700, n // 7 + 1), 7)[:n].astype(np.int32)     # flat stretches: the four-in-one add
    return c


def region_cases(n):
    """name -> list of (start, end) on an array of n values (n >= 600)"""
    rng = np.random.default_rng(0xBED)
    c = {}
    c["none"] = []
    c["empty"] = [(5, 5), (0, 0), (n, n), (9, 3)]
    c["clipped_both_ends"] = [(-10, 7), (n - 5, n + 100), (-3, n + 3)]
    c["outside"] = [(n, n + 50), (n + 10, n + 20), (-20, -5), (-20, 0)]
    c["overlapping_duplicate_unsorted"] = [(100, 400), (50, 150), (100, 400), (399, 401), (0, 1), (300, 310)]
    c["whole_array"] = [(0, n)]
    c["tile_seams"] = [(0, TILE - 1), (0, TILE), (0, TILE + 1), (1, TILE + 1), (TILE - 1, 2 * TILE + 1), (7, 7 + 2 * TILE)]
    s = rng.integers(-20, n + 10, 3000)
    c["batch_3000"] = [(int(a), int(a + l)) for a, l in zip(s, rng.integers(0, 600, 3000))]
    return c


# means on a rounding tie, and one that carries: (values, W) whose one window has that mean
TIES = [
    (np.array([1] + [0] * 199, dtype=np.int32), 200, "0.01"),          # 0.005 -> 0.01
    (np.array([1] + [0] * 7, dtype=np.int32), 8, "0.13"),              # 0.125 -> 0.13
    (np.array([1] * 199 + [0], dtype=np.int32), 200, "1.00"),          # 0.995 -> carries into the integer part
    (np.array([3] * 399 + [2], dtype=np.int32), 400, "3.00"),          # 2.9975 -> 3.00
    (np.array([I32MAX] * 5, dtype=np.int32), 5, f"{I32MAX}.00"),
    (np.array([I32MAX, I32MAX - 1, I32MAX], dtype=np.int32), 3, f"{I32MAX - 1}.67"),
]
