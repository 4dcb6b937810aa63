"""Inputs for the NB transform alone (K5: k_nb_raw, k_nb_scale_mm, nb_reference_levels between them; negative_binomial_transfer,
rsi.cpp:1145-1185) at its sizes, at every place its minimum can sit, and at the inputs where the device's log may differ from libm's:
tests/test_nb_cases.py on the CPU, tests/test_nb_edges.py on the GPU through rsi_hot_debug_nb_transform; the reference's answers for the
cases built from a depth array: tools/make_golden_nb.py -> golden/nb_edges.npz.

numpy and math only, seeded.  A case is a Case: name, group, claim, binsum (int64), m, ncompact, RDmedian, r, and expect, what the case claims
about itself; tests/test_nb_cases.py proves every claim from the restatement below, never from the library.

The restatement.  Per bin Python's math.sqrt / math.log -- the machine's libm, the one the compiled reference links, not numpy's own log
-- in the reference's order of operations, rounded to float32 where the reference stores a float.  A bin's raw value depends on its sum
alone (the bins are whole: nb = ncompact / m, the reference's i2 clamp never fires), so an array is a table over its distinct sums.

Hard inputs.  The divide and the square roots are correctly rounded on both sides, so log's argument is the same double on the device and
in libm; the two logs may differ in the last place.  The double t = 2 sqrt(r) log(..) is then rounded to float: a difference in t's last
places changes the float only when t lies next to a rounding midpoint.  An input is HARD when the low 29 mantissa bits of the host's t lie
within HARD_D of 2^28 -- computed from the host side alone.  HARD_D = 8: the device's double log is documented at 1 ulp, libm's is
about 0.52 ulp, the product with 2 sqrt(r) rounds once more: under 4 ulps of t, doubled.  (The 1 ulp is the figure of the HIP math API's
table for double-precision log; the ROCm documents installed next to the compiler used here carry no such table to quote it from.)
Outside hard inputs the device must give the same float; on a hard input it may differ by one float step.
"""
import math
import struct
from collections import namedtuple

import numpy as np

Case = namedtuple("Case", "name group claim binsum m ncompact RDmedian r expect")

F32 = np.float32
THREADS = 256
PER_BLOCK = 4 * THREADS        # launch_nb_raw / launch_nb_scale_minmax: a workgroup for every 1024 bins ...
GRID_CAP = 512                 # ... up to 512 of them (kMaxGrid): 131 072 threads a stride, 524 288 bins at four a thread
HARD_D = 8
SIZES = (3, 4, 8, 255, 256, 257, 1023, 1024, 1025, 131071, 131072, 131073, 524287, 524288, 524289)
PLACES = ("bin0", "bin1", "bin2", "last", "last_workgroup", "second_stride", "several")


def grid(nb):
    return max(1, min(GRID_CAP, (nb + PER_BLOCK - 1) // PER_BLOCK))


# ---- the reference's transform, restated (rsi.cpp:1145-1185) ------------------------------------------------------------------------------
def nbt(total, m2, r):
    """2.0*sqrt(r)*log( sqrt((sum+0.25)/(m2*r-0.5)) + sqrt(1.0+(sum+0.25)/(m2*r-0.5)) ), the double."""
    q = (total + 0.25) / (m2 * r - 0.5)
    return 2.0 * math.sqrt(r) * math.log(math.sqrt(q) + math.sqrt(1.0 + q))


def is_hard(t):
    """The double t lies within HARD_D units of its last place of a midpoint between two floats."""
    if not math.isfinite(t):
        return False
    low = struct.unpack("<q", struct.pack("<d", t))[0] & ((1 << 29) - 1)
    return abs(low - (1 << 28)) <= HARD_D


Restated = namedtuple("Restated", "raw T tmin hard_raw hard_T t0 t2 levels")


def transform(binsum, m, ncompact, RDmedian, r):
    """negative_binomial_transfer from the bin sums on: raw (the floats before the minimum is taken off), T, the minimum, the hard flags."""
    nb = binsum.size
    assert ncompact // m == nb and nb >= 3
    uniq, inv = np.unique(binsum, return_inverse=True)
    td = [nbt(float(int(s)), float(m), r) for s in uniq]          # m2 = double(i2 - i1 + 1) = m for every bin
    table = np.array(td, dtype=np.float64).astype(F32)            # RDt[i] = (float) ...
    raw = table[inv]
    hard_raw = np.array([is_hard(t) for t in td], dtype=bool)[inv]
    med = nbt(RDmedian * m, float(m), r)
    dele = nbt(RDmedian / 2.0 * float(m), float(m), r)
    dup = nbt(RDmedian * 1.5 * float(m), float(m), r)
    # double tmin = RDt[0]; if (RDt[i] < tmin) tmin = RDt[i]: the smallest float (a NaN never wins)
    tmin = float(raw[0])
    rest = raw[~np.isnan(raw)]
    if rest.size and not math.isnan(tmin):
        tmin = float(rest.min())
    with np.errstate(all="ignore"):
        T = (raw.astype(np.float64) - tmin).astype(F32)           # RDt[i] -= tmin
        med_nbt = np.float64(med) - tmin                          # numpy doubles: a division by zero gives what C gives
        T = (T.astype(np.float64) / med_nbt * RDmedian).astype(F32)
        levels = np.array([(np.float64(dele) - tmin) / med_nbt * RDmedian, (np.float64(dup) - tmin) / med_nbt * RDmedian,
                           med_nbt / med_nbt * RDmedian]).astype(F32)
    T[:3] = levels                                                # RDt[0] = del_nbt; RDt[1] = dup_nbt; RDt[2] = med_nbt
    at_min = raw == F32(tmin)
    hard_T = hard_raw | bool(hard_raw[at_min].any())              # a hard minimum moves every bin
    hard_T[:3] = bool(hard_raw[at_min].any())                     # the three levels hang on the minimum alone (their logs are the host's)
    return Restated(raw, T, F32(tmin), hard_raw, hard_T, levels[0], levels[2], (dele, med, dup))


def plan(T):
    """What k_nb_scale_mm leaves for the first quantile grid: (flags, buckets, minimum) from T's min / max / non-finite values."""
    if not np.isfinite(T).all():
        return 2, 0, F32(0)
    ymin, ymax = float(T.min()), float(T.max())
    if ymax - ymin < 0.01:
        return 4, 0, F32(ymin)
    n = int((ymax - ymin) / 0.01 + 2)
    return (8, 0, F32(ymin)) if n > 1 << 20 else (0, n, F32(ymin))


def float_steps(a, b):
    """Distance of two float32 arrays in float steps (NaN against NaN is 0, whatever the payload; NaN against a number is huge)."""
    def key(x):
        i = x.view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    d = np.abs(key(a) - key(b))
    na, nb_ = np.isnan(a), np.isnan(b)
    return np.where(na & nb_, 0, np.where(na | nb_, 1 << 40, d))


# ---- the domain sweep and the hard list ------------------------------------------------------------------------------------------------
# (RDmedian, MAD, m) with half-integer medians and MADs, as the reference's 0.01-grid medians of integers are; r = RDmedian / MAD
SWEEP = ((30.0, 4.0, 101), (30.5, 4.5, 101), (15.0, 2.0, 101), (7.5, 1.0, 101), (60.0, 8.0, 101), (99.5, 12.5, 101), (30.0, 4.0, 51), (45.5, 6.0, 201))
SWEEP_SUMS = 1 << 16


def sweep_cases():
    return [Case(f"sweep_{med:g}_{mad:g}_{m}", "sweep", f"every sum 0 .. 2^16 - 1 at RDmedian {med:g}, MAD {mad:g}, m {m}",
                 np.arange(SWEEP_SUMS, dtype=np.int64), m, SWEEP_SUMS * m, med, med / mad, {}) for med, mad, m in SWEEP]


def hard_case(total, m, RDmedian, mad):
    """A stored hard input in a call of its own: eight bins, a zero-sum bin as the known minimum, the hard sum on bins 3 and 7."""
    b = np.array([total, total, total, total, 0, int(RDmedian * m), int(RDmedian * m) + 1, total], dtype=np.int64)
    return Case(f"hard_{RDmedian:g}_{mad:g}_{total}", "hard", "an input whose double lies next to a float midpoint", b, m, 8 * m, RDmedian,
                RDmedian / mad, dict(hard_bins=[0, 1, 2, 3, 7]))


# ---- the cases built from a depth array: RDmedian, the 31 subsample MADs and r are the reference's own (golden/nb_edges.npz) ---------------
def stored_inputs():
    """[(name, rd, m)]: seeded depth arrays of a few thousand bins at most, a small m."""
    out = []
    for name, seed, nb, m, extra, lam, shape in (("rd_poisson_30", 0x4B01, 1500, 5, 0, 30.0, 0.0), ("rd_gampois_40", 0x4B02, 2300, 7, 3, 40.0, 6.0),
                                                 ("rd_poisson_8", 0x4B03, 257, 11, 10, 8.0, 0.0), ("rd_gampois_100", 0x4B04, 1025, 3, 1, 100.0, 4.0),
                                                 ("rd_three_bins", 0x4B05, 3, 31, 0, 20.0, 0.0)):
        rng = np.random.default_rng(seed)
        n = nb * m + extra
        mean = rng.gamma(shape, lam / shape, size=n) if shape else np.full(n, lam)
        rd = rng.poisson(mean).astype(np.int32)
        if nb > 100:
            rd[40 * m:43 * m] = 0               # a stretch of empty bins: the minimum, three times
            rd[90 * m:91 * m] //= 2
        out.append((name, rd, m))
    return out


def binsums(rd, m):
    nb = rd.size // m
    return rd[:nb * m].astype(np.int64).reshape(nb, m).sum(axis=1)


# ---- building ------------------------------------------------------------------------------------------------------------------------
def place_bins(nb, place):
    """The bins that hold the minimum for a placement, or None where the size has no such place."""
    g = grid(nb)
    stride = g * THREADS
    if place in ("bin0", "bin1", "bin2"):
        return [int(place[-1])]
    if place == "last":
        return [nb - 1]
    if place == "last_workgroup":           # a bin of the last workgroup's first stride that is none of the above
        b = (g - 1) * THREADS + 5
        return [b] if 3 <= b < nb - 1 else None
    if place == "second_stride":            # a bin only the second grid stride visits
        b = stride + 7
        return [b] if b < nb - 1 else None
    if place == "several":
        bins = sorted({1, nb // 2, nb - 1, min(nb - 1, stride + 1)})
        return bins if len(bins) >= 3 and nb >= 8 else None
    raise ValueError(place)


def drawn_sums(rng, nb, RDmedian, m, distinct=3000):
    """nb sums drawn from at most `distinct` values around RDmedian * m, none below 0.6 of it."""
    centre = RDmedian * m
    pool = np.unique(np.maximum(rng.normal(centre, centre * 0.12, size=distinct), centre * 0.6).astype(np.int64))
    return pool[rng.integers(0, pool.size, size=nb)]


_cases = None


def _build():
    C = []
    rng = np.random.default_rng(0x4B5EED)
    big_places = {131071: ("bin0", "last", "several", "second_stride"), 131072: ("bin1", "last_workgroup", "second_stride"),
                  131073: ("bin2", "last", "second_stride"), 524287: ("bin0", "last", "several", "second_stride"),
                  524288: ("bin1", "last_workgroup", "second_stride"), 524289: ("bin2", "last", "second_stride")}
    for i, nb in enumerate(SIZES):
        m = (101, 51, 11)[i % 3]
        extra = (0, 1, m - 1)[i % 3]                       # ncompact a multiple of m, and not
        RDmedian, mad = ((30.0, 4.0), (30.5, 4.5), (12.0, 2.5))[i % 3]
        for place in big_places.get(nb, PLACES):
            bins = place_bins(nb, place)
            if bins is None:
                continue
            b = drawn_sums(rng, nb, RDmedian, m)
            low = int(b.min()) - 1 - int(rng.integers(0, 50))
            b[bins] = low
            C.append(Case(f"nb_{nb}_{place}", "sizes", f"{nb} bins, the minimum on bin(s) {bins}", b, m, nb * m + extra, RDmedian, RDmedian / mad,
                          dict(min_bins=bins, place=place)))
    # ---- sums and r at their ends ----------------------------------------------------------------------------------------------------------
    b = drawn_sums(rng, 700, 30.0, 101)
    b[333] = 0
    C.append(Case("zero_sum_bin", "ends", "a bin of sum 0: the minimum", b, 101, 700 * 101, 30.0, 7.5, dict(min_bins=[333])))
    deep = float((1 << 31) - 100) + 0.5
    b = (np.int64(deep * 101) + np.random.default_rng(0x4B5EEE).integers(-10 ** 9, 0, size=600)).astype(np.int64)
    b[17] = (1 << 31) * 101 - 1
    C.append(Case("deep_coverage", "ends", "sums near 2^31 m", b, 101, 600 * 101 + 50, deep, deep / 40000.5, dict(near=float(1 << 31) * 101)))
    for name, r in (("r_one", 1.0), ("r_million", 999999.5)):
        b = drawn_sums(rng, 513, 30.0, 101)
        C.append(Case(name, "ends", f"r = {r:g}", b, 101, 513 * 101, 30.0, r, {}))
    # ---- degenerate: every bin holds the median level's sum and the transform of it is a float: med_nbt = 0 -----------------------------------
    s, r = DEGENERATE
    C.append(Case("degenerate", "ends", "the minimum equals the median level: med_nbt = 0, every value is non-finite", np.full(40, s, dtype=np.int64), 1,
                  40, float(s), r, dict(nonfinite=True)))
    return C


# (sum, r) at m = 1 for which 2 sqrt(r) log(..) is a double with 29 zero bits at its low end, a float: found by a search over
# r = k / 4 and sums below 2^17 with this machine's libm; tests/test_nb_cases.py asserts that it still is one
DEGENERATE = (38336, 1642.75)


def all_cases():
    global _cases
    if _cases is None:
        _cases = _build()
        assert len({c.name for c in _cases}) == len(_cases)
    return _cases


def get_case(name):
    return next(c for c in all_cases() if c.name == name)


# ---- what golden/nb_edges.npz adds: the stored cases' scalars and answers, the hard list --------------------------------------------------
def stored_cases(z):
    """[(Case, the reference's T)] of the depth arrays, with the reference's own RDmedian and r (z: the loaded golden file)."""
    import json
    names, off = json.loads(str(z["names"])), z["off"]
    out = []
    for name, rd, m in stored_inputs():
        i = names.index(name)                                      # a case without a golden answer is an error, not a skip
        c = Case(name, "stored", f"a depth array of {rd.size} bases, m = {m}", binsums(rd, m), m, rd.size, float(z["RDmedian"][i]), float(z["r"][i]),
                 dict(rd=rd))
        out.append((c, z["T"][off[i]:off[i + 1]]))
    return out


def hard_cases(z):
    """[(Case, the stored libm answer t)] of the hard list."""
    return [(hard_case(int(s), 101, float(med), float(mad)), float(t))
            for med, mad, s, t in zip(z["hard_median"], z["hard_mad"], z["hard_sum"], z["hard_t"])]
