"""The keyed form of the NB transform and its quantile chains (k_nb_keys, k_nb_apply): cases and a NumPy restatement of "every
statistic from the histogram of the bin sums".

The restatement.  A whole bin's value is a function of its integer sum, so the transform is a table over the distinct sums
(nb_cases.transform already works that way) and a quantile over the bins is a quantile over (value, count) pairs: the minimum and the
maximum of the occupied values, partition_stat_tp's bucket of every occupied value (grid_restatement.buckets), the counts added per
bucket, the walk to n // 2.  Bins 0..2 hold the three levels, not their sums' values, and are three pairs of their own; their sums
still count for the raw minimum.  tests/test_nb_keyed_cases.py holds this to the array forms (nb_cases.transform, nb_cases.plan,
grid_restatement.pair) with ==; tests/test_nb_keyed.py holds the device to it.

numpy and math only, seeded."""
from collections import namedtuple

import numpy as np

import grid_restatement as gr
import nb_cases as nc

F32 = np.float32
KEY_LIMIT = 1 << 15                 # pipeline_steps.h: kNbKeyLimit
EMPTY, NONFINITE, DEGENERATE, TOO_WIDE = 1, 2, 4, 8

Case = namedtuple("Case", "name binsum m K RDmedian r mask form")

Keyed = namedtuple("Keyed", "T tmin out records")   # out = (median, count, MAD, count); records = (flags, np, flags, np)


def _record(vals, cnts):
    """(flags, buckets, ymin) of a (value, count) list: grid_plan_block's tests in their order."""
    vals = vals[cnts > 0]
    if vals.size == 0:
        return EMPTY, 0, 0.0
    if not np.isfinite(vals).all():
        return NONFINITE, 0, 0.0
    ymin, ymax, npb = gr.span(vals)
    if npb is None:
        return DEGENERATE, 0, ymin
    return (TOO_WIDE, 0, ymin) if npb > gr.CAP else (0, npb, ymin)


def _walk(vals, cnts, ymin, npb):
    """The bucket at which the running count reaches total // 2, as a value; the total."""
    h = np.bincount(gr.buckets(vals, ymin).astype(np.int64), weights=cnts.astype(np.float64), minlength=npb).astype(np.int64)
    total = int(cnts.sum())
    b = int(np.argmax(np.cumsum(h) >= total // 2))
    return ymin + b * gr.DY, total


def nbt(total, m2, r):
    """nb_cases.nbt, with C's NaN where Python's math raises (a negative quotient under the square root)."""
    try:
        return nc.nbt(total, m2, r)
    except ValueError:
        return float("nan")


def transform_per_bin(binsum, m, RDmedian, r):
    """negative_binomial_transfer bin by bin, for the inputs nb_cases.transform does not take (non-finite values): T and the minimum."""
    raw = np.array([nbt(float(int(s)), float(m), r) for s in binsum], dtype=np.float64).astype(F32)
    ok = raw[~np.isnan(raw)]
    tmin = float(ok.min()) if ok.size and not np.isnan(raw[0]) else float(raw[0])
    med, dele, dup = nbt(RDmedian * m, float(m), r), nbt(RDmedian / 2.0 * float(m), float(m), r), nbt(RDmedian * 1.5 * float(m), float(m), r)
    with np.errstate(all="ignore"):
        med_nbt = np.float64(med) - tmin
        T = ((raw.astype(np.float64) - tmin).astype(F32).astype(np.float64) / med_nbt * RDmedian).astype(F32)
        T[:3] = np.array([(np.float64(dele) - tmin) / med_nbt * RDmedian, (np.float64(dup) - tmin) / med_nbt * RDmedian,
                          med_nbt / med_nbt * RDmedian]).astype(F32)
    return T, F32(tmin)


def keyed(binsum, m, RDmedian, r, mask=None, raw_table=None):
    """The transform and the (median, MAD) pair of the bins with mask == 0, from the distinct sums and their counts alone.
    raw_table: {sum: float32 raw value} to use in place of the host's libm (a device's own logs on hard inputs)."""
    binsum = np.asarray(binsum, dtype=np.int64)
    nb = binsum.size
    uniq, inv = np.unique(binsum, return_inverse=True)
    if raw_table is None:
        raw_u = np.array([nbt(float(int(s)), float(m), r) for s in uniq], dtype=np.float64).astype(F32)
    else:
        raw_u = np.array([raw_table[int(s)] for s in uniq], dtype=F32)
    # the raw minimum over the occupied sums, special bins included (a NaN never wins unless all are)
    ok = raw_u[~np.isnan(raw_u)]
    tmin = float(ok.min()) if ok.size else float(raw_u[0])
    med, dele, dup = nbt(RDmedian * m, float(m), r), nbt(RDmedian / 2.0 * float(m), float(m), r), nbt(RDmedian * 1.5 * float(m), float(m), r)
    with np.errstate(all="ignore"):
        med_nbt = np.float64(med) - tmin
        t_u = (raw_u.astype(np.float64) - tmin).astype(F32)
        t_u = (t_u.astype(np.float64) / med_nbt * RDmedian).astype(F32)
        levels = np.array([(np.float64(dele) - tmin) / med_nbt * RDmedian, (np.float64(dup) - tmin) / med_nbt * RDmedian,
                           med_nbt / med_nbt * RDmedian]).astype(F32)
    T = t_u[inv]
    T[:3] = levels
    sel = np.ones(nb, dtype=bool) if mask is None else (np.asarray(mask) == 0)
    # (value, count) pairs: the distinct sums of the selected bins behind bin 2, then the three levels
    body = sel.copy()
    body[:3] = False
    cnt_u = np.bincount(inv[body], minlength=uniq.size).astype(np.int64)
    vals = np.concatenate([t_u, levels])
    cnts = np.concatenate([cnt_u, sel[:3].astype(np.int64)])
    f0, np0, ymin0 = _record(vals, cnts)
    chosen = T[sel]
    med_v, n0, mad_v, n1 = 0.0, 0, 0.0, 0
    if f0 == 0:
        med_v, n0 = _walk(vals[cnts > 0], cnts[cnts > 0], ymin0, np0)
    # the MAD's record: around the record's own median, 0 where that one carries a flag
    dev = gr.abs_dev(vals, med_v if f0 == 0 else 0.0)
    f1, np1, ymin1 = _record(dev, cnts)
    if f0 == NONFINITE or (f0 == 0 and f1 == NONFINITE):
        return Keyed(T, F32(tmin), None, (f0, np0, f1, np1))
    if f0 == EMPTY:
        out = (0.0, 0, 0.0, 0)
    elif (f0 | f1) & TOO_WIDE or f0 == DEGENERATE:      # the host-driven forms, from the array
        out = gr.pair(chosen)
    else:
        if f1 == 0:
            mad_v, n1 = _walk(dev[cnts > 0], cnts[cnts > 0], ymin1, np1)
        elif f1 == DEGENERATE:
            mad_v, n1 = gr.index_order_mean(gr.abs_dev(chosen, med_v)), chosen.size
        out = (med_v, n0, mad_v, n1)
    return Keyed(T, F32(tmin), out, (f0, np0, f1, np1))


def arrays(binsum, m, RDmedian, r, mask=None):
    """The same from the arrays: nb_cases.transform, nb_cases.plan's tests, grid_restatement.pair."""
    binsum = np.asarray(binsum, dtype=np.int64)
    try:
        full = nc.transform(binsum, m, binsum.size * m, RDmedian, r)
        T, tmin = full.T, full.tmin
    except ValueError:
        T, tmin = transform_per_bin(binsum, m, RDmedian, r)
    chosen = gr.selected(T, mask)
    if chosen.size == 0:
        return T, tmin, (0.0, 0, 0.0, 0), (EMPTY, 0)
    f0, np0, _ = nc.plan(chosen)
    if f0 == NONFINITE:
        return T, tmin, None, (f0, np0)
    return T, tmin, gr.pair(chosen), (f0, np0)


# ---- cases ---------------------------------------------------------------------------------------------------------------------------
M, MED, R = 101, 30.0, 7.5
K0 = M * int(MED * 4) + 1           # -m 101 -cap 4 at a median of 30: 12 121 possible sums


def drawn(rng, nb, K=K0, centre=MED * M):
    return np.clip(rng.normal(centre, centre * 0.15, size=nb), 0, K - 1).astype(np.int64)


def _build():
    rng = np.random.default_rng(0x6B657973)
    C = []

    def add(name, b, m=M, K=K0, med=MED, r=R, mask=None, form=1):
        C.append(Case(name, np.asarray(b, dtype=np.int64), m, K, med, r, None if mask is None else np.asarray(mask, dtype=np.int32), form))

    for nb in (8, 9, 1023, 1024, 1025, 4097):
        add(f"nb_{nb}", drawn(rng, nb))
    add("nb_7_no_route", drawn(rng, 7), form=-1)
    same = np.full(600, 2000)
    add("one_sum", same)
    mk = np.zeros(600, dtype=np.int32)
    mk[:3] = 1
    add("one_sum_levels_masked", same, mask=mk)                       # the selection's range is 0: degenerate, the mean on the host
    add("two_sums", np.where(rng.random(700) < 0.4, 2500, 3400))
    add("all_distinct", rng.permutation(4097) + 1000)
    b = drawn(rng, 1500)
    b[10], b[20] = 0, K0 - 1
    add("ends_occupied", b)
    b = drawn(rng, 3000, K=KEY_LIMIT, centre=20000.0)                 # most sums behind the LDS window of the counters
    b[5], b[6] = 0, KEY_LIMIT - 1
    add("k_at_limit", b, K=KEY_LIMIT)
    add("k_above_limit", b, K=KEY_LIMIT + 1, form=-1)
    b = np.maximum(drawn(rng, 1300), 2000)
    b[1] = 0
    add("minimum_on_a_special_bin", b)                                # the raw minimum sees it, the scaled min / max do not
    b = np.minimum(drawn(rng, 1300), 5000)
    b[2] = K0 - 1
    add("maximum_on_a_special_bin", b)
    b = 3029 + rng.integers(0, 400, size=900)                         # the minimum one below the median level's sum: a tiny med_nbt, values spread
    add("too_wide", b)                                                # over millions of buckets -- the host-driven medians follow
    add("non_finite", drawn(rng, 300, K=200, centre=40.0), m=1, K=200, med=40.0, r=0.4)    # m r - 0.5 < 0
    for c in nc.all_cases():
        if c.binsum.size <= 1025 and c.group in ("sizes", "ends"):
            K = int(c.binsum.max()) + 1
            ok = c.binsum.size >= 8 and K <= KEY_LIMIT and int(c.binsum.min()) >= 0
            add("nb_cases_" + c.name, c.binsum, m=c.m, K=K, med=c.RDmedian, r=c.r, form=1 if ok else -1)
    # ---- masks, on one array ----
    b = drawn(rng, 1025)
    n = b.size
    add("mask_all", b, mask=np.ones(n))
    mk = np.ones(n)
    mk[517] = 0
    add("mask_all_but_one", b, mask=mk)
    for k in range(3):
        mk = np.zeros(n)
        mk[k] = 1
        add(f"mask_special_{k}", b, mask=mk)
        mk = (rng.random(n) < 0.3).astype(np.int32)
        mk[:3] = 1
        mk[k] = 0
        add(f"mask_specials_but_{k}", b, mask=mk)
    b2 = b.copy()
    b2[100:160] = 2777
    add("mask_one_key_whole", b2, mask=(b2 == 2777))
    add("mask_moves_the_median", b, mask=(b < np.quantile(b, 0.4)))
    add("mask_random", b, mask=(rng.random(n) < 0.5))
    # ---- a sum outside the table: the launch declines, the chain of launches answers ----
    b = drawn(rng, 1100)
    b[700] = K0
    add("declined", b, form=0)
    add("declined_masked", b, mask=(rng.random(b.size) < 0.2), form=0)
    return C


_cases = None


def all_cases():
    global _cases
    if _cases is None:
        _cases = _build()
        assert len({c.name for c in _cases}) == len(_cases)
    return _cases
