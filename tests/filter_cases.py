"""Inputs for filterstatus alone (rsi.cpp:948-1047 behind a scan pass: the level sums, choose_levels, runs_from_export / prepare_runs and
k_trim_runs) at the edges of its two walks, its run list and its routes: tests/test_filter_cases.py on the CPU, tests/test_filter_edges.py
on the GPU through rsi_hot_debug_filterstatus; the reference's answers: tools/make_golden_filter.py -> golden/filter_edges.npz.

numpy only, seeded.  A case is a Case: name, group, claim (what it was built for, in words), T (float32 bins), status (int32: what the scan
pass left), Lmax, dev, and expect, what the case claims about itself; tests/test_filter_cases.py proves every claim from the restatement
below, never from the library.

Thresholds under control.  Every unmarked bin holds 32.0, whose float sum is exact up to 2^24 terms: the unmarked mean m0 is 32.0 and the
two thresholds are 32 -+ dev in double.  With dev = 4 a DEL bin is trimmed while it is above 28 and a DUP bin while it is below 36: SOLID
bins (10 / 50) stop a walk, SOFT bins (30 / 34) are trimmed.  Every case but those of the level choice ends in a DEL run at a level of its
own, [soft, solid, solid, soft]: its mean of 20 keeps leveldel at or below 0 whatever else the case holds (an absent level inside the
level range holds 0.0 and counts as "below": without such a run a DUP level of 2 and no level 1 would leave the status unfiltered), and it
is the LAST run, which get_continuous_segments never emits -- so every case also states that its two soft bins stay.

The library's constants that place a case are restated here; the CPU test states the derived numbers.
"""
from collections import namedtuple

import numpy as np

Case = namedtuple("Case", "name group claim T status Lmax dev expect")

THREADS = 256                  # positions a walk of k_trim_runs looks at per step
RUNS_INLINE = 200              # kRunsInline: runs that ride in the kernel arguments
EAGER_BOUNDS = 1024            # kEagerBounds: boundary entries (two a run, the last run included) that come back in the mailbox
FS_LIST_CAP = 1 << 20          # kFsListCap: marked bins the device's level sums take
MAX_L, HARD_MAX_L = 10400, 1 << 22   # kMaxL: level sums on the device up to here; kHardMaxL
ROUTE_DEVICE, ROUTE_DECLINED, ROUTE_LONG = 0, 1, 2
F32 = np.float32
FILL = F32(32.0)
DEL_SOLID, DEL_SOFT, DUP_SOLID, DUP_SOFT = F32(10.0), F32(30.0), F32(50.0), F32(34.0)
LMAX = 99                      # 10000 / 101: what a default run scans with


# ---- the reference's filterstatus, restated (rsi.cpp:955-1044) ------------------------------------------------------------------------
def continuous_segments(status):
    """get_continuous_segments(status, 1) (rsi.cpp:291-326): stretches of adjacent marked bins of one sign; the LAST one is never
    emitted.  The loop over the marked bins, as index arithmetic: a run starts where the bin before is unmarked or of the other sign."""
    nz = np.nonzero(status)[0]
    if nz.size == 0:
        return []
    sign = status[nz] > 0
    new = np.ones(nz.size, dtype=bool)
    new[1:] = (np.diff(nz) > 1) | (sign[1:] != sign[:-1])
    first = np.nonzero(new)[0]
    starts = nz[first]
    ends = nz[np.concatenate((first[1:] - 1, [nz.size - 1]))]
    return [(int(s), int(e)) for s, e in zip(starts[:-1], ends[:-1])]


def continuous_segments_loop(status):
    """The same, as the reference's loop reads (used by the CPU test on the small cases)."""
    out, start, end, count = [], 0, 0, 0
    for i in np.nonzero(status)[0]:
        i = int(i)
        if count == 0:
            start = end = i
            count = 1
            continue
        if float(status[i]) * float(status[end]) > 0 and i - end <= 1:
            end = i
            continue
        out.append((start, end))
        start = end = i
        count += 1
    return out


def level_means(T, status):
    """RDsum / RDsumcount over [min status, max status] (rsi.cpp:955-976): per level a float accumulation in index order (np.cumsum in
    float32 adds one element at a time), then float32(sum / double(count)); an absent level holds 0.0."""
    lo, hi = int(status.min()), int(status.max())
    nl = hi - lo + 1
    idx = (status.astype(np.int64) - lo)
    cnt = np.bincount(idx, minlength=nl)
    order = np.argsort(idx, kind="stable")
    sums = np.zeros(nl, dtype=F32)
    pos = 0
    Ts = T[order]
    for l in np.nonzero(cnt)[0]:
        sums[l] = np.cumsum(Ts[pos:pos + cnt[l]], dtype=F32)[-1]
        pos += cnt[l]
    mean = sums.copy()
    present = cnt != 0
    mean[present] = (sums[present].astype(np.float64) / cnt[present].astype(np.float64)).astype(F32)
    return lo, hi, cnt, mean


Filtered = namedtuple("Filtered", "status has_level0 trim leveldel leveladd m0 runs")


def filterstatus_numpy(T, status, dev):
    """filterstatus_tp: the filtered status and what decided it.  has_level0 False: the reference would index RDsum[-minlevel] out of
    range (the library leaves the status as it is); trim False: "status not filtered"."""
    st = status.copy()
    lo, hi, cnt, mean = level_means(T, st)
    if not (lo <= 0 <= hi):
        return Filtered(st, False, False, 0, 0, F32(0), None)
    m0 = mean[-lo]
    m64 = mean.astype(np.float64)
    below = np.nonzero(m64 < float(m0) - dev)[0]            # the first level, from the lowest, whose mean is below m0 - dev
    leveldel = int(below[0]) + lo if below.size else lo
    above = np.nonzero(m64 > float(m0) + dev)[0]            # the last level, from the highest, whose mean is above m0 + dev
    leveladd = int(above[-1]) + lo if above.size else hi
    if leveldel > 0 or leveladd < 0 or leveldel > leveladd:
        return Filtered(st, True, False, leveldel, leveladd, m0, None)
    delthr, addthr = float(m0) - dev, float(m0) + dev
    runs = continuous_segments(st)
    t = T.astype(np.float64)
    for i1, i2 in runs:
        while (t[i1] > delthr and st[i1] < 0) or (t[i1] < addthr and st[i1] > 0):
            st[i1] = 0
            i1 += 1
            if i1 >= i2:
                break
        while (t[i2] > delthr and st[i2] < 0) or (t[i2] < addthr and st[i2] > 0):
            st[i2] = 0
            i2 -= 1
            if i2 <= i1:
                break
    return Filtered(st, True, True, leveldel, leveladd, m0, runs)


def expected_info(case, f):
    """info[0..8] of rsi_hot_debug_filterstatus from the restatement's result f and the restated constants."""
    marked = int(np.count_nonzero(case.status))
    bad = not bool(((case.T >= 0) & (case.T <= F32(3.0e38))).all())
    route = ROUTE_LONG if case.Lmax > MAX_L else (ROUTE_DECLINED if bad or marked > FS_LIST_CAP else ROUTE_DEVICE)
    if f.trim:
        entries = 2 * (len(f.runs) + 1) if marked else 0
        runs, inl, copied = len(f.runs), int(len(f.runs) <= RUNS_INLINE), int(entries > EAGER_BOUNDS)
    else:
        runs = inl = copied = -1
    m0 = int(np.array([f.m0], dtype=F32).view(np.int32)[0]) if f.has_level0 else 0
    return [runs, inl, copied, route, int(f.has_level0), int(f.trim), f.leveldel if f.has_level0 else 0, f.leveladd if f.has_level0 else 0, m0]


# ---- building ------------------------------------------------------------------------------------------------------------------------
def soft_solid(n, level, kept):
    """A run of n bins at `level` (one level or one per bin): soft everywhere but at the offsets `kept`, which are solid."""
    level = np.broadcast_to(np.asarray(level, dtype=np.int32), (n,))
    v = np.where(level < 0, DEL_SOFT, DUP_SOFT).astype(F32)
    k = np.asarray(sorted(kept), dtype=np.int64)
    v[k] = np.where(level[k] < 0, DEL_SOLID, DUP_SOLID)
    return v, level


TAIL_LEVEL = -2


def layout(parts, lead=3, tail_level=TAIL_LEVEL, tail_gap=2, trail=2):
    """parts: [(values, level(s), gap in front)] -> T, status, [(start, end)] of the parts.  Unmarked bins hold 32.0; a gap of 0 puts a
    run against the one before it (they must differ in sign).  tail_level: the DEL run [soft, solid, solid, soft] that ends the case
    (None: no such run), tail_gap bins behind the last part and `trail` unmarked bins behind it."""
    T, st, where = [np.full(lead, FILL, dtype=F32)], [np.zeros(lead, dtype=np.int32)], []
    pos = lead
    parts = list(parts)
    if tail_level is not None:
        parts.append((np.array([DEL_SOFT, DEL_SOLID, DEL_SOLID, DEL_SOFT], dtype=F32), tail_level, tail_gap))
    for k, (values, level, gap) in enumerate(parts):
        values = np.asarray(values, dtype=F32)
        level = np.broadcast_to(np.asarray(level, dtype=np.int32), values.shape)
        g = gap if k > 0 else 0
        T.append(np.full(g, FILL, dtype=F32))
        st.append(np.zeros(g, dtype=np.int32))
        pos += g
        T.append(values)
        st.append(level)
        where.append((pos, pos + values.size - 1))
        pos += values.size
    T.append(np.full(trail, FILL, dtype=F32))
    st.append(np.zeros(trail, dtype=np.int32))
    return np.concatenate(T), np.concatenate(st).astype(np.int32), where


WALK_LENGTHS = (1, 2, 3, 255, 256, 257, 258, 511, 512, 513, 1025, 5000)
KEPT_OFFSETS = (0, 1, 254, 255, 256, 257, -2, -1)     # the one solid bin of a run, from the left; negative: from the right end


def walk_patterns(n):
    """The runs of one length: [(pattern, kept offsets)].  one_k: a single solid bin at offset k -- the left walk stops on it and the
    right walk comes down to the bin above it, so it alone stays; all_soft: the left walk takes every bin but the last, the right walk
    the last; last_solid: the left walk takes all but the last and the last stays; interior: two solid bins with soft bins between
    them, which no walk reaches."""
    pats = [("all_soft", [])]
    seen = set()
    for k in KEPT_OFFSETS:
        k = k if k >= 0 else n + k
        if 0 <= k < n and k not in seen:
            seen.add(k)
            pats.append((f"one_{k}", [k]))
    if n >= 2:
        pats.append(("last_solid", [n - 1]))
    if n >= 5:
        pats.append(("interior", [1, n - 2]))
        pats.append(("interior_wide", [n // 3, n - 1 - n // 3]))
    return pats


_cases = None


def _build():
    C = []

    def add(name, group, claim, parts, Lmax=LMAX, dev=4.0, expect=None, **kw):
        T, st, where = layout(parts, **kw)
        e = dict(expect or {})
        e["where"] = where
        C.append(Case(name, group, claim, T, st, Lmax, float(dev), e))

    # ---- walk geometry: every pattern of a length in one case, DEL and DUP in turn, 0, 1 or 2 bins between the runs -------------------
    for n in WALK_LENGTHS:
        parts, pats = [], []
        for k, (pat, kept) in enumerate(walk_patterns(n)):
            level = -1 if k % 2 == 0 else 1
            v, lv = soft_solid(n, level, kept)
            parts.append((v, lv, (0, 1, 2)[k % 3] if k else 0))
            pats.append((pat, kept))
        add(f"walk_len_{n}", "walks", f"runs of {n} bins: {', '.join(p for p, _ in pats)}", parts, expect=dict(patterns=pats))

    # ---- exact ties and the double threshold ---------------------------------------------------------------------------------------------
    up = np.nextafter(F32(28.0), F32(99))
    dn = np.nextafter(F32(36.0), F32(0))
    add("tie_del_28", "ties", "DEL bins of exactly 28.0 stop both walks; the next float above is trimmed",
        [([up, up, 28.0, up, up, 28.0, up], -1, 0), ([up, up, up], -3, 2)], expect=dict(kept=[[2, 3, 4, 5], []]))
    add("tie_dup_36", "ties", "DUP bins of exactly 36.0 stop both walks; the next float below is trimmed",
        [([dn, dn, 36.0, dn, dn, 36.0, dn], 1, 0), ([dn, dn, dn], 3, 2)], expect=dict(kept=[[2, 3, 4, 5], []]))
    f321 = F32(32.1)
    add("double_threshold_dup", "ties", "dev = 0.1: float32(32.1) is below the double 32.0 + 0.1 and is trimmed; a float comparison keeps it",
        [([f321, f321, 50.0, f321], 1, 0)], dev=0.1, expect=dict(kept=[[2]]))
    f317 = F32(31.7)
    add("double_threshold_del", "ties", "dev = 0.3: float32(31.7) is above the double 32.0 - 0.3 and is trimmed; a float comparison keeps it",
        [([f317, f317, 10.0, f317], -1, 0)], dev=0.3, expect=dict(kept=[[2]]))

    # ---- neighbours, ends, levels ---------------------------------------------------------------------------------------------------------
    d5, _ = soft_solid(5, -1, [2])
    u5, _ = soft_solid(5, 1, [2])
    add("adjacent_del_dup", "neighbours", "a DEL run and a DUP run with no bin between them", [(d5, -1, 0), (u5, 1, 0)], expect=dict(kept=[[2], [2]]))
    add("adjacent_dup_del", "neighbours", "a DUP run and a DEL run with no bin between them", [(u5, 2, 0), (d5, -3, 0)], expect=dict(kept=[[2], [2]]))
    singles = [([DEL_SOFT], -1, 0), ([DUP_SOLID], 1, 0), ([DEL_SOLID], -1, 0), ([DUP_SOFT], 1, 0), ([DEL_SOFT], -3, 0), ([DUP_SOFT], 2, 0)]
    add("single_bin_runs", "neighbours", "runs of one bin against each other, soft and solid", singles, expect=dict(kept=[[], [0], [0], [], [], []]))
    add("run_from_bin_0", "neighbours", "the first run starts on bin 0", [(d5, -1, 0)], lead=0, expect=dict(kept=[[2]]))
    add("all_soft_from_bin_0", "neighbours", "a run of soft bins from bin 0: every bin goes", [(soft_solid(300, 1, [])[0], 1, 0)], lead=0, expect=dict(kept=[[]]))
    add("last_run_on_last_bin", "neighbours", "the last run ends on the last bin: never trimmed; the run before it is", [(u5, 1, 0)], trail=0,
        expect=dict(kept=[[2]]))
    add("last_run_against_the_one_before", "neighbours", "the last run lies against the run before it", [(u5, 1, 0)], tail_gap=0, expect=dict(kept=[[2]]))
    lv = np.array([-3] * 4 + [-7] * 4 + [-3] * 4, dtype=np.int32)
    v, _ = soft_solid(12, lv, [5, 6])
    add("levels_3_and_7", "neighbours", "levels -3 and -7 in one run", [(v, lv, 0)], expect=dict(kept=[[5, 6]]))
    v, _ = soft_solid(600, -1, [400])
    v[100] = np.nan
    add("nan_stops_a_walk", "neighbours", "a NaN bin inside a run stops the left walk; the level sums go to the host loop", [(v, -1, 0)],
        expect=dict(kept=[list(range(100, 401))]))

    # ---- the run list: inline / pointers, eager / copied -----------------------------------------------------------------------------------
    rng = np.random.default_rng(0xF17E01)

    def short_runs(k):
        parts = []
        for i in range(k):
            n = int(rng.integers(1, 6))
            level = int(rng.choice([-5, -3, -1])) if i % 2 else int(rng.choice([1, 2, 4]))
            kept = [j for j in range(n) if rng.random() < 0.4]
            parts.append((soft_solid(n, level, kept)[0], level, int(rng.integers(0, 3)) if i else 0))
        return parts
    for k in (1, 2, 200, 201, 511, 512, 513, 3000):
        add(f"runs_{k}", "lists", f"{k} runs of 1..5 bins behind the drop", short_runs(k), expect=dict(runs=k))
    C.append(Case("no_marked_bin", "lists", "no marked bin at all", np.full(700, FILL, dtype=F32), np.zeros(700, dtype=np.int32), LMAX, 4.0,
                  dict(where=[], runs=0)))
    add("one_run_only", "lists", "one run: it is the last, nothing is trimmed", [], expect=dict(runs=0))

    # ---- the level choice --------------------------------------------------------------------------------------------------------------------
    add("level_gap", "levels", "levels -5, -3, 0, 2: -5 is not below m0 - dev, the absent -4 holds 0.0 and is: leveldel = -4",
        [(soft_solid(6, -5, [])[0], -5, 0), (soft_solid(6, 2, [3])[0], 2, 2)], tail_level=-3,
        expect=dict(kept=[[], [3]], leveldel=-4, leveladd=2, levels=[-5, -3, 0, 2]))
    add("not_filtered", "levels", "a DUP level whose mean is below m0 - dev: leveldel = 1, the status comes back as it went in",
        [(np.array([20.0, 20.0, 34.0], dtype=F32), 1, 0), (np.array([34.0, 20.0, 34.0], dtype=F32), 1, 2)], tail_level=None,
        expect=dict(trim=False, leveldel=1))
    C.append(Case("no_unmarked_bin", "levels", "every bin is a DEL bin: no level 0, the status comes back as it went in",
                  soft_solid(500, -1, [250])[0], np.full(500, -1, dtype=np.int32), LMAX, 4.0, dict(where=[(0, 499)], has_level0=False)))

    # ---- routes: each with runs that need trimming ---------------------------------------------------------------------------------------
    v, _ = soft_solid(40, -1, [20])
    v[21] = F32(-5.0)
    add("negative_bin", "routes", "a negative bin: the device declines, the host loop runs", [(v, -1, 0), (u5, 1, 3)], expect=dict(kept=[[20, 21], [2]]))
    for name, extra in (("marked_at_cap", 0), ("marked_beyond_cap", 1)):
        # eight runs of 131 071 bins and the tail's four are 2^20 - 4 marked bins; a ninth run brings them to 2^20 (+ 1)
        parts = []
        for k, depth in enumerate((0, 1, 255, 256, 257, 5000, 70000, 131070)):
            n = 131071
            kept = [depth, n - 1 - min(depth, 3)] if k < 7 else [depth]     # the last one: its last bin alone is solid
            parts.append((soft_solid(n, -1 if k % 2 == 0 else 1, kept)[0], -1 if k % 2 == 0 else 1, k % 3))
        parts.append((soft_solid(4 + extra, 3, [1])[0], 3, 1))
        add(name, "routes", f"2^20 {'+ 1 ' if extra else ''}marked bins: the device's list {'overflows, the host loop runs' if extra else 'holds them'}", parts)
    for L in (MAX_L, MAX_L + 1):
        lv = np.array([-L, -1, -1, -1, -1, -1], dtype=np.int32)
        lu = np.array([1, 1, 1, 1, 1, L], dtype=np.int32)
        add(f"lmax_{L}", "routes", f"Lmax = {L}, with bins at levels -Lmax and +Lmax", [(soft_solid(6, lv, [3])[0], lv, 0), (soft_solid(6, lu, [2])[0], lu, 1)],
            Lmax=L, expect=dict(kept=[[3], [2]]))
    return C


def all_cases():
    global _cases
    if _cases is None:
        _cases = _build()
        assert len({c.name for c in _cases}) == len(_cases)
    return _cases


def get_case(name):
    return next(c for c in all_cases() if c.name == name)


def golden_cases():
    """Every case the reference can run: without an unmarked level it indexes its level sums out of range."""
    return [c for c in all_cases() if c.name != "no_unmarked_bin"]
