"""Inputs for ONE scan pass (rsistatus, rsi.cpp:1191-1259) at its edges: tests/test_scan_cases.py on the CPU, tests/test_scan_edges.py
on the GPU through rsi_hot_debug_scan; the reference's answers: tools/make_golden_scan.py -> golden/scan_edges.npz.

numpy only, seeded.  A case is a Case: name, group, T (float32 bins), medint (int32 bin medians), RDmedian, tmedian, tlamda, Lmax, and

* ref      True: the expected status is the reference's (the golden file).  Such a case keeps all four trimming walks of every hit
           inside [0, nb) -- walks_inside() proves it with the bounded restatement BEFORE the reference is called: the reference
           walks off the array there.  False: the reference has no behaviour (the escapes) or is not the yardstick (exactness (a));
* expect   what the case claims about itself; tests/test_scan_cases.py proves every claim from the reference's arithmetic restated
           here (ref_score, first_marks, resolve), never from the library.

The library's constants that place a case (tile 256, detection workgroup 1024, thresholds in the kernel arguments up to Lmax 223,
LDS tile up to 3800, kMaxL 10 400, the mark levels' cap) are restated below; the CPU test states the derived numbers.

Left out: the scan forms beyond 13 200 lengths (per-L counts in device memory past 20 000, 32-bit staged indices past 32 000: they stay
with the long tests of test_hot_extra.py), NaN and infinite bins.
"""
import math
from collections import namedtuple

import numpy as np

Case = namedtuple("Case", "name group T medint RDmedian tmedian tlamda Lmax ref expect")

TILE, DET_BINS, THREADS, SCAN_PAD = 256, 1024, 256, 8
THR_INLINE_L = 232 - SCAN_PAD - 1   # 223: thresholds ride in the kernel arguments
SCAN_LDS_L, MAX_L, BOTH_CAP = 3800, 10_400, 16_384
LDS_BYTES = 160 * 1024
F32 = np.float32


# ---- the library's shapes, restated (kernels_bin.hip: scan_lds_bytes, scan_tile_shape, detect_lds_bytes, launch_rsi_scan) -----------
def scan_lds_bytes(count, kcap, ix_bytes=2):
    return ((count + 1) + THREADS) * 8 + 2 * (kcap + 1) * count * 4 + count * 4 + 9 * (count + 2) * ix_bytes


def kcap_for(Lmax):
    count = TILE + 2 * (Lmax // 2 + 1)
    k = 0
    while (2 << k) <= Lmax and k < 6:
        k += 1
    if Lmax <= SCAN_LDS_L:
        while k > 0 and scan_lds_bytes(count, k) + 4 * THREADS * 4 + 1024 > LDS_BYTES:
            k -= 1
    return k


def detect_lds_bytes(Lmax):
    count = DET_BINS + 2 * (Lmax // 2 + 1)
    return (Lmax + 1 + SCAN_PAD) * 8 + ((count + 2) & ~1) * 4 + 16


def detect_runs(Lmax):
    return detect_lds_bytes(Lmax) + THREADS * 8 + 64 <= LDS_BYTES


def max_parts(Lmax):
    return min(8, (Lmax + SCAN_PAD - 1) // SCAN_PAD)


# ---- the reference's arithmetic, restated -----------------------------------------------------------------------------------------
def ref_score(window, tmedian):
    """((float)(sum / L) - tmedian) * sqrt(L) as rsistatus forms it from runmeantp's mean (rsi.cpp:1205, wufunctions.cpp:628-630), for a
    window whose sliding sum is exact (the callers keep the values on a common grid): the sum is then math.fsum's."""
    L = len(window)
    s = math.fsum(float(x) for x in window)
    return (float(F32(s / L)) - tmedian) * math.sqrt(float(L))


def np_median(a):
    return float(np.median(np.asarray(a, dtype=np.int64)))


def score_hits(T, tmedian, tlamda, Lmax):
    """[(L, centre)] per sweep (0 DEL, 1 DUP), lengths then positions ascending, by the reference's own sliding double sums."""
    nb = T.size
    y = T.astype(np.float64)
    Ls = np.arange(1, Lmax + 1)
    h = Ls // 2
    rootL = np.sqrt(Ls.astype(np.float64))
    sums = np.cumsum(y)[Ls - 1].copy()
    out = {0: [], 1: []}
    for first in range(1, nb):
        last = first + Ls - 1
        live = last < nb
        if not live.any():
            break
        sums[live] = sums[live] - y[first - 1] + y[last[live]]
        smo = (sums / Ls).astype(np.float32).astype(np.float64)
        i = h + first
        scan = live & (i >= h + 1) & (i < nb - h - 1)
        score = (smo - tmedian) * rootL
        for sweep, cond in ((0, score <= -tlamda), (1, score >= tlamda)):
            for k in np.nonzero(scan & cond)[0]:
                out[sweep].append((int(Ls[k]), int(i[k])))
    for s in out:
        out[s].sort()
    return out


def first_marks(case, exact_median=np_median):
    """The two sweeps WITHOUT the stop rule and without precedence: fd[j] / fu[j] = the smallest L whose trimmed interval reaches bin j
    (0: none) -- what the kernels keep before k_level_stop.  Walks are bounded (a walk that leaves the array marks nothing).  Also
    counts: straddles (even L, exactly L/2 bins beyond the median limit: the test needs the middle pair), escapes, hits, empty
    (trimmed intervals with i1 > i2), outside (a walk that ended outside its window), cross_tile (a hit centred in one tile of
    256 bins whose interval lies in another; cross_fwd / cross_back per sweep: in the next / the previous tile), win_starts / win_ends
    (first and last bins of the windows that passed the median test), value_moved / median_moved / both_moved (walks that left
    their starting bin; both at one end of one hit), full_lanes (centres that hit at every L of a sweep), lengths / aligns (the set of
    interval lengths, and of their starts modulo 64)."""
    T, medint, nb = case.T, case.medint, case.T.size
    hits = score_hits(T, case.tmedian, case.tlamda, case.Lmax)
    first = [np.zeros(nb, dtype=np.int64), np.zeros(nb, dtype=np.int64)]
    stat = dict(straddles=0, escapes=0, hits=[len(hits[0]), len(hits[1])], empty=0, outside=0, passed=0, cross_tile=0, full_lanes=0,
                lengths=set(), aligns=set(), cross_fwd=[0, 0], cross_back=[0, 0], win_starts=set(), win_ends=set(), value_moved=0,
                median_moved=0, both_moved=0)
    for sweep in (0, 1):
        per_lane = {}
        for L, pos in hits[sweep]:
            per_lane[pos] = per_lane.get(pos, 0) + 1
        stat["full_lanes"] += sum(1 for n in per_lane.values() if n == case.Lmax)
    for sweep in (0, 1):
        dele = sweep == 0
        lim = case.RDmedian * (0.75 if dele else 1.25)
        walks_on = (T > case.tmedian, medint > lim) if dele else (T < case.tmedian, medint < lim)
        stops = [np.flatnonzero(~w) for w in walks_on]               # where the value walk / the median walk stops, ascending

        def walk_up(q, j):      # `while walks_on[q][j]: j += 1`, nb when it never stops
            k = int(np.searchsorted(stops[q], j))
            return int(stops[q][k]) if k < stops[q].size else nb

        def walk_down(q, j):    # `while walks_on[q][j]: j -= 1`, -1 when it never stops
            k = int(np.searchsorted(stops[q], j, side="right")) - 1
            return int(stops[q][k]) if k >= 0 else -1
        for L, pos in hits[sweep]:
            i1 = pos - L // 2
            i2 = i1 + L - 1
            w = medint[i1:i2 + 1]
            beyond = int(np.count_nonzero(w <= lim)) if dele else int(np.count_nonzero(w >= lim))
            if L % 2 == 0 and beyond == L // 2:
                stat["straddles"] += 1
            wm = exact_median(w)
            if (wm > lim) if dele else (wm < lim):
                continue
            stat["passed"] += 1
            a, b = i1, i2
            v1 = walk_up(0, i1)
            i1 = walk_up(1, v1) if v1 < nb else nb
            v2 = walk_down(0, i2)
            i2 = walk_down(1, v2) if v2 >= 0 else -1
            if i1 >= nb or i2 < 0:
                stat["escapes"] += 1
                continue
            stat["win_starts"].add(a)
            stat["win_ends"].add(b)
            stat["value_moved"] += (v1 != a) + (v2 != b)
            stat["median_moved"] += (i1 != v1) + (i2 != v2)
            stat["both_moved"] += (v1 != a and i1 != v1) + (v2 != b and i2 != v2)
            if i1 > b or i2 < a:
                stat["outside"] += 1
            if i1 > i2:
                stat["empty"] += 1
                continue
            stat["lengths"].add(i2 - i1 + 1)
            stat["aligns"].add(i1 % 64)
            if i1 // TILE == i2 // TILE != pos // TILE:
                stat["cross_tile"] += 1
                stat["cross_fwd" if pos // TILE < i1 // TILE else "cross_back"][sweep] += 1
            seg = first[sweep][i1:i2 + 1]
            seg[seg == 0] = L
    return first[0], first[1], stat


def resolve(fd, fu, Lmax):
    """Stop rule and precedence from the first-L arrays, as k_level_stop / resolved_status apply them: (status, ldel, ldup, both,
    marked) with marked[sweep] = {L: bins counted after length L} up to the stop."""
    nb = fd.size
    marked = [{}, {}]

    def sweep_stop(first, blocked, rec):
        cum = 0
        for L in range(1, Lmax + 1):
            cum += int(np.count_nonzero((first == L) & ~blocked))
            rec[L] = cum
            if float(cum) / float(nb) > 0.2:
                return L
        return Lmax

    none = np.zeros(nb, dtype=bool)
    ldel = sweep_stop(fd, none, marked[0])
    is_del = (fd > 0) & (fd <= ldel)
    ldup = sweep_stop(fu, is_del, marked[1])
    is_dup = ~is_del & (fu > 0) & (fu <= ldup)
    st = np.where(is_del, -fd, np.where(is_dup, fu, 0)).astype(np.int32)
    both = int(np.count_nonzero((fd > 0) & (fu > 0)))
    return st, ldel, ldup, both, marked


def walks_inside(case, exact_median=np_median):
    """No trimming walk of any hit the reference would replay leaves [0, nb): the bounded restatement counts none."""
    from scan_restatement import rsistatus_numpy
    _, esc = rsistatus_numpy(case.T, case.medint, case.RDmedian, case.tmedian, case.tlamda, case.Lmax, exact_median, bounded=True)
    return esc == 0


# ---- the exactness flag, restated (kernels_bin.hip: ScanExact) -----------------------------------------------------------------------
def pow2_of(av):
    """The power of two of a non-zero finite float |v| (2^-126 for a subnormal)."""
    m, e = math.frexp(float(av))
    return 2.0 ** max(e - 1, -126)


def inexact_expected(T, Lmax, detect):
    """info[2] for these bins: per workgroup (detect: 1024 owned bins, else 256) the stretch is the owned bins and Lmax/2+1 bins each
    side; it is flagged when sum |v| >= 2^30 pow2(smallest non-zero |v|); a flagged stretch counts its owned non-zero bins with
    2^30 pow2(|v|) <= sum |v|, or 1 when none is owned.  Sums are math.fsum's.  The cases keep every bin but the smallest
    away from its own bound: there the kernel's double sum may be rounded."""
    nb, halo, own = T.size, Lmax // 2 + 1, (DET_BINS if detect else TILE)
    a = np.abs(T.astype(np.float64))
    p2 = np.where(a > 0, 2.0 ** np.maximum(np.frexp(a)[1] - 1, -126), np.inf)      # pow2_of, per bin
    total = 0
    for first in range(0, nb, own):
        lo, hi = max(0, first - halo), min(nb, first + own + halo)
        if not (a[lo:hi] > 0).any():
            continue
        asum = math.fsum(a[lo:hi])      # correctly rounded, and every bound is a power of two: asum >= bound as for the exact sum
        if asum < 2.0 ** 30 * p2[lo:hi].min():
            continue
        mine = slice(first, min(nb, first + own))
        owned = int(np.count_nonzero((a[mine] > 0) & (2.0 ** 30 * p2[mine] <= asum)))
        total += owned if owned else 1
    return total


# ---- building blocks ---------------------------------------------------------------------------------------------------------------
def flat(nb, t=40.0, m=40):
    return np.full(nb, t, dtype=F32), np.full(nb, m, dtype=np.int32)


def put(T, medint, a, b, t, m):
    """bins [a, b) get value t and median m"""
    T[a:b] = F32(t)
    medint[a:b] = m


def case(name, group, T, medint, RDmedian, tmedian, tlamda, Lmax, ref=True, **expect):
    assert T.dtype == F32 and medint.dtype == np.int32 and T.size == medint.size and 1 <= Lmax <= T.size
    return Case(name, group, T, medint, float(RDmedian), float(tmedian), float(tlamda), int(Lmax), ref, expect)


# ---- threshold ties ----------------------------------------------------------------------------------------------------------------
TIE_LENGTHS = (1, 2, 3, 4, 7, 8, 9, 16, 99, 196, 223, 224)


def tie_windows(L, sweep, tmedian, tlamda):
    """Three windows of L float bins: A, the last that still hits when one bin is stepped with nextafter; B, one float step of that bin
    beyond (no hit); C, one step inside (hit).  Found under the reference's own expression (ref_score), never the library's
    thresholds."""
    sign = -1.0 if sweep == 0 else 1.0
    away = F32(np.inf) * F32(-sign)        # towards tmedian: out of the hit region
    into = F32(np.inf) * F32(sign)

    def hit(w):
        s = ref_score(w, tmedian)
        return s <= -tlamda if sweep == 0 else s >= tlamda

    w = np.full(L, F32(tmedian + sign * tlamda / math.sqrt(L)), dtype=F32)
    for _ in range(1 << 16):
        if hit(w):
            break
        w[0] = np.nextafter(w[0], into)
    assert hit(w)
    for _ in range(1 << 16):
        nxt = w.copy()
        nxt[0] = np.nextafter(nxt[0], away)
        if not hit(nxt):
            break
        w = nxt
    A, B, C = w.copy(), w.copy(), w.copy()
    B[0] = np.nextafter(A[0], away)
    C[0] = np.nextafter(A[0], into)
    assert hit(A) and not hit(B) and hit(C)
    return A, B, C


def tie_case(L, sweep, big):
    """Each window alone in a flat chromosome: shorter windows inside it and longer ones around it score strictly less, so the
    detection pass has to list its tile for that one (bin, L)."""
    tmedian, tlamda = (524288.0, 65536.0) if big else (40.0, 10.0)
    Lmax = 224 if L == 224 else 223
    A, B, C = tie_windows(L, sweep, tmedian, tlamda)
    nb, starts = 2500, (300, 1100, 1900)
    T, medint = flat(nb, tmedian, 40)
    for s, w in zip(starts, (A, B, C)):
        T[s:s + L] = w
        medint[s:s + L] = 20 if sweep == 0 else 60
    name = f"tie_{'big' if big else 'mid'}_{'del' if sweep == 0 else 'dup'}_L{L}"
    return case(name, "ties", T, medint, 40.0, tmedian, tlamda, Lmax, L=L, sweep=sweep, starts=starts, hit=(True, False, True),
                escapes=0, inexact=0)


# ---- tiles and ends ------------------------------------------------------------------------------------------------------------------
def tile_case(Lmax, long_form, edge, family):
    """A deletion on the first tile edge (edge = 255 / 256 / 257) and a duplication on the edge of a detection workgroup's four tiles,
    768 bins on (1023 / 1024 / 1025); family 0: the deletion ends on its edge and the duplication starts on its own, family 1 the
    other way round; and a short deletion in the last, partial tile.  nb = 3300: the detection workgroup of bins 1024 ... 2047 is an
    interior one, the first and the last reach a chromosome end.  Short events (about Lmax / 2 bins) are seen by windows centred in
    the neighbouring tile; long ones (Lmax + 40) make every lane inside run a full run of hits.  The event that STARTS on an edge
    is preceded by six bins with its median and a value just past tmedian: a window centred in the tile before it then passes the
    median test, the value walk passes over those bins, and the hit marks only bins of the next tile, through the halo (without
    them such a window holds the event in less than half of its bins).  The event that ends on an edge is reached from the tile
    behind it as it is: an even window reaches one bin further left than right.
    One placement cannot exist: a long event at Lmax 224 (264 bins) that ends on bin 255 / 256 / 257."""
    ln = Lmax + 40 if long_form else max(3, Lmax // 2)
    nb = 3300
    T, medint = flat(nb)
    e2 = edge + 768
    assert family == 1 or edge - ln + 1 >= 3
    if family == 0:          # DEL ends on the edge, DUP starts on the second
        put(T, medint, edge - ln + 1, edge + 1, 30.0, 20)
        put(T, medint, e2 - 6, e2, 39.0, 60)
        put(T, medint, e2, e2 + ln, 50.0, 60)
    else:                    # DEL starts on the edge, DUP ends on the second
        put(T, medint, edge - 6, edge, 41.0, 20)
        put(T, medint, edge, edge + ln, 30.0, 20)
        put(T, medint, e2 - ln + 1, e2 + 1, 50.0, 60)
    put(T, medint, nb - 60, nb - 45, 28.0, 20)
    name = f"tile_L{Lmax}_{'long' if long_form else 'short'}_e{edge}_{'ends' if family == 0 else 'starts'}"
    return case(name, "tiles", T, medint, 40.0, 40.0, 10.0, Lmax, escapes=0, inexact=0, event_len=ln, edge=edge, family=family)


def ends_case(Lmax, k, long_form):
    """A deletion that starts on bin k and a duplication that ends on bin nb - 1 - k (k = 0, 1, 2): the reference centres windows on i
    in [L/2 + 1, nb - L/2 - 2], so the outermost bins are reached through trimmed intervals only, if at all."""
    ln = Lmax + 40 if long_form else max(4, Lmax // 2)
    nb = 700
    T, medint = flat(nb)
    put(T, medint, k, k + ln, 30.0, 20)
    put(T, medint, nb - k - ln, nb - k, 50.0, 60)
    return case(f"ends_L{Lmax}_{'long' if long_form else 'short'}_k{k}", "tiles", T, medint, 40.0, 40.0, 10.0, Lmax, escapes=0, inexact=0)


def small_nb_case(nb, Lmax):
    T, medint = flat(nb)
    if nb >= 4:
        a = max(1, nb // 3)
        put(T, medint, a, min(nb - 1, a + max(1, min(40, nb // 4))), 25.0, 20)
    if nb >= 200:
        put(T, medint, nb - 30, nb - 2, 55.0, 60)
    return case(f"small_nb{nb}_L{Lmax}", "tiles", T, medint, 40.0, 40.0, 10.0, Lmax, escapes=0, inexact=0)


# ---- the median test ---------------------------------------------------------------------------------------------------------------
def median_limits_case(RDmedian):
    """Events whose bin medians sit on floor(lim), floor(lim) + 1, ceil(lim) - 1, ceil(lim) of each sweep's limit (0.75 / 1.25 RDmedian:
    an integer at 40, not at 41 and 30.5), 12 bins each, under Lmax = 20: longer windows take in background medians."""
    nb = 1000
    T, medint = flat(nb, 40.0, int(RDmedian))
    ld, lu = RDmedian * 0.75, RDmedian * 1.25
    vals = [(0, v) for v in (math.floor(ld), math.floor(ld) + 1, math.ceil(ld) - 1, math.ceil(ld))] + \
           [(1, v) for v in (math.floor(lu), math.floor(lu) + 1, math.ceil(lu) - 1, math.ceil(lu))]
    for k, (sweep, v) in enumerate(vals):
        a = 60 + 110 * k
        put(T, medint, a, a + 12, 20.0 if sweep == 0 else 60.0, int(v))
    return case(f"median_limits_rd{RDmedian}", "median", T, medint, RDmedian, 40.0, 10.0, 20, escapes=0, inexact=0,
                medians=[v for _, v in vals])


def median_pairs_case():
    """Even windows with exactly L/2 bins beyond the limit (RDmedian 40: 30 and 50) whose middle pair averages to the limit, just below
    and just above it: an event of 2k deep bins, the first k with the near median, the last k with the far one."""
    nb = 1400
    T, medint = flat(nb)
    pairs = [(0, 29, 31), (0, 28, 31), (0, 29, 32), (0, 30, 31), (1, 49, 51), (1, 49, 52), (1, 48, 51), (1, 49, 50)]
    spots = []
    for n, (sweep, lo, hi) in enumerate(pairs):
        for j, k in enumerate((1, 2, 5)):
            a = 50 + 160 * n + 50 * j
            near, far = (lo, hi) if sweep == 0 else (hi, lo)
            put(T, medint, a, a + k, 20.0 if sweep == 0 else 60.0, near)
            put(T, medint, a + k, a + 2 * k, 20.0 if sweep == 0 else 60.0, far)
            spots.append((sweep, a, 2 * k, 0.5 * (lo + hi)))
    return case("median_pairs", "median", T, medint, 40.0, 40.0, 10.0, 20, escapes=0, inexact=0, spots=spots, min_straddles=24)


MID_LANE = 300     # the lane of median_mid_case


def median_mid_case():
    """One lane (centre MID_LANE) whose even windows straddle at L = 4, do not at 6 and 8 (four of six, five of eight bins beyond the
    limit), and straddle again at 10 and 12 with another pair: the incrementally kept ScanMid has to pick the pair up again."""
    nb = 700
    T, medint = flat(nb)
    i = MID_LANE
    put(T, medint, i - 6, i + 6, 20.0, 35)                     # twelve deep bins, medians above 30 unless set below
    for off, m in ((-2, 25), (0, 25), (-1, 35), (1, 35),       # L = 4: two of four; pair (25, 35) -> 30.0, passes by equality
                   (-3, 29), (2, 29),                          # L = 6: four of six
                   (-4, 27), (3, 33),                          # L = 8: five of eight
                   (-5, 32), (4, 32),                          # L = 10: five of ten; pair (29, 32) -> 30.5, fails
                   (-6, 30), (5, 31)):                         # L = 12: six of twelve; pair (30, 31) -> 30.5, fails
        medint[i + off] = m
    return case("median_mid_lane", "median", T, medint, 40.0, 40.0, 10.0, 20, escapes=0, inexact=0,
                lane=i, beyond={4: 2, 6: 4, 8: 5, 10: 5, 12: 6})


def median_random_case(RDmedian, seed):
    """Deep events whose medians are drawn from floor(lim) - 1 ... floor(lim) + 2: straddling tests are frequent."""
    rng = np.random.default_rng(seed)
    nb = 1500
    T, medint = flat(nb, 40.0, int(RDmedian))
    for n in range(6):
        sweep = n % 2
        lim = RDmedian * (0.75 if sweep == 0 else 1.25)
        a = 80 + 230 * n
        ln = int(rng.integers(25, 60))
        T[a:a + ln] = F32(15.0 if sweep == 0 else 65.0)
        medint[a:a + ln] = rng.integers(math.floor(lim) - 1, math.floor(lim) + 3, size=ln)
    return case(f"median_random_rd{RDmedian}", "median", T, medint, RDmedian, 40.0, 10.0, 20, escapes=0, inexact=0, min_straddles=100)


# ---- trim walks ----------------------------------------------------------------------------------------------------------------------
def trim_predicates_case(seed):
    """Events in which single bins carry only one of the two predicates of a walk (DEL: value <= tmedian, median <= limit), or the value
    exactly tmedian (the walk stops there in both sweeps): at both ends of the event -- the gained end of a run of hits -- and
    inside.  The reference walks the value first, then the median."""
    rng = np.random.default_rng(seed)
    nb = 1600
    T, medint = flat(nb)
    events = []
    for n in range(8):
        sweep = n % 2
        a, ln = 90 + 180 * n, 40 + 3 * n
        events.append((sweep, a, ln))
        deep, near, far, past = (22.0, 20, 40, 45.0) if sweep == 0 else (58.0, 60, 40, 35.0)
        put(T, medint, a, a + ln, deep, near)
        kinds = rng.integers(0, 8, size=ln)
        kinds[:3] = (1, 2, 3)[n % 3], (2, 3, 1)[n % 3], 0
        kinds[-3:] = 0, (3, 1, 2)[n % 3], (1, 2, 3)[n % 3]
        for j, k in enumerate(kinds):
            if k == 1: medint[a + j] = far                  # only the value predicate holds
            if k == 2: T[a + j] = F32(past)                 # only the median predicate holds
            if k == 3: T[a + j] = F32(40.0)                 # exactly tmedian
    return case(f"trim_predicates_s{seed}", "trim", T, medint, 40.0, 40.0, 10.0, 20, escapes=0, inexact=0, events=events)


def trim_outside_case(dist, Lmax=20, at=700, nb=1500):
    """A window whose forward median walk finds its bin only `dist` bins beyond the window (inside the halo of the tile, or beyond it),
    and the mirror image for the backward walk: four bins just above tmedian with a deletion's median, then four bins at 0 with the
    background's.  Both intervals are empty: the other walk has stopped inside the window."""
    T, medint = flat(nb)
    for a, mirror in ((at, False), (at + 300, True)):
        first, second = (slice(a, a + 4), slice(a + 4, a + 8)) if not mirror else (slice(a + 4, a + 8), slice(a, a + 4))
        T[first] = F32(41.0); medint[first] = 20
        T[second] = F32(0.0); medint[second] = 40
        c = a + 8 + dist if not mirror else a - 1 - dist
        medint[c] = 20                                       # the bin that catches the walk (value tmedian, a deletion's median)
    return case(f"trim_outside_d{dist}", "trim", T, medint, 40.0, 40.0, 10.0, Lmax, escapes=0, inexact=0, min_outside=2, min_empty=2)


def escape_case(side):
    """trim_outside without the catching bin, at a chromosome end: the median walk finds no bin before the array ends.  The reference
    reads past the array there; the library marks nothing and counts the walk (divergence 1)."""
    nb = 600
    T, medint = flat(nb)
    if side == 0:      # forward walk off the end
        a = nb - 40
        T[a:a + 4] = F32(41.0); medint[a:a + 4] = 20
        T[a + 4:a + 8] = F32(0.0); medint[a + 4:a + 8] = 40
    else:              # backward walk off the start
        a = 30
        T[a + 4:a + 8] = F32(41.0); medint[a + 4:a + 8] = 20
        T[a:a + 4] = F32(0.0); medint[a:a + 4] = 40
    put(T, medint, 300, 310, 25.0, 20)                       # an ordinary event next to it
    return case(f"escape_{'end' if side == 0 else 'start'}", "escapes", T, medint, 40.0, 40.0, 10.0, 20, ref=False, inexact=0, min_escapes=1)


# ---- marks ---------------------------------------------------------------------------------------------------------------------------
def marks_lengths_case(offset):
    """Isolated events of every length 1 ... 2 * 64 + 3, each seen by windows of about its own length only (depth 10.5 / sqrt(len) under
    tlamda 10), so the trimmed intervals have every length; the running position puts them at every alignment against the 64-bin
    blocks of the mark levels, `offset` shifts all of them."""
    Lmax, gap = 131, 150
    lens = list(range(1, 2 * 64 + 4))
    nb = offset + 200 + sum(lens) + gap * len(lens) + 200
    T, medint = flat(nb)
    a, spots = offset + 200, []
    for ln in lens:
        put(T, medint, a, a + ln, 40.0 - 10.5 / math.sqrt(ln), 20)
        spots.append((a, ln))
        a += ln + gap
    return case(f"marks_lengths_o{offset}", "marks", T, medint, 40.0, 40.0, 10.0, Lmax, escapes=0, inexact=0, spots=spots, kcap=6)


def marks_nested_case():
    """Overlapping intervals from different L: a shallow plateau (seen from L = 25 on) around narrow deep events (seen at L = 1): the
    smallest L wins bin by bin."""
    nb = 900
    T, medint = flat(nb)
    put(T, medint, 200, 330, 38.0, 20)
    put(T, medint, 250, 255, 20.0, 20)
    put(T, medint, 300, 301, 10.0, 20)
    put(T, medint, 500, 640, 42.0, 60)
    put(T, medint, 560, 563, 60.0, 60)
    return case("marks_nested", "marks", T, medint, 40.0, 40.0, 10.0, 99, escapes=0, inexact=0)


# Lmax -> the cap of the mark levels there: floor(log2(Lmax)) up to 6, lowered where the LDS tile would not fit (scan_tile_shape)
KCAP_LMAX = {1: 0, 3: 1, 7: 2, 15: 3, 31: 4, 63: 5, 64: 6, 1563: 6, 1564: 5, 1752: 4, 1980: 3, 2270: 2, 2644: 1, 3148: 0}


def two_events_and_tie(name, group, Lmax, **expect):
    """nb = Lmax + 400 bins: two short events and one tie window (length 9)."""
    nb = Lmax + 400
    T, medint = flat(nb)
    put(T, medint, nb // 3, nb // 3 + 12, 30.0, 20)
    put(T, medint, 2 * nb // 3, 2 * nb // 3 + 17, 50.0, 60)
    L = min(9, Lmax)
    A, _, _ = tie_windows(L, 0, 40.0, 10.0)
    s = nb // 2
    T[s:s + L] = A
    medint[s:s + L] = 20
    return case(name, group, T, medint, 40.0, 40.0, 10.0, Lmax, escapes=0, inexact=0, tie_start=s, tie_L=L, **expect)


# ---- stop rule and precedence --------------------------------------------------------------------------------------------------------
def fifth_case(sweep, Lmax):
    """nb = 1000: 200 single deep bins (a fifth, marked at L = 1: portion > 0.2 is false, the sweep goes on), then ONE more bin at L = 2
    (201: it stops there), and an event only L >= 5 sees, which stays unmarked.  The one bin: two bins of 32.9 (no hit at L = 1, a hit
    at L = 2), the first with a deletion's median, the second with the background's -- the window median 30 passes by equality and
    the median walk trims the second bin away.  For the DUP sweep the mirror image, next to a deletion of 150 bins that the DEL
    sweep keeps and the DUP count must leave out."""
    nb = 1000
    T, medint = flat(nb)
    up = sweep == 1
    deep, m = (55.0, 60) if up else (25.0, 20)
    for j in range(200):
        put(T, medint, 100 + 3 * j + (j // 50) * 20, 100 + 3 * j + (j // 50) * 20 + 1, deep, m)
    put(T, medint, 20, 22, 47.1 if up else 32.9, m)
    medint[21] = 40
    put(T, medint, 50, 58, 44.5 if up else 35.5, m)
    if up:
        put(T, medint, 830, 980, 20.0, 20)
    return case(f"fifth_{'dup' if up else 'del'}_L{Lmax}", "stop", T, medint, 40.0, 40.0, 10.0, Lmax, escapes=0, inexact=0,
                sweep=sweep, marked={1: 200, 2: 201}, stop=2)


def both_case(nb):
    """Alternating bins 10 / 45 with medians 20 / 60, tlamda 4: every bin is a hit at L = 1, the DEL sweep stops there, and the windows
    of three bins around a 45 reach it for the DEL sweep at L = 3, above its stop: the DUP sweep takes those nb / 2 bins, and they
    count towards its stop.  nb / 2 entries for the `both` list (16 384)."""
    T = np.where(np.arange(nb) % 2 == 0, F32(10.0), F32(45.0)).astype(F32)
    medint = np.where(np.arange(nb) % 2 == 0, 20, 60).astype(np.int32)
    return case(f"both_alternating_nb{nb}", "stop", T, medint, 40.0, 40.0, 4.0, 5, escapes=0, inexact=0,
                stops=(1, 1), both_min=nb // 2 - 4)


def both_del_wins_case():
    """Fifty sparse triples 10 / 45 / 10: the DEL sweep reaches the 45 at L = 3 and never stops, so the bin is a deletion's although the
    DUP sweep saw it at L = 1."""
    nb = 2000
    T, medint = flat(nb)
    for j in range(50):
        a = 100 + 35 * j
        put(T, medint, a, a + 3, 10.0, 20)
        put(T, medint, a + 1, a + 2, 45.0, 60)
    return case("both_del_wins", "stop", T, medint, 40.0, 40.0, 4.0, 20, escapes=0, inexact=0, stops=(20, 20), both_min=50)


# ---- the exactness flag --------------------------------------------------------------------------------------------------------------
def below(x):
    return float(np.nextafter(F32(x), F32(0.0)))


def exact_a_case(n):
    """(a) values at the edges of the former range test -- 2^-10 and the float below it, 2^20 and the float below it, their negatives,
    zeros.  What decides is the stretch: sum |v| against 2^30 times the power of two of each bin."""
    lo, hi = 2.0 ** -10, 2.0 ** 20
    nb = 200
    T = np.zeros(nb, dtype=F32)
    if n == 0:      # the sum is at 2^20 and beyond: every bin of 2^-10 and below is too small
        vals = [hi, -hi, below(hi), -below(hi), lo, -lo, below(lo), -below(lo), lo, below(lo)]
    elif n == 1:    # the sum stays below 2^20: the bins of 2^-10 are fine, the floats below it (power of two 2^-11) are not
        vals = [below(hi)] + [lo] * 10 + [-lo] * 10 + [below(lo)] * 3 + [-below(lo)] * 2
    elif n == 2:    # nothing too small: the sum stays below 2^20 and no bin below 2^-10
        vals = [-below(hi)] + [lo] * 40
    elif n == 3:    # one bin tips the sum to exactly 2^20: sum = (2^20 - 2^-4) + 64 * 2^-10
        vals = [below(hi)] + [lo] * 64
    elif n == 4:    # ... and one bin fewer leaves it a step below
        vals = [below(hi)] + [lo] * 63
    else:           # large values alone, far outside the former range: exact
        vals = [2.0 ** 24, -2.0 ** 25, 2.0 ** 21] * 5
    pos = np.random.default_rng(0xE8AC + n).permutation(np.arange(5, nb - 5))[:len(vals)]
    T[pos] = np.array(vals, dtype=F32)
    medint = np.full(nb, 40, dtype=np.int32)
    exp = {0: 6, 1: 5, 2: 0, 3: 64, 4: 0, 5: 0}[n]
    return case(f"exact_a{n}", "exact_a", T, medint, 40.0, 0.0, 1.0e30, 20, ref=False, escapes=0, inexact=exp)


def exact_a_tiles_case():
    """(a) over several tiles: every bin near 2^19, seven bins of 2^-10 ... 2^-9 away from the tile edges (further than the halo): each
    is counted once, by the workgroup that owns it, with or without the detection pass."""
    nb = 3000
    rng = np.random.default_rng(0xE8B0)
    T = (2.0 ** 19 + rng.integers(0, 4096, size=nb) * 16.0).astype(F32)
    spots = [40, 300, 700, 1100, 1500, 2200, 2900]
    T[spots] = (2.0 ** -10 * (1.0 + rng.integers(0, 1 << 20, size=len(spots)) / float(1 << 21))).astype(F32)
    medint = np.full(nb, 40, dtype=np.int32)
    return case("exact_a_tiles", "exact_a", T, medint, 40.0, 0.0, 1.0e30, 20, ref=False, escapes=0, inexact=len(spots))


# seed, large values uniform in [2^a, 2^b): 385, 271 and 14 windows whose two means differ (with [2^10, 2^12) this generator gives none)
def exact_a_halo_case():
    """(a) a stretch whose only too-small bin lies in its halo: one bin of 2^-10 at 1020, zeros before it, every bin from 1024 on at 2^19
    (Lmax 20: a halo of 11 bins).  The workgroup that owns bin 1020 (bins 0 ... 1023 with a detection pass, 768 ... 1023 without)
    stages eleven large bins and counts its bin; the next one (from 1024) stages bin 1020 in its halo, owns no small bin and counts
    one for the stretch; no other stretch holds a small bin.  Two, by hand, on either route."""
    nb = 2100
    T = np.zeros(nb, dtype=F32)
    T[1024:] = F32(2.0 ** 19)
    T[1020] = F32(2.0 ** -10)
    return case("exact_a_halo", "exact_a", T, np.full(nb, 40, dtype=np.int32), 40.0, 0.0, 1.0e30, 20, ref=False, escapes=0, inexact=2)


EXACT_B_SHAPES = ((0xB001, 18, 20), (0xB002, 18, 20), (0xB003, 14, 16))
EXACT_B_PICKS = 5


def exact_b_chromosome(seed, a, b):
    rng = np.random.default_rng(seed)
    nb = 3000
    T = rng.uniform(2.0 ** a, 2.0 ** b, size=nb).astype(F32)
    tiny = rng.random(nb) < 0.1
    T[tiny] = rng.uniform(2.0 ** -10, 2.0 ** -8, size=int(tiny.sum())).astype(F32)
    return T


def exact_b_windows(T, Lmax):
    """[(L, centre, reference's float mean, exactly summed window's float mean)] where the two differ, over the windows the scan
    visits.  The exact sum is math.fsum's: the correctly rounded double of the window's sum, here from integer prefixes (every
    value is a multiple of 2^-33)."""
    nb = T.size
    y = T.astype(np.float64)
    scaled = y * 2.0 ** 33
    assert (scaled == np.floor(scaled)).all()
    P = np.array([0] + list(np.cumsum(np.array([int(v) for v in scaled], dtype=object))), dtype=object)
    Ls = np.arange(1, Lmax + 1)
    sums = np.cumsum(y)[Ls - 1].copy()
    out = []
    for first in range(1, nb):
        last = first + Ls - 1
        live = last < nb
        if not live.any():
            break
        sums[live] = sums[live] - y[first - 1] + y[last[live]]
        i = Ls // 2 + first
        scan = live & (i < nb - Ls // 2 - 1)
        ex = np.zeros(Lmax)
        ex[live] = (P[first + Ls[live]] - P[first]).astype(np.float64) / 2.0 ** 33
        mref, mex = (sums / Ls).astype(np.float32), (ex / Ls).astype(np.float32)
        for k in np.nonzero(scan & (mref != mex))[0]:
            out.append((int(Ls[k]), int(i[k]), float(mref[k]), float(mex[k])))
    return out


_B_CACHE = {}


def exact_b_cases():
    """(b) mixed magnitudes: the sliding sums are rounded, so the reference's float mean differs from the exactly summed window's in a few
    hundred windows.  For up to EXACT_B_PICKS of them per chromosome (tmedian, tlamda) are set so that one of the two is a hit by
    equality and the other is no hit.  All medians are 20: every DEL hit passes the median test, no DUP hit does."""
    out = []
    for seed, a, b in EXACT_B_SHAPES:
        Lmax = 200
        T = exact_b_chromosome(seed, a, b)
        key = (seed, a, b)
        if key not in _B_CACHE:
            _B_CACHE[key] = exact_b_windows(T, Lmax)
        wins = _B_CACHE[key]
        tmedian = float(2.0 ** b)
        # the lowest means first: few other windows hit below them
        order = sorted(wins, key=lambda w: (min(w[2], w[3]) - tmedian) * math.sqrt(w[0]))[:EXACT_B_PICKS]
        medint = np.full(T.size, 20, dtype=np.int32)
        for n, (L, pos, mref, mex) in enumerate(order):
            root = math.sqrt(float(L))
            # the lower mean is a hit by equality, the higher one is no hit
            tlamda = -((min(mref, mex) - tmedian) * root)
            out.append(case(f"exact_b_{seed:x}_{n}", "exact_b", T, medint, 40.0, tmedian, tlamda, Lmax, escapes=0,
                            window=(L, pos), mref=mref, mex=mex, differing=len(wins)))
    return out


# ---- the list ------------------------------------------------------------------------------------------------------------------------
_CASES = None


def all_cases():
    global _CASES
    if _CASES is not None:
        return _CASES
    cs = []
    for big in (False, True):
        for sweep in (0, 1):
            for L in TIE_LENGTHS:
                cs.append(tie_case(L, sweep, big))
    for Lmax in (20, 99, 224):
        for long_form in (False, True):
            for edge in (255, 256, 257):
                for family in (0, 1):
                    # thinned at 224, where the CPU replay of a case walks through 100 000 ... 170 000 hits: each edge once; the long
                    # event of 264 bins cannot end on bin 255 ... 257, so all three long ones start there
                    if Lmax < 224 or family == (1 if long_form or edge == 256 else 0):
                        cs.append(tile_case(Lmax, long_form, edge, family))
            for k in (0, 1, 2):
                if Lmax < 224 or not long_form or k == 0:
                    cs.append(ends_case(Lmax, k, long_form))
    for nb in (1, 2, 3, 4):
        cs.append(small_nb_case(nb, nb))
    for nb in (255, 256, 257, 1024, 1025):
        cs.append(small_nb_case(nb, 99))
    for nb in (255, 257):
        cs.append(small_nb_case(nb, nb))
    for rd in (40.0, 41.0, 30.5):
        cs.append(median_limits_case(rd))
    cs.append(median_pairs_case())
    cs.append(median_mid_case())
    for rd, seed in ((40.0, 0x3ED1), (41.0, 0x3ED2), (30.5, 0x3ED3)):
        cs.append(median_random_case(rd, seed))
    for seed in (0x7A11, 0x7A12):
        cs.append(trim_predicates_case(seed))
    for dist in (0, 5, 9, 40, 400):
        cs.append(trim_outside_case(dist))
    for off in (0, 21, 43):
        cs.append(marks_lengths_case(off))
    cs.append(marks_nested_case())
    for Lmax, k in KCAP_LMAX.items():
        cs.append(two_events_and_tie(f"kcap{k}_L{Lmax}", "marks", Lmax, kcap=k))
    for sweep in (0, 1):
        for Lmax in (2, 20):
            cs.append(fifth_case(sweep, Lmax))
    cs.append(both_case(4000))
    cs.append(both_case(40_000))
    cs.append(both_del_wins_case())
    last_detect = max(L for L in range(13_000, 13_400) if detect_runs(L))
    for Lmax, route in ((223, "thresholds in the arguments"), (224, "thresholds in memory"), (3800, "LDS tile"), (3801, "device-memory tile"),
                        (10_400, "resident work block"), (10_401, "long form"), (last_detect, "last detection pass"),
                        (last_detect + 1, "no detection pass")):
        cs.append(two_events_and_tie(f"route_L{Lmax}", "routes", Lmax, route=route))
    for n in range(6):
        cs.append(exact_a_case(n))
    cs.append(exact_a_tiles_case())
    cs.append(exact_a_halo_case())
    cs.extend(exact_b_cases())
    cs.append(escape_case(0))
    cs.append(escape_case(1))
    names = [c.name for c in cs]
    assert len(set(names)) == len(names)
    _CASES = cs
    return cs


def case_names(group=None):
    return [c.name for c in all_cases() if group is None or c.group == group]


def get_case(name):
    return next(c for c in all_cases() if c.name == name)
