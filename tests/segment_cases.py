"""Inputs for the segment search alone (get_rsi_segments, rsi.cpp:1060-1117: k_run_prefix + k_best_subsegment, segment_items /
segments_from_best around them) at its ties, seams and list forms: tests/test_segment_cases.py on the CPU, tests/test_segment_edges.py
on the GPU through rsi_hot_debug_segments; the reference's answers: tools/make_golden_segments.py -> golden/segment_edges.npz.

numpy only, seeded.  A case is a Case: name, group, claim (what it was built for, in words), T (float32 bins), status (int32), runs (the
marked runs the reference's get_continuous_segments emits: every run but the last, which it never emits -- every case ends in a run of
one bin that is there to be dropped), tmedian, pairs_per_item (0: what a run chooses) and expect, what the case claims about itself;
tests/test_segment_cases.py proves every claim from the restatement below, never from the library.

The exactness condition.  Inside the runs every value is 0 or a float32 in [2^-6, 2^9) and a run has at most 8192 bins: every value is
then a multiple of 2^-29 and every partial sum lies below 2^22, so it is exact in a double.  The reference's sliding sum and the
device's prefix difference are then the same number, and the score -- a division, a subtraction, an absolute value, a square root, a
product, each rounded once (-ffp-contract=off) -- is the same bits.  exact_condition() checks it.

The library's constants that place a case are restated here; the CPU test states the derived numbers.
"""
import math
from collections import namedtuple

import numpy as np

Case = namedtuple("Case", "name group claim T status runs tmedian pairs_per_item expect")

THREADS, ROUND = 256, 4            # offsets per length a workgroup takes at once; lengths per round of a thread (kernels_bin.hip)
BEST_LDS = 6144                    # kBestLds: doubles of a run's prefix (len + 1 of them) staged in LDS
RUNS_INLINE, ITEMS_INLINE = 200, 150   # kRunsInline, kItemsInline: lists that ride in the kernel arguments
MAILBOX_MAX_COPY = 512 << 10       # kMailboxMaxCopy: bytes of run status values that come back through the mailbox
MAX_RUN = 8192
DEL, DUP = 0, 1
F32 = np.float32


# ---- the library's host decisions, restated (pipeline_steps.h: segment_pairs_per_item, segment_items; pipeline.hip: rsi_segments) -----
def pairs_per_item(runs, lonely=True):
    ppi = 1 << 16
    if lonely:
        total = sum((e - s + 1) * (e - s + 2) // 2 for s, e in runs)
        room = max(8, ITEMS_INLINE - 2 * len(runs))
        ppi = min(ppi, max(1 << 13, total // room + 1))
    return ppi


def segment_items(runs, ppi):
    """[(run, len, Lbeg, Lend)]: lengths [Lbeg, Lend) of one run."""
    items = []
    for r, (s, e) in enumerate(runs):
        n = e - s + 1
        L = 1
        while L <= n:
            pairs, Le = 0, L
            while Le <= n and pairs < ppi:
                pairs += n - Le + 1
                Le += 1
            items.append((r, n, L, Le))
            L = Le
    return items


def expected_info(case):
    """info[0..5] of rsi_hot_debug_segments and the pairs per item, from the restated constants: runs, items, inline, status through the
    mailbox, runs beyond the LDS staging, segments (tlamda = 0: one per run)."""
    ppi = case.pairs_per_item or pairs_per_item(case.runs)
    items = segment_items(case.runs, ppi)
    bins = sum(e - s + 1 for s, e in case.runs)
    inline = len(case.runs) <= RUNS_INLINE and len(items) <= ITEMS_INLINE
    mailbox = inline and bins * 4 <= MAILBOX_MAX_COPY
    unstaged = sum(1 for s, e in case.runs if e - s + 2 > BEST_LDS)
    return [len(case.runs), len(items), int(inline), int(mailbox), unstaged, len(case.runs), min(ppi, 0x7fffffff)]


# ---- the reference's loops, restated ------------------------------------------------------------------------------------------------
def continuous_segments(status):
    """get_continuous_segments(status, 1) (rsi.cpp:291-326): stretches of marked bins of one sign; the LAST one is never emitted."""
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


_memo = {}


def best_subsegment(values, tmedian):
    """The double loop of rsi.cpp:1082-1100 over one run, lengths then offsets ascending, strict comparisons: (offset, L, score) of the
    first maximum -- (0, len, 0.0) when nothing scored -- and every (L, offset) that attains it.  The sums are exact (exact_condition),
    so the sliding sum is the difference of exact prefixes; one row of numpy per L, each element rounded as the scalar loop rounds."""
    key = (values.tobytes(), float(tmedian))
    if key in _memo:
        return _memo[key]
    n = values.size
    P = np.concatenate(([0.0], np.cumsum(values.astype(np.float64))))
    opt, at, attain = 0.0, (0, n), []
    for L in range(1, n + 1):
        score = np.abs((P[L:] - P[:n - L + 1]) / float(L) - tmedian) * math.sqrt(float(L))
        top = float(score.max())
        if top > opt:
            opt, at = top, (int(np.argmax(score)), L)
            attain = [(L, int(j)) for j in np.nonzero(score == top)[0]]
        elif top == opt and opt > 0:
            attain += [(L, int(j)) for j in np.nonzero(score == top)[0]]
    _memo[key] = (at[0], at[1], opt, attain)
    return _memo[key]


def get_rsi_segments_numpy(T, status, tmedian):
    """get_rsi_segments: per emitted run (start, end, type, score, attaining set).  The type is the sign of the grid median of the status
    values covered (rsi.cpp:1105); a run has one sign, so that is the sign of any of them."""
    out = []
    for s, e in continuous_segments(status):
        j, L, opt, attain = best_subsegment(np.ascontiguousarray(T[s:e + 1]), tmedian)
        a, b = s + j, s + j + L - 1
        covered = status[a:b + 1]
        assert (covered > 0).all() or (covered < 0).all()
        dup = float(np.median(covered)) > 0
        out.append((a, b, DUP if dup else DEL, opt if dup else -opt, attain))
    return out


def exact_condition(case):
    for s, e in case.runs:
        v = case.T[s:e + 1]
        if e - s + 1 > MAX_RUN or not (((v == 0) | ((v >= F32(2.0 ** -6)) & (v < F32(2.0 ** 9)))).all()):
            return False
    return case.T.dtype == np.float32


# ---- building ------------------------------------------------------------------------------------------------------------------------
def layout(parts, tmedian, lead=3):
    """parts: [(values, status values or one level, gap in front)] -> T, status, runs; unmarked bins carry tmedian rounded to float32;
    a gap of 0 puts a run against the one before it (they must differ in sign).  Ends in the run of one bin that is never emitted."""
    fill = F32(tmedian)
    T, st, runs = [np.full(lead, fill, dtype=F32)], [np.zeros(lead, dtype=np.int32)], []
    pos = lead
    for k, (values, level, gap) in enumerate(parts):
        values = np.asarray(values, dtype=F32)
        level = np.broadcast_to(np.asarray(level, dtype=np.int32), values.shape)
        if k > 0:
            T.append(np.full(gap, fill, dtype=F32))
            st.append(np.zeros(gap, dtype=np.int32))
            pos += gap
        T.append(values)
        st.append(level)
        runs.append((pos, pos + values.size - 1))
        pos += values.size
    T += [np.full(2, fill, dtype=F32), np.full(1, fill + F32(1), dtype=F32)]
    st += [np.zeros(2, dtype=np.int32), np.ones(1, dtype=np.int32)]
    return np.concatenate(T), np.concatenate(st).astype(np.int32), runs


def filler(n, tmedian):
    """n bins that score next to nothing: tmedian itself when it is an integer, else the two integers around it in turn."""
    if float(tmedian).is_integer():
        return np.full(n, tmedian, dtype=F32)
    lo = math.floor(tmedian)
    return (lo + (np.arange(n) % 2)).astype(F32)


def planted(n, tmedian, plants):
    """A run of n filler bins with values planted: plants = [(offset, values)]."""
    v = filler(n, tmedian)
    for off, vals in plants:
        vals = np.asarray(vals, dtype=F32)
        v[off:off + vals.size] = vals
    return v


def gamma_run(rng, n, scale=8.0):
    v = rng.gamma(4.0, scale, size=n).astype(F32)
    return np.clip(v, F32(2.0 ** -6), np.nextafter(F32(2.0 ** 9), F32(0)))


_cases = None


def _build():
    C = []

    def add(name, group, claim, parts, tmedian, ppi=0, **expect):
        T, st, runs = layout(parts, tmedian)
        C.append(Case(name, group, claim, T, st, runs, float(tmedian), ppi, expect))

    # ---- run lengths: one run, and two runs of opposite sign against each other --------------------------------------------------
    rng = np.random.default_rng(0x5E6001)
    for n in (1, 2, 3, 4, 5, 7, 8, 9, 255, 256, 257, 6142, 6143, 6144):
        add(f"len_{n}", "lengths", f"one run of {n} bins", [(gamma_run(rng, n), -3 if n % 2 else 2, 0)], 30.0, lengths=[n])
    for a, b in ((1, 1), (2, 3), (4, 5), (7, 8), (9, 4), (255, 256), (257, 255), (6143, 6144)):
        add(f"pair_{a}_{b}", "lengths", f"runs of {a} and {b} bins of opposite sign, no bin between them",
            [(gamma_run(rng, a), 2, 0), (gamma_run(rng, b), -2, 0)], 30.0, lengths=[a, b], adjacent=True)

    # ---- ties: integer bins as -MED makes them, tmedian an integer and an integer + 0.5 ---------------------------------------------
    for tm, tag in ((10.0, "int"), (10.5, "half")):
        up = 14.0   # |14 - tmedian| at L = 1
        for d in (100, 256, 400):
            add(f"tie_offsets_{d}_{tag}", "ties", f"the maximum at L = 1 at two offsets {d} apart: the first wins",
                [(planted(700, tm, [(120, [up]), (120 + d, [up])]), 1, 0)], tm, attain=[(1, 120), (1, 120 + d)],
                same_thread=(d % THREADS == 0))
        # L = 1 against L = 4: |v - t| = 2 |mean4 - t|
        four = [12, 12, 12, 12] if tag == "int" else [12, 12, 12, 13]
        add(f"tie_L1_L4_{tag}", "ties", "the maximum at L = 1 and at L = 4 (sqrt 4 exact): L = 1 wins",
            [(planted(60, tm, [(5, [up]), (30, four)]), 1, 0)], tm, attain=[(1, 5), (4, 30)])
        add(f"tie_L1_L4_items_{tag}", "ties", "the same with L = 1 and L = 4 in different work items (8192 pairs an item)",
            [(planted(3000, tm, [(1500, [up]), (2000, four)]), -1, 0)], tm, ppi=8192, attain=[(1, 1500), (4, 2000)], split=(1, 4))
        add(f"first_offset_{tag}", "ties", "the maximum at the run's first offset", [(planted(300, tm, [(0, [up])]), 1, 0)], tm, attain=[(1, 0)])
        add(f"last_offset_{tag}", "ties", "the maximum at the run's last offset", [(planted(300, tm, [(299, [up])]), 1, 0)], tm, attain=[(1, 299)])
        add(f"first_and_last_{tag}", "ties", "the maximum at the first and at the last offset: the first wins",
            [(planted(300, tm, [(0, [up]), (299, [up])]), -1, 0)], tm, attain=[(1, 0), (1, 299)])
        add(f"whole_run_{tag}", "ties", "the maximum is the whole run", [(np.full(300, 12.0, dtype=F32), 1, 0)], tm, attain=[(300, 0)])
    # L = 1 against L = 64: |18 - 10| = 8 |11 - 10|; 40 bins between them keep every window over both below 8.  With tmedian 10.5:
    # |18 - 10.5| = 8 (60 / 64): 36 elevens and 28 twelves, evenly spread so that no part of the block scores more, a ten on each side
    spread = 11 + (np.floor((np.arange(64) + 1) * 28 / 64) - np.floor(np.arange(64) * 28 / 64))
    for tm, tag, blk, lead in ((10.0, "int", [11.0] * 64, 0), (10.5, "half", [10.0] + list(spread) + [10.0], 1)):
        add(f"tie_L1_L64_{tag}", "ties", "the maximum at L = 1 and at L = 64 (sqrt 64 exact): L = 1 wins",
            [(planted(120, tm, [(0, [18.0]), (41 - lead, blk)]), 1, 0)], tm, attain=[(1, 0), (64, 41)])
        for n, ppi in ((300, 8192), (1200, 65536), (1200, 0)):
            add(f"tie_L1_L64_items_{ppi}_{tag}", "ties", f"the same in different work items, pairs_per_item {ppi}",
                [(planted(n, tm, [(100, [18.0]), (180 - lead, blk)]), 1, 0)], tm, ppi=ppi, attain=[(1, 100), (64, 180)], split=(1, 64))

    # ---- nothing scores: every window mean is tmedian -------------------------------------------------------------------------------
    for n in (1, 300):
        for level in (-2, 3):
            add(f"flat_{n}_{'dup' if level > 0 else 'del'}", "nothing", "every value is tmedian: the whole run, score 0, type by the status",
                [(np.full(n, 25.0, dtype=F32), level, 0)], 25.0, whole=True)

    # ---- list forms ------------------------------------------------------------------------------------------------------------------
    rng = np.random.default_rng(0x5E6002)

    def short_runs(k):
        return [(gamma_run(rng, int(rng.integers(1, 6))), 1 if i % 2 else -1, int(rng.integers(0, 3)) if i else 0) for i in range(k)]
    for k in (150, 151, 200, 201):
        add(f"runs_{k}", "lists", f"{k} runs of 1..5 bins: an item each", short_runs(k), 30.0)
    # one run cut into 150 and into 151 items
    for want in (150, 151):
        n = want    # with 1 pair an item every length is an item of its own
        add(f"items_{want}", "lists", f"one run of {n} bins, an item per length: {n} items", [(gamma_run(rng, n), 1, 0)], 30.0, ppi=1)
    # sixteen runs of 8192 bins are 512 KB of status values: the mailbox's limit; one bin more exceeds it
    big = [planted(8192, 20.0, [(1000 + 37 * k, [40.0]), (5000, [24.0] * 16)]) for k in (0, 1)]
    levels = np.where(np.arange(8192) < 3000, 1, np.where(np.arange(8192) < 6000, 7, 40)).astype(np.int32)
    sixteen = [(big[k % 2], levels if k % 2 else -levels, 0) for k in range(16)]
    add("mailbox_at_limit", "lists", "131072 run bins: their status values ride in the mailbox", sixteen, 20.0, ppi=1 << 40)
    add("mailbox_beyond", "lists", "131073 run bins: the status array is copied", sixteen + [(np.array([29.0], dtype=F32), 1, 5)], 20.0, ppi=1 << 40)

    # ---- type: levels of one sign mixed; the segment covers part of them --------------------------------------------------------------
    lv = np.array([-1] * 40 + [-7] * 40 + [-40] * 40, dtype=np.int32)
    add("levels_del_part", "type", "levels -1, -7, -40 in one run; the segment lies in the -7 stretch",
        [(planted(120, 30.0, [(50, [12.0] * 20)]), lv, 0), (planted(50, 30.0, [(10, [44.0] * 8)]), 3, 0)], 30.0, part=True)
    add("levels_dup_part", "type", "levels 1, 7, 40 in one run against a DEL run; the segment lies in the 40 stretch",
        [(planted(50, 30.0, [(10, [11.0] * 8)]), -3, 0), (planted(120, 30.0, [(90, [52.0] * 20)]), -lv, 0)], 30.0, part=True)

    # ---- NB-like: gamma floats, no constructed ties ----------------------------------------------------------------------------------
    rng = np.random.default_rng(0x5E6003)
    for k in range(3):
        parts = []
        for i in range(100):
            n = int(rng.integers(1, 401))
            parts.append((gamma_run(rng, n, 6.0 + k), int(rng.choice([-5, -2, -1, 1, 2, 6])), int(rng.integers(1, 30))))
        add(f"nb_like_{k}", "nb_like", "100 runs of 1..400 bins of gamma floats", parts, 28.0 + 0.37 * k)
    return C


def all_cases():
    global _cases
    if _cases is None:
        _cases = _build()
        assert len({c.name for c in _cases}) == len(_cases)
    return _cases


def get_case(name):
    return next(c for c in all_cases() if c.name == name)


def run_list(case):
    return np.array(case.runs, dtype=np.int32).reshape(-1, 2)
