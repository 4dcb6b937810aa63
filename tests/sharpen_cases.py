"""Inputs for the edge refinement alone (optimize_with_derivative, rsi.cpp:889-944, called twice, rsi.cpp:1876-1877: k_sharpen_edges under
DeviceTester::sharpen) at its ties, seams, range checks and list forms: tests/test_sharpen_cases.py on the CPU, tests/test_sharpen_edges.py
on the GPU through rsi_hot_debug_sharpen; the reference's answers: tools/make_golden_sharpen.py -> golden/sharpen_edges.npz.

numpy only, seeded.  A case is a Case: name, group, claim, depth (int32, the compacted depth), jobs (int32 [k, 3]: start, end, type) and
expect, what the case claims about itself; tests/test_sharpen_cases.py proves every claim from the restatement below.

dd[i] = (sum of the len values left of from + i) - (sum of the len values from there on), i in [0, to - from).  A step of -h in otherwise
constant depth at position from + i makes dd[i] = len h the one maximum; a step of +h the one minimum: that is how extrema are planted.

Group `crossed`: the first call leaves end < start, and in the second the reference's loops index its vector out of range (DESIGN section
2, divergence 4).  Those cases are not in the golden file; they are judged by the restatement's rule "the entries that exist", which is
what the library's host path and the oracle do.

The kernel's shapes (kernels_cand.hip) are restated below to place extrema on seams; the CPU test states the derived numbers.
"""
from collections import namedtuple

import numpy as np

Case = namedtuple("Case", "name group claim depth jobs expect")

CHUNKS, TILE = 16, 256       # kEdgeChunks: pieces per search window; values a workgroup walks at once
WS_MIN_JOBS = 256            # the workspace is laid out for max(256, 2 njobs) jobs when it must grow
DEL, DUP, UNTYPED = 0, 1, 2


# ---- the kernel's shapes, restated ------------------------------------------------------------------------------------------------------
def reach_of(length):
    return max(250, int(length / 4))       # C division: towards zero


def piece_of(index, wbase, wspan):
    """(piece, tile inside the piece) of dd index `index` in a window of wspan entries from wbase."""
    cs = (wspan + CHUNKS - 1) // CHUNKS
    return (index - wbase) // cs, ((index - wbase) % cs) // TILE


def ws_jobs_after(before, njobs):
    return max(WS_MIN_JOBS, 2 * njobs) if njobs > before else before


# ---- the reference's loop, restated ---------------------------------------------------------------------------------------------------
def optimize(rd, start, end, typ):
    """One call of optimize_with_derivative on one candidate: (start, end, report).  The reference's order: the two range checks, dd,
    the start search over the first 2 reach entries, the end search over the last 2 reach, each a strict comparison against 0 and then
    against the best so far, so the first extremum wins; index 0 is found and never applied.  report: early ('start' / 'end': the range
    check that returned), oob (the reference's loops would leave dd: fewer than 2 reach entries -- the searches here then cover the
    entries that exist), lo / hi (the lowest and highest index of rd read), win[w] = (window's first index, entries, extremum, indices
    attaining it, index taken or -1)."""
    n = rd.size
    length = end - start + 1
    reach = reach_of(length)
    nstart, nend = start - reach, end + reach
    rep = dict(early=None, oob=False, reach=reach, nstart=nstart, win=[None, None], lo=None, hi=None)
    if nstart < 2 * length:
        rep["early"] = "start"
        return start, end, rep
    if nend > n - 2 * length:
        rep["early"] = "end"
        return start, end, rep
    nstep = nend - nstart
    rep["oob"] = 2 * reach > nstep
    p = rd.astype(np.int64)
    dd0 = int(p[nstart - length:nstart].sum() - p[nstart:nstart + length].sum()) if length > 0 else 0
    q = np.arange(nstart, nend - 1)                                   # i - 1 of the reference's recurrence
    rep["lo"] = min(nstart - abs(length), nstart)
    rep["hi"] = max(nend - 2 + abs(length), nend - 2)
    assert rep["lo"] >= 0 and rep["hi"] < n, "the recurrence leaves the array"
    dd = np.concatenate(([dd0], dd0 + np.cumsum(-p[q - length] + 2 * p[q] - p[q + length])))
    assert dd.size == nstep
    if typ > 1:
        return start, end, rep
    new = [start, end]
    for w in (0, 1):
        base = 0 if w == 0 else max(0, nstep - 2 * reach)
        stop = min(2 * reach, nstep) if w == 0 else nstep
        v = dd[base:stop]
        want_max = (typ == DEL) == (w == 0)
        ext = int(v.max() if want_max else v.min())
        attain = [base + int(i) for i in np.nonzero(v == ext)[0]]
        imax = attain[0] if (ext > 0 if want_max else ext < 0) else -1
        rep["win"][w] = (base, stop - base, ext, attain, imax)
        if imax > 0:
            new[w] = nstart + imax if w == 0 else nend - nstep + imax
    return new[0], new[1], rep


def refine(rd, start, end, typ, calls=2):
    """`calls` calls: (start, end, [report per call])."""
    reps = []
    for _ in range(calls):
        start, end, r = optimize(rd, start, end, typ)
        reps.append(r)
    return start, end, reps


def refine_jobs(case, calls=2):
    out, reps = [], []
    for s, e, t in case.jobs:
        a, b, r = refine(case.depth, int(s), int(e), int(t), calls)
        out.append((a, b))
        reps.append(r)
    return np.array(out, dtype=np.int32).reshape(-1, 2), reps


def stays_inside(reps):
    """No call of the reference would index its vector out of range."""
    return all(not r["oob"] for r in reps)


# ---- building ------------------------------------------------------------------------------------------------------------------------
def stepped(n, base, steps=(), spikes=()):
    d = np.full(n, base, dtype=np.int64)
    for pos, delta in steps:
        d[pos:] += delta
    for pos, delta in spikes:
        d[pos] += delta
    assert d.min() >= 0 and d.max() < 2 ** 31
    return d.astype(np.int32)


def job_at(nstart, length):
    """The candidate whose dd starts at position nstart."""
    start = nstart + reach_of(length)
    return start, start + length - 1


_cases = None


def _build():
    C = []

    def add(name, group, claim, depth, jobs, **expect):
        C.append(Case(name, group, claim, np.ascontiguousarray(depth, dtype=np.int32), np.array(jobs, dtype=np.int32).reshape(-1, 3), expect))

    # ---- candidate lengths ------------------------------------------------------------------------------------------------------------
    rng = np.random.default_rng(0x5A4001)
    for k, length in enumerate((1, 2, 15, 16, 17, 31, 32, 33, 999, 1000, 1003, 1004, 8192, 8200)):
        n = 4000 if length < 999 else (8000 if length < 8192 else 50_000)
        start = {4000: 1700, 8000: 3100, 50_000: 20_000}[n]
        end = start + length - 1
        typ = k % 2
        # short candidates on constant depth (on Poisson depth their first call wanders and crosses), long ones on Poisson(30)
        d = rng.poisson(30, n).astype(np.int64) if length >= 999 else np.full(n, 30, dtype=np.int64)
        d[start - 7:end + 6] += 18 if typ == DUP else -18       # the event: from 7 bases before the candidate to 5 behind it
        d = np.clip(d, 0, 250)
        add(f"len_{length}", "lengths", f"a candidate of {length} bases with its event 7 and 5 bases wider", d, [(start, end, typ)],
            length=length, reach=max(250, length // 4))

    # ---- the two range checks, a base on each side -------------------------------------------------------------------------------------
    n = 4000
    d = rng.poisson(30, n).astype(np.int64)
    for s, e in ((440, 560), (3440, 3560)):
        d[s:e] -= 15
    d = np.clip(d, 0, 250)
    for name, start, early in (("from_eq_2len", 450, None), ("from_eq_2len_m1", 449, "start")):
        add(name, "range", "from = start - 250 against 2 len = 200", d, [(start, start + 99, DEL)], early=early)
    for name, end, early in (("to_eq_n_m2len", n - 450, None), ("to_eq_n_m2len_p1", n - 449, "end")):
        add(name, "range", "to = end + 250 against n - 2 len = n - 200", d, [(end - 99, end, DEL)], early=early)

    # ---- where the extremum lies: steps planted in constant depth; len 600, reach 250: the searches (500 entries, pieces of 32) lie
    # 99 entries apart, so no first call crosses ---------------------------------------------------------------------------------------
    n, length, nstart = 5000, 600, 1300
    s, e = job_at(nstart, length)
    wb1 = length - 1                                    # first index of the end search: 1099 entries, the last 500
    for typ, sign, tag in ((DEL, -1, "del"), (DUP, +1, "dup")):
        for idx in (31, 32, 479, 480, 499):
            add(f"start_{tag}_idx{idx}", "seams", f"the start search's extremum on index {idx} of 500: pieces of 32", stepped(n, 40, [(nstart + idx, 10 * sign)]),
                [(s, e, typ)], win=0, attain=[idx], zero_other=idx != 499)      # 499: the end search sees the step's far slope, all of the wrong sign
            add(f"end_{tag}_idx{idx}", "seams", f"the end search's extremum on index {idx} of its 500", stepped(n, 40, [(nstart + wb1 + idx, -10 * sign)]),
                [(s, e, typ)], win=1, attain=[wb1 + idx], zero_other=True)
        add(f"index0_{tag}", "index0", "the extremum on index 0: found, nothing moves", stepped(n, 40, [(nstart, 10 * sign)]), [(s, e, typ)],
            win=0, attain=[0], unmoved=True)
        add(f"index0_and_5_{tag}", "index0", "the extremum on index 0 and again on index 5: the first wins, nothing moves",
            stepped(n, 40, [(nstart, 2 * sign)], [(nstart + 4, -5 * sign)]), [(s, e, typ)], win=0, attain=[0, 5], unmoved=True)
    # two equal extrema: len 10, steps at least len apart; so close to the array's start that the second call returns at once
    n, length, nstart = 3000, 10, 300
    s, e = job_at(nstart, length)
    for a, b, tag in ((70, 85, "same_piece"), (70, 200, "two_pieces"), (95, 96 + 10, "neighbour_pieces")):
        add(f"equal_{tag}", "equal", f"two equal maxima on indices {a} and {b}: the first wins", stepped(n, 60, [(nstart + a, -10), (nstart + b, -10)]),
            [(s, e, DEL)], win=0, attain=[a, b], pieces=tag)
    n, length, nstart = 5000, 600, 1300
    s, e = job_at(nstart, length)
    add("zero_extremum", "zero", "the start search's maximum is exactly 0, everything else below: the start stays", stepped(n, 40, [(nstart + 700, 10)]),
        [(s, e, DEL)], win=0, ext=0, unmoved_start=True)
    add("constant", "zero", "constant depth: every dd is 0", stepped(n, 37), [(1400, 1499, DEL), (1400, 1499, DUP), (1200, 1800, DEL)], unmoved=True)
    # len 8200: pieces of 257, a tile of 256 and one more entry: the carried prefix
    n, length, nstart = 50_000, 8200, 17_950
    s, e = job_at(nstart, length)
    for idx in (3 * 257 + 255, 3 * 257 + 256, 4 * 257):
        add(f"tile_idx{idx}", "seams", f"len 8200, pieces of 257: the extremum on index {idx} (piece, tile) = {piece_of(idx, 0, 4100)}",
            stepped(n, 30, [(nstart + idx, -10)]), [(s, e, DEL)], win=0, attain=[idx], zero_other=True)

    # ---- types, for the start search and the end search separately ------------------------------------------------------------------------
    n, length, nstart = 5000, 600, 1300
    s, e = job_at(nstart, length)
    for which, pos in (("start", nstart + 200), ("end", nstart + length - 1 + 300)):
        for sign in (-1, 1):
            add(f"types_{which}_{'down' if sign < 0 else 'up'}", "types", f"a step {'down' if sign < 0 else 'up'} in the {which} search, for DEL, DUP and an untyped candidate",
                stepped(n, 40, [(pos, 10 * sign)]), [(s, e, DEL), (s, e, DUP), (s, e, UNTYPED)])

    # ---- values ---------------------------------------------------------------------------------------------------------------------------
    big = 2 ** 30
    add("depth_2p30", "values", "depths of 2^30 on a few bases: the int64 steps 2 p[q] and the sign of the accumulated first entry",
        stepped(n, 30, [(nstart + 200, -10), (nstart + 820, 10)], [(nstart - 50, big), (nstart + 3, big), (nstart + 260, big), (nstart + 700, big), (nstart + 701, big)]),
        [(s, e, DEL), (s, e, DUP), (s + 40, e + 60, DEL)], int32_only=True)
    add("depth_254_255", "values", "254 / 255 in byte storage", stepped(n, 255, [(nstart + 200, -1), (nstart + 820, 1)]), [(s, e, DEL), (s, e, DUP)])

    # ---- job lists -------------------------------------------------------------------------------------------------------------------------
    rng = np.random.default_rng(0x5A4002)
    n = 8000
    d = rng.poisson(30, n).astype(np.int64)
    events = [(900, 1100, 0.5), (1900, 2400, 1.5), (3300, 3420, 0.4), (4300, 5000, 1.6), (5900, 6000, 0.5), (6700, 6750, 1.7)]
    for a, b, f in events:
        d[a:b] = rng.poisson(30 * f, b - a)
    d = np.clip(d, 0, 250).astype(np.int32)

    def near_events(k):
        jobs = []
        while len(jobs) < k:
            a, b, f = events[int(rng.integers(len(events)))]
            st, en = a + int(rng.integers(-60, 61)), b + int(rng.integers(-60, 61))
            typ = (DEL if f < 1 else DUP) if rng.random() < 0.8 else int(rng.integers(0, 3))
            if en >= st and stays_inside(refine(d, st, en, typ)[2]):
                jobs.append((st, en, typ))
        return jobs
    for k in (1, 256, 257, 3):
        add(f"jobs_{k}", "lists", f"a list of {k} jobs", d, near_events(k), njobs=k)
    mixed = []
    for i in range(30):
        a, b, f = events[i % len(events)]
        mixed.append([(a + 20, b - 15, DEL if f < 1 else DUP), (100 + i, 200 + i, DEL), (a + 20, b - 15, UNTYPED)][i % 3])
    add("jobs_mixed", "lists", "refined, unchanged and untyped jobs in turn: the early returns leave their neighbours' arrival counters alone", d, mixed)

    # ---- crossed: the first call leaves end < start ---------------------------------------------------------------------------------------
    n = 3000
    for name, a, b, typ, sign in (("crossed_del_50", 1400, 1450, DEL, 1), ("crossed_del_1", 1400, 1401, DEL, 1), ("crossed_dup_80", 1380, 1460, DUP, -1)):
        dep = stepped(n, 60, [(a, 30 * sign), (b, -30 * sign)])
        add(name, "crossed", f"a {'bump' if sign > 0 else 'dip'} on [{a}, {b}) inside both searches: the first call leaves end < start",
            dep, [(1350, 1449, typ)], crossed_job=0)
    dep = stepped(n, 60, [(1400, 30), (1450, -30), (2200, -25), (2400, 25)])
    add("crossed_in_a_list", "crossed", "a crossed job between two ordinary ones", dep, [(2190, 2390, DEL), (1350, 1449, DEL), (2210, 2410, DEL)],
        crossed_job=1)

    # ---- random: Poisson(30) with planted events, candidates of 20 .. 3000 bases -------------------------------------------------------------
    rng = np.random.default_rng(0x5A4003)
    for k in range(3):
        n = 8000
        d = rng.poisson(30, n).astype(np.int64)
        ev = []
        pos = 700
        while pos < n - 1500:
            w = int(np.exp(rng.uniform(np.log(20), np.log(1200))))
            f = float(rng.choice([0.5, 1.5, 0.3, 2.0]))
            d[pos:pos + w] = rng.poisson(30 * f, w)
            ev.append((pos, pos + w - 1, DEL if f < 1 else DUP))
            pos += w + int(rng.integers(300, 900))
        d = np.clip(d, 0, 250).astype(np.int32)
        jobs = []
        while len(jobs) < 100:
            if rng.random() < 0.7:
                a, b, typ = ev[int(rng.integers(len(ev)))]
                st, en = a + int(rng.integers(-80, 81)), b + int(rng.integers(-80, 81))
            else:
                w = int(np.exp(rng.uniform(np.log(20), np.log(3000))))
                st = int(rng.integers(0, n - w))
                en, typ = st + w - 1, int(rng.integers(0, 2))
            if 0 <= st <= en < n and stays_inside(refine(d, st, en, typ)[2]):
                jobs.append((st, en, typ))
        add(f"random_{k}", "random", "100 candidates on Poisson(30) with planted events", d, jobs)
    return C


def all_cases():
    global _cases
    if _cases is None:
        _cases = _build()
        assert len({c.name for c in _cases}) == len(_cases)
    return _cases


def get_case(name):
    return next(c for c in all_cases() if c.name == name)


def storages(case):
    """Both storages wherever the values fit a byte."""
    return (1, 4) if int(case.depth.max()) <= 255 and not case.expect.get("int32_only") else (4,)
