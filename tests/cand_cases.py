"""Inputs for the neighbourhood test of a candidate alone (isitcnvwrap + isitcnv, rsi.cpp:101-287: plan_test on the host, DeviceTester::test
over k_candidate_test / k_cand_gather, k_cand_sums, k_cand_hist) at the edges of its walks, slots, seams, quantile grids and decline flags:
tests/test_cand_cases.py on the CPU, tests/test_cand_edges.py on the GPU through rsi_hot_debug_candidate_tests; the reference's answers:
tools/make_golden_cand.py -> golden/cand_edges.npz.

numpy only, seeded.  A case is a Case: name, group, claim, depth (int32: the compacted depth, or bin medians in the bin form), span_all
(what the stage compares depth.size with), RDmedian, P (m, minmlen, chklen, buffer, maxchkbp), cands (int32 [k, 4]: start, end, type,
status), index (the entries tested) and expect, what the case claims about itself; tests/test_cand_cases.py proves every claim from the
restatement below.  Every builder runs for both kinds, `_del` and `_dup`.

Depth is uniform on 25 .. 35 around RDmedian 30 unless a case says otherwise: a deletion's walk drops values above 3 RDmedian = 90, a
duplication's those below 0.15 RDmedian = 4.5; neither occurs unless planted.  The candidate's own bases are 10 .. 20 (DEL) or 45 .. 60 (DUP).

Not in the golden file (the reference has no behaviour there, its Array throws): a neighbourhood no longer than the candidate (group
`empty`, DESIGN section 2 divergence 5), and a right walk that fills all of `capacity` slots where 2 chklen d is not an integer (group
`fraction`: the reference then writes one slot past its array).  Those are judged by the restatement's rule, which is the host walk's:
status -9 / the walk stops at `capacity`.
"""
import json
import math
import os
from collections import namedtuple

import numpy as np

Case = namedtuple("Case", "name group claim depth span_all RDmedian P cands index expect")

DEL, DUP = 0, 1
CHAIN_MAX = 48                 # kChainMax: neighbour intervals handed to the device per side
HIST_BINS = 16384              # kCandHistBins
CHUNKS = 16                    # kCandChunks
THREADS = 1024                 # kTestThreads
PER = {4: 16, 1: 64}           # positions a thread holds of a trip, by the width of the stored values
TRIP = {4: 16 * THREADS, 1: 64 * THREADS}
DEFAULT_P = dict(m=101, minmlen=3.01, chklen=2.5, buffer=0.05, maxchkbp=100000)
NO_GOLDEN = ("empty", "fraction")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cand_edges.npz")
EXACT = ("cnvmed", "cnviqr", "refmed", "refsd", "refiqr")       # grid values and their differences: compared bit for bit
CLOSE = ("p1", "cnvsd")                                         # at the project's rtol = 1e-6


def load_golden(path=GOLDEN):
    """name -> one dict per tested candidate, in the order of the case's index."""
    z = np.load(path)
    names, off = json.loads(str(z["names"])), z["off"]
    fi, ff = json.loads(str(z["int_fields"])), json.loads(str(z["float_fields"]))
    ints, floats = z["ints"], z["floats"]
    out = {}
    for i, n in enumerate(names):
        out[n] = [{**{f: int(ints[k][j]) for j, f in enumerate(fi)}, **{f: float(floats[k][j]) for j, f in enumerate(ff)}}
                  for k in range(off[i], off[i + 1])]
    return out


# ---- the plan: plan_test (host_calls.cpp), the list-only part of isitcnvwrap (rsi.cpp:185-211, 238-241) ---------------------------------
def plan(n, span_all, P, cands, ci):
    s, e, st = cands[:, 0], cands[:, 1], cands[:, 3]
    count = len(cands)
    body_len = int(e[ci] - s[ci] + 1)
    d = body_len
    if n == span_all and d < P["m"] * P["minmlen"]:
        d = int(P["m"] * P["minmlen"])
    if n < span_all // 2 and d < P["minmlen"]:
        d = int(P["minmlen"]) + 1
    T = dict(d=d, body_len=body_len, capacity=int(P["chklen"] * d * 2), margin=int(body_len * P["buffer"] + 1), top=int(P["chklen"] * d - 1),
             right_cap=2 * P["chklen"] * d, budget=P["maxchkbp"] * 10)
    T["edge_branch"] = bool(n - e[ci] < P["chklen"] * d)
    if T["edge_branch"]:
        T["top"] = T["capacity"] - 1 - n + int(e[ci])
    cut = 0
    pos = int(s[ci]) - T["margin"]
    nb = ci - 1
    while pos > 0 and nb > 0 and pos < s[nb]:
        nb -= 1
    while nb > 0 and st[nb] == -9:
        nb -= 1
    T["left_first"] = nb
    left = []
    while nb >= 0 and len(left) < CHAIN_MAX:
        left.append(nb)
        nb -= 1
        while nb > 0 and st[nb] == -9:
            nb -= 1
    if nb >= 0:
        cut |= 1
    pos = int(e[ci]) + T["margin"]
    nb = ci + 1
    while pos < n - 2 and nb < count and pos > e[nb]:
        nb += 1
    while nb < count - 1 and st[nb] == -9:
        nb += 1
    T["right_first"] = nb
    right = []
    while nb < count and len(right) < CHAIN_MAX:
        right.append(nb)
        nb += 1
        while nb < count - 1 and st[nb] == -9:
            nb += 1
    if nb < count:
        cut |= 2
    T["avail"] = None
    if not (cut & 1) and T["top"] >= 0:
        avail = int(s[ci]) - T["margin"] - 2 - sum(int(e[k] - s[k] + 1) for k in left)
        T["avail"] = avail
        if avail >= 2 * (T["top"] + 1) + 64:
            cut |= 4
    T.update(cut=cut, left_chain=left, right_chain=right)
    return T


# ---- one side of the walk (rsi.cpp:214-228, 242-256), a straight stretch at a time -------------------------------------------------------
def extreme(v, kind, RDmedian):
    v = np.asarray(v).astype(np.float64)
    return v > RDmedian * 3.0 if kind == DEL else v < RDmedian * 0.15


def walk(depth, kind, RDmedian, cands, nb, pos, room, direction):
    """The reference's loop from `pos` with `room` slots left and its neighbour pointer at `nb`: the values in the order they are taken,
    the last position examined (`pos` itself when none is), and per straight stretch -- the device starts a sequence of trips at each --
    its first position, the trigger's offset t (position = first + direction (1 + t)), the offset of the value that filled the last slot,
    how many positions were examined and how many values taken.  The pointer moves as the reference's does: over status -9 entries, but
    never past list index 0 / the last index."""
    n = depth.size
    s, e, st = cands[:, 0], cands[:, 1], cands[:, 3]
    count = len(cands)
    vals, stretches, reach, jumps, lo, hi = [], [], pos, 0, None, None
    ended = "full" if room <= 0 else "edge"
    while room > 0 and (pos > 2 if direction < 0 else pos < n - 2):
        p = np.arange(pos - 1, 1, -1) if direction < 0 else np.arange(pos + 1, n - 1)
        lo, hi = (int(p.min()) if lo is None else min(lo, int(p.min()))), (int(p.max()) if hi is None else max(hi, int(p.max())))
        v = depth[p]
        ext = extreme(v, kind, RDmedian)
        have = nb >= 0 if direction < 0 else nb < count
        inside = (p >= s[nb]) & (p <= e[nb]) if have else np.zeros(p.size, dtype=bool)
        hit = np.nonzero(~ext & inside)[0]
        tstar = int(hit[0]) if hit.size else None
        take = ~ext & ~inside
        if tstar is not None:
            take[tstar:] = False
        idx = np.nonzero(take)[0]
        rec = dict(first=pos, trigger=tstar, fill_t=None, examined=int(p.size if tstar is None else tstar + 1), taken=int(min(idx.size, room)), room=room)
        stretches.append(rec)
        if idx.size >= room:
            rec["fill_t"] = int(idx[room - 1])
            rec["examined"], rec["trigger"] = rec["fill_t"] + 1, None      # the walk stops in front of the trigger
            vals.append(v[idx[:room]])
            reach, room, ended = int(p[rec["fill_t"]]), 0, "full"
            break
        vals.append(v[idx])
        room -= idx.size
        if tstar is None:
            reach = int(p[-1])
            break
        reach = int(p[tstar])
        jumps += 1
        if direction < 0:
            pos = int(s[nb]) - 1
            nb -= 1
            while nb > 0 and st[nb] == -9:
                nb -= 1
        else:
            pos = int(e[nb]) + 1
            nb += 1
            while nb < count - 1 and st[nb] == -9:
                nb += 1
    out = np.concatenate(vals) if vals else np.zeros(0, dtype=depth.dtype)
    return dict(values=out.astype(np.int64), reach=reach, stretches=stretches, jumps=jumps, ended=ended, lo=lo, hi=hi)


# ---- partition_stat_tp (wufunctions.cpp:364-424) -----------------------------------------------------------------------------------------
def grid_stat(x, dy):
    """(lqt, med, uqt, buckets or None, the three buckets or None) of the float64 array x: minimum / index-order mean / maximum where the
    range is below dy or a rank is 0 (count < rank never holds), else ymin + bucket dy of the first bucket whose cumulated count reaches
    n / 4, n / 2, 3 n / 4."""
    n = x.size
    ymin, ymax = float(x.min()), float(x.max())
    q = [ymin, float(np.cumsum(x)[-1]) / float(n), ymax]
    if ymax - ymin < dy:
        return q[0], q[1], q[2], None, None
    nbk = int((ymax - ymin) / dy + 2)
    b = ((x - ymin) / dy + 0.5).astype(np.int64)
    cnt = np.bincount(b, minlength=nbk)
    cum = np.cumsum(cnt)
    before = cum - cnt
    at = [None, None, None]
    for k, r in enumerate((n // 4, n // 2, n * 3 // 4)):
        hit = np.nonzero((before < r) & (cum >= r))[0]
        if hit.size:
            at[k] = int(hit[0])
            q[k] = ymin + float(at[k]) * dy
    return q[0], q[1], q[2], nbk, (at, cum)


def normal_cdf(x):
    """alglib's normaldistribution (Cephes ndtr) as host_calls.cpp restates it."""
    num = [0.007547728033418631287834, -0.288805137207594084924010, 14.3383842191748205576712, 38.0140318123903008244444,
           3017.82788536507577809226, 7404.07142710151470082064, 80437.3630960840172832162]
    den = [0.0, 1.0, 38.0190713951939403753468, 658.070155459240506326937, 6379.60017324428279487120, 34216.5257924628539769006,
           80437.3630960840172826266]
    cnum = [0.0, 0.5641877825507397413087057563, 9.675807882987265400604202961, 77.08161730368428609781633646, 368.5196154710010637133875746,
            1143.262070703886173606073338, 2320.439590251635247384768711, 2898.0293292167655611275846, 1826.3348842295112592168999]
    cden = [1.0, 17.14980943627607849376131193, 137.1255960500622202878443578, 661.7361207107653469211984771, 2094.384367789539593790281779,
            4429.612803883682726711528526, 6089.5424232724435504633068, 4958.82756472114071495438422, 1826.3348842295112595576438]

    def horner(c, t):
        a = c[0]
        for k in c[1:]:
            a = k + t * a
        return a
    z = x / 1.41421356237309504880
    sign = 1.0 if z > 0 else (-1.0 if z < 0 else 0.0)
    az = abs(z)
    if az < 0.5:
        t = az * az
        erf = sign * 1.1283791670955125738961589031 * az * horner(num, t) / horner(den, t)
    elif az >= 10:
        erf = sign
    else:
        erf = sign * (1 - math.exp(-(az * az)) * horner(cnum, az) / horner(cden, az))
    return 0.5 * (erf + 1)


# ---- the whole test of cands[ci] ---------------------------------------------------------------------------------------------------------
def restate(case, ci):
    """Everything the hook reports for one record, from the reference's loops: the plan, the two walks, the thinning, the running mean, the
    two grid walks and isitcnv's decision; and the shapes the kernels derive from them."""
    depth, n, P, cands = case.depth, case.depth.size, case.P, case.cands
    kind = int(cands[ci, 2])
    T = plan(n, case.span_all, P, cands, ci)
    R = dict(plan=T, kind=kind)
    start, end = int(cands[ci, 0]), int(cands[ci, 1])
    # left: top + 1 slots, filled downwards; the gap closed at the front when the sequence runs out (rsi.cpp:229-234)
    L = walk(depth, kind, case.RDmedian, cands, T["left_first"], start - T["margin"], T["top"] + 1, -1)
    if T["top"] < 0:
        L["reach"] = start                       # no walk: the kernels report the candidate's start
    used0 = L["values"].size
    assert T["top"] >= -1, "a top below -1 would make the reference start its right side at a negative slot"
    # right: appended while used < 2 chklen d; the reference's array has `capacity` slots
    room = min(T["capacity"], math.ceil(T["right_cap"])) - used0
    Rt = walk(depth, kind, case.RDmedian, cands, T["right_first"], end + T["margin"], room, +1)
    free = walk(depth, kind, case.RDmedian, cands, T["right_first"], end + T["margin"], min(T["capacity"], math.ceil(T["right_cap"])), +1)
    Rt["reach"] = Rt["reach"] if room > 0 else end + T["margin"]
    R.update(left=L, right=Rt, used0=used0, rcnt=Rt["values"].size, left_reach=L["reach"], right_reach=Rt["reach"],
             right_reach_free=free["reach"])
    # the reference writes slot `capacity` when it takes one more value than fits: possible only where 2 chklen d is no integer
    R["past_capacity"] = bool(T["right_cap"] > T["capacity"] and Rt["ended"] == "full" and room > 0)
    ref = np.concatenate([L["values"][::-1], Rt["values"]])
    body = depth[start:end + 1].astype(np.int64)
    R["nref_raw"], R["thin"], R["ref_raw"] = ref.size, False, ref
    total = ref.size + body.size
    if total > T["budget"]:                      # rsi.cpp:264-282
        nref = int(float(ref.size) / float(total) * float(T["budget"]))
        nbody = int(float(body.size) / float(total) * float(T["budget"]))
        jr = (np.arange(nref, dtype=np.float64) / float(nref) * float(ref.size)).astype(np.int64) if nref > 0 else np.zeros(0, dtype=np.int64)
        jb = (np.arange(nbody, dtype=np.float64) / float(nbody) * float(body.size)).astype(np.int64) if nbody > 0 else np.zeros(0, dtype=np.int64)
        R["thin_index"] = (jr, jb)
        ref, body = ref[jr], body[jb]
        R["thin"] = True
    width, nwin = body.size, ref.size - body.size
    R.update(nref=ref.size, nbody=width, nwin=nwin, empty=bool(nwin <= 0 or width <= 0))
    # flag 8: a chain the host cut at 48 entries was consumed to its end.  The split form's right walk, where the host does not vouch for
    # the left one (cut bit 4), is given all of `capacity` and may use the chain up where the reference's walk would have stopped before
    R["chain_used_up"] = (bool(T["cut"] & 1) and L["jumps"] >= len(T["left_chain"]), bool(T["cut"] & 2) and Rt["jumps"] >= len(T["right_chain"]))
    R["chain_used_up_free"] = bool(T["cut"] & 2) and (Rt if T["cut"] & 4 else free)["jumps"] >= len(T["right_chain"])
    R["short_left"] = bool((T["cut"] & 4) and T["top"] >= 0 and used0 < T["top"] + 1)
    R["flags"] = {0: 8 if any(R["chain_used_up"]) else 0,                      # by form: one workgroup, split
                  1: (8 if R["chain_used_up"][0] or R["chain_used_up_free"] else 0) | (16 if R["short_left"] else 0)}
    if R["empty"]:
        R["flags"] = {f: v | 1 for f, v in R["flags"].items()}
        R["judged"] = dict(type=kind, status=-9, geno=0)      # the host walk's answer; the reference's Array throws
        return R
    # the candidate: integer grid
    bq = grid_stat(body.astype(np.float64), 1.0)
    s1, s2 = int(body.sum()), int((body * body).sum())
    assert s2 < 2 ** 53, "the sum of squares must stay exact in a double"
    R.update(body_min=int(body.min()), body_max=int(body.max()), body_s1=float(s1), body_s2=float(s2), body_q=bq[:3], body_nbk=bq[3], body_walk=bq[4])
    # the running mean (rsi.cpp:113-124): exact integer sums, float means
    csum = np.concatenate(([0], np.cumsum(ref)))
    means = ((csum[width:width + nwin] - csum[:nwin]).astype(np.float64) / float(width)).astype(np.float32)
    mq = grid_stat(means.astype(np.float64), 0.01)
    m64 = means.astype(np.float64)
    R.update(means=means, ref_q=mq[:3], ref_nbk=mq[3], ref_walk=mq[4])
    # all means equal and their sums below 2^53 in units of the mean's last bit: s1 and s2 are exact whatever the order
    R["constant_means"] = bool(means.min() == means.max() and float(means[0]) == int(means[0]) and nwin * float(means[0]) ** 2 < 2.0 ** 53)
    R["ref_s1"], R["ref_s2"] = math.fsum(m64), math.fsum(m64 * m64)            # exactly rounded; a float's square is exact in a double
    R["ref_s1_bound"] = (nwin - 1) * 2.0 ** -53 * math.fsum(np.abs(m64))
    R["ref_s2_bound"] = (nwin - 1) * 2.0 ** -53 * R["ref_s2"]
    fl = (2 if bq[3] is not None and bq[3] > HIST_BINS else 0) | (4 if mq[3] is not None and mq[3] > HIST_BINS else 0)
    R["flags"] = {f: v | fl for f, v in R["flags"].items()}
    # what the split form derives (kernels_cand.hip: cand_geometry, cand_sum_chunks, cand_sum_chunk_len, cand_chunk_len)
    chunks = min(CHUNKS, 4 * ref.size // width)
    R["split"] = dict(used0_mod16=used0 % 16, chunks=chunks, sum_chunk_len=(((nwin + chunks - 1) // chunks) + 3) & ~3,
                      hist_chunk_len=(((nwin + CHUNKS - 1) // CHUNKS) + 3) & ~3)
    R["split"]["sum_chunks_with_windows"] = -(-nwin // R["split"]["sum_chunk_len"])        # the chunks behind them leave neutral elements
    R["split"]["hist_chunks_with_windows"] = -(-nwin // R["split"]["hist_chunk_len"])
    # isitcnv's decision (rsi.cpp:126-169), sums in index order
    sm = float(np.cumsum(m64)[-1])
    sq = float(np.cumsum(m64 * m64)[-1])
    mu = sm / float(nwin)
    ref_var = sq / float(nwin) - mu * mu
    bmu = float(s1) / float(width)
    cnv_var = float(s2) / float(width) - bmu * bmu
    spread = math.sqrt(ref_var) if ref_var >= 0 else float("nan")
    if spread < 1e-3:
        spread = mq[1] / 40.0 + 1e-3
    J = dict(type=kind, status=1, geno=1, p1=1.0, cnvmed=bq[1], cnvsd=math.sqrt(cnv_var) if cnv_var >= 0 else float("nan"), cnviqr=bq[2] - bq[0],
             refmed=mq[1], refiqr=mq[2] - mq[0], refsd=(mq[2] - mq[0]) / 1.349)
    R.update(ref_var=ref_var, cnv_var=cnv_var, spread=spread, nu=None)
    observed = DUP if J["cnvmed"] > case.RDmedian else DEL
    if kind != observed:
        J["status"] = -9
    elif kind == DEL:
        level = max(min(mq[1], case.RDmedian), 0.8 * case.RDmedian)
        R["nu_num"], R["nu_scale"] = 3.0 * J["cnvmed"] - 2.0 * level, level
        nu = R["nu_num"] / spread
        J["p1"] = normal_cdf(nu)
        if nu > 0:
            J["status"], J["geno"] = -9, 0
        R["nu"] = nu
    else:
        level = max(mq[1], case.RDmedian)
        R["nu_num"], R["nu_scale"] = 2.5 * J["cnvmed"] - 3.0 * level, level
        nu = R["nu_num"] / spread / 1.5
        J["p1"] = 1.0 - normal_cdf(nu)
        if nu < 0:
            J["status"], J["geno"] = -9, 0
        R["nu"] = nu
    R["judged"] = J
    return R


def reads(R):
    """(lowest, highest) index of the depth any loop of the record reads (None, None when nothing is read)."""
    lo = [x for x in (R["left"]["lo"], R["right"]["lo"]) if x is not None]
    hi = [x for x in (R["left"]["hi"], R["right"]["hi"]) if x is not None]
    return (min(lo) if lo else None), (max(hi) if hi else None)


def in_golden(case):
    return case.group not in NO_GOLDEN


def trip_position(t, storage_bytes):
    """Where offset t of a straight stretch falls: (trip, thread, position in the thread, lane, wave)."""
    per, trip = PER[storage_bytes], TRIP[storage_bytes]
    k = t % trip
    return t // trip, k // per, k % per, (k // per) % 64, k // per // 64


def forms(case):
    """(storage, form) pairs a case runs in: form bit 0 = split, bit 1 = byte depth gathered as int32."""
    out = [(4, 1), (4, 0)]
    if int(case.depth.max()) <= 255 and not case.expect.get("int32_only"):
        out = [(1, 1), (1, 0), (1, 3), (1, 2)] + out
    return out


def stored_bytes(storage, form):
    return 1 if storage == 1 and not (form & 2) else 4


def kernel_name(storage, form):
    return ("candidate_test" if form & 1 else "candidate_test_one_wg") + ("_i32" if storage == 1 and (form & 2) else "")


# ---- building ----------------------------------------------------------------------------------------------------------------------------
def limits(kind, RDmedian):
    """The extreme limit of a kind and the nearest planted values: (limit, a value that is extreme, the nearest that is not)."""
    if kind == DEL:
        lim = RDmedian * 3.0
        return lim, int(math.floor(lim)) + 1, int(math.floor(lim))
    lim = RDmedian * 0.15
    return lim, int(math.ceil(lim)) - 1, int(math.ceil(lim))


def scene(kind, n, body, nbs=(), seed=1, RDmedian=30.0, extremes=(), base=(25, 36), body_values=None, sets=()):
    """depth[n] uniform on base, the candidate `body` = (start, end) filled with its kind's values, neighbours nbs = (start, end, status)
    left as they are, an extreme value of the kind on every position of `extremes`, then sets = (position, value) last.  Returns
    (depth, cands, index of the candidate)."""
    rng = np.random.default_rng(seed)
    d = rng.integers(base[0], base[1], n).astype(np.int64)
    s, e = body
    d[s:e + 1] = rng.integers(10, 21, e - s + 1) if kind == DEL else rng.integers(45, 61, e - s + 1)
    if body_values is not None:
        d[s:e + 1] = body_values
    _, ext, _ = limits(kind, RDmedian)
    for p in extremes:
        d[p] = ext
    for p, v in sets:
        d[p] = v
    assert d.min() >= 0 and d.max() < 2 ** 31
    rows = sorted([(a, b, kind, st) for a, b, st in nbs] + [(s, e, kind, 0)], key=lambda r: (r[0], r[3] != 0))
    cands = np.array(rows, dtype=np.int32).reshape(-1, 4)
    ci = [i for i, r in enumerate(rows) if (r[0], r[1], r[3]) == (s, e, 0)][0]
    return d.astype(np.int32), cands, ci


_cases = None
KINDS = ((DEL, "del"), (DUP, "dup"))


def _build():
    C = []

    def add(name, group, claim, depth, cands, index, P=None, span_all=None, RDmedian=30.0, **expect):
        PP = dict(DEFAULT_P)
        PP.update(P or {})
        depth = np.ascontiguousarray(depth, dtype=np.int32)
        assert depth.size <= 300_000, name
        C.append(Case(name, group, claim, depth, int(depth.size if span_all is None else span_all), float(RDmedian), PP,
                      np.ascontiguousarray(cands, dtype=np.int32).reshape(-1, 4), [int(i) for i in np.atleast_1d(index)], expect))

    # d = 128 bases, m = 1 (so d is the candidate's length), chklen = S / 128: S slots on each side, all numbers exact
    def sides(S):
        return dict(m=1, chklen=S / 128.0)
    BODY = 128
    MARGIN = int(BODY * 0.05 + 1)      # 7

    for kind, tag in KINDS:
        # ---- triggers: a neighbour's first ordinary base at offset t of the walk's first stretch, on both sides ----------------------------
        for t in (0, 15, 16, 63, 64, 1023, 1024, 4095, 4096, 16383, 16384, 16389, 65535, 65536, 65541):
            S = t + 700
            nbl = 40
            s0 = 3 + S + nbl + 64 + MARGIN                     # sequence enough on the left: S values, the neighbour, some to spare
            e0 = s0 + BODY - 1
            lpos, rpos = s0 - MARGIN, e0 + MARGIN              # the walks' first positions; offset t is lpos - 1 - t / rpos + 1 + t
            nbs = [(lpos - 1 - t - nbl + 1, lpos - 1 - t, 0), (rpos + 1 + t, rpos + 1 + t + nbl - 1, 0)]
            n = rpos + 1 + t + nbl + (S - t) + 64
            d, cands, ci = scene(kind, n, (s0, e0), nbs, seed=100 + t)
            add(f"trigger_t{t}_{tag}", "triggers", f"both walks meet a neighbour at offset {t} of their first stretch", d, cands, ci, P=sides(S),
                trigger=t, taken_each=S)
        # two neighbours inside one trip: the second is met by the stretch that starts behind the first
        S, nbl, t1, gap = 900, 30, 100, 50
        s0 = 3 + S + 2 * nbl + 64 + MARGIN
        e0 = s0 + BODY - 1
        lpos, rpos = s0 - MARGIN, e0 + MARGIN
        nbs = [(lpos - 1 - t1 - nbl + 1, lpos - 1 - t1, 0), (lpos - 1 - t1 - nbl - gap - nbl + 1, lpos - 1 - t1 - nbl - gap, 0),
               (rpos + 1 + t1, rpos + t1 + nbl, 0), (rpos + 1 + t1 + nbl + gap, rpos + t1 + nbl + gap + nbl, 0)]
        d, cands, ci = scene(kind, rpos + 1 + S + 2 * nbl + 64, (s0, e0), nbs, seed=7)
        add(f"two_triggers_{tag}", "triggers", "two neighbours within one trip's reach on each side", d, cands, ci, P=sides(S), triggers=[t1, gap])
        # a neighbour whose first met bases are extreme: no jump there, the trigger is the next ordinary base inside
        nbs = [(lpos - 1 - t1 - nbl + 1, lpos - 1 - t1, 0), (rpos + 1 + t1, rpos + t1 + nbl, 0)]
        ex = [lpos - 1 - t1, lpos - 2 - t1, rpos + 1 + t1, rpos + 2 + t1]
        d, cands, ci = scene(kind, rpos + 1 + S + 2 * nbl + 64, (s0, e0), nbs, seed=8, extremes=ex)
        add(f"first_extreme_{tag}", "triggers", "the neighbour's first two met bases are extreme: the trigger is the third", d, cands, ci, P=sides(S),
            triggers=[t1 + 2])
        # a neighbour of extreme values only is never jumped and the pointer stays: the next neighbour's values are taken
        nbs = [(lpos - 1 - t1 - nbl + 1, lpos - 1 - t1, 0), (lpos - 400, lpos - 380, 0), (rpos + 1 + t1, rpos + t1 + nbl, 0), (rpos + 380, rpos + 400, 0)]
        ex = list(range(lpos - 1 - t1 - nbl + 1, lpos - t1)) + list(range(rpos + 1 + t1, rpos + t1 + nbl + 1))
        d, cands, ci = scene(kind, rpos + 1 + S + 2 * nbl + 64, (s0, e0), nbs, seed=9, extremes=ex)
        add(f"all_extreme_{tag}", "triggers", "a neighbour of extreme values only: never jumped, the one behind it is walked through", d, cands, ci,
            P=sides(S), triggers=[])
        # ---- where neighbours lie -------------------------------------------------------------------------------------------------------------
        nbs = [(lpos - 20, lpos + 3, 0), (rpos - 3, rpos + 20, 0)]
        d, cands, ci = scene(kind, rpos + 1 + S + 2 * nbl + 64, (s0, e0), nbs, seed=10)
        add(f"starts_inside_{tag}", "placement", "both walks start inside a neighbour: a trigger on their first position", d, cands, ci, P=sides(S),
            triggers=[0])
        nbs = [(lpos - 60, lpos - 31, 0), (lpos - 30, lpos - 11, 0), (rpos + 11, rpos + 30, 0), (rpos + 31, rpos + 60, 0)]
        d, cands, ci = scene(kind, rpos + 1 + S + 2 * nbl + 64, (s0, e0), nbs, seed=11)
        add(f"adjacent_{tag}", "placement", "adjacent neighbours: the stretch behind a jump triggers on its first position", d, cands, ci, P=sides(S),
            triggers=[10, 0])
        nbs = [(lpos - 60, lpos - 25, 0), (lpos - 30, lpos - 11, 0), (rpos + 11, rpos + 30, 0), (rpos + 25, rpos + 60, 0)]
        d, cands, ci = scene(kind, rpos + 1 + S + 2 * nbl + 64, (s0, e0), nbs, seed=12)
        add(f"overlapping_{tag}", "placement", "overlapping neighbours: the jump lands inside the next one", d, cands, ci, P=sides(S), triggers=[10, 0])
        # neighbours that reach position 0 and n - 1, close enough for the walks to get there
        s1 = 400
        e1 = s1 + BODY - 1
        n1 = e1 + 400
        nbs = [(0, 150, 0), (n1 - 150, n1 - 1, 0)]
        d, cands, ci = scene(kind, n1, (s1, e1), nbs, seed=13)
        add(f"reach_the_ends_{tag}", "placement", "neighbours that cover position 0 and n - 1: both walks end by a jump past the array", d, cands, ci,
            P=sides(900), ends=True)
        # ---- rejected neighbours: skipped in the middle, never at list index 0 / the last index --------------------------------------------------
        S = 500
        s0 = 3 + S + 400
        e0 = s0 + BODY - 1
        lpos, rpos = s0 - MARGIN, e0 + MARGIN
        nbs = [(lpos - 300, lpos - 281, -9), (lpos - 200, lpos - 181, -9), (lpos - 100, lpos - 81, 0),
               (rpos + 81, rpos + 100, 0), (rpos + 181, rpos + 200, -9), (rpos + 281, rpos + 300, -9)]
        d, cands, ci = scene(kind, rpos + S + 400, (s0, e0), nbs, seed=14)
        add(f"rejected_{tag}", "rejected", "status -9 in the middle is walked through, at list index 0 and at the last index it is jumped", d, cands, ci,
            P=sides(S), jumps=(2, 2))
        nbs = [(lpos - 100, lpos - 81, -9), (rpos + 81, rpos + 100, -9)]
        d, cands, ci = scene(kind, rpos + S + 400, (s0, e0), nbs, seed=15)
        add(f"rejected_only_{tag}", "rejected", "the only neighbours are rejected and sit at the list's two ends: jumped all the same", d, cands, ci,
            P=sides(S), jumps=(1, 1))

        # ---- the extreme limit: 3 RDmedian / 0.15 RDmedian an integer, a half, just above and just below an integer -----------------------------
        for lt, med in (("int", 30.0 if kind == DEL else 40.0), ("half", 30.5 if kind == DEL else 30.0), ("above", 30.0 + 2.0 ** -40 if kind == DEL else 40.0 + 2.0 ** -38),
                        ("below", 30.0 - 2.0 ** -40 if kind == DEL else 40.0 - 2.0 ** -38)):
            lim, _, _ = limits(kind, med)
            S = 300
            s0 = 3 + S + 200
            e0 = s0 + BODY - 1
            lpos, rpos = s0 - MARGIN, e0 + MARGIN
            near = [int(math.floor(lim)) - 1, int(math.floor(lim)), int(math.floor(lim)) + 1, int(math.ceil(lim))]
            sets = [(lpos - 10 - 3 * k, v) for k, v in enumerate(near)] + [(rpos + 10 + 3 * k, v) for k, v in enumerate(near)]
            d, cands, ci = scene(kind, rpos + S + 200, (s0, e0), (), seed=16, RDmedian=med, sets=sets,
                                 body_values=None if kind == DEL else np.random.default_rng(3).integers(60, 80, BODY))
            add(f"limit_{lt}_{tag}", "limits", f"values around the limit {lim!r}: floor - 1, floor, floor + 1, ceil on each side", d, cands, ci, P=sides(S),
                RDmedian=med, near=near, limit_kind=lt)

        # ---- slots ----------------------------------------------------------------------------------------------------------------------------
        for S in (16384, 16385, 65536, 65537):          # no value dropped: the last slot is filled by offset S - 1: a trip's last position, the next trip's first
            s0 = 3 + S + 50
            e0 = s0 + BODY - 1
            d, cands, ci = scene(kind, e0 + MARGIN + S + 50, (s0, e0), (), seed=17)
            add(f"slots_{S}_{tag}", "slots", f"{S} slots on each side, nothing dropped", d, cands, ci, P=sides(S), fill_t=S - 1)
        # mid-thread: 37 extremes in front, so the value that fills the last of 1000 slots sits at offset 1036
        S = 1000
        s0 = 3 + S + 200
        e0 = s0 + BODY - 1
        lpos, rpos = s0 - MARGIN, e0 + MARGIN
        ex = [lpos - 1 - 5 * k for k in range(37)] + [rpos + 1 + 5 * k for k in range(37)]
        d, cands, ci = scene(kind, rpos + S + 200, (s0, e0), (), seed=18, extremes=ex)
        add(f"slots_midthread_{tag}", "slots", "37 extremes in front: the last of 1000 slots is filled at offset 1036", d, cands, ci, P=sides(S), fill_t=1036)
        # one slot a side: d = 1, chklen = 1 (minmlen below 1 so that d is not raised)
        d, cands, ci = scene(kind, 200, (100, 100), (), seed=19)
        add(f"room_1_{tag}", "slots", "capacity 2: one slot on each side, a candidate of one base, one window", d, cands, ci,
            P=dict(m=1, minmlen=0.5, chklen=1.0), capacity=2, nwin=1)
        # the left walk runs out of sequence with 0, 1 and top values taken
        # (a candidate of 16 bases: margin 1, d = 16, chklen 2.5: 40 slots a side)
        S = 40
        for want in (0, 1, S - 1):
            s0 = 1 + 2 + want                              # the walk visits start - margin - 1 .. 2
            e0 = s0 + 15
            d, cands, ci = scene(kind, e0 + 300, (s0, e0), (), seed=20)
            add(f"left_short_{want}_{tag}", "slots", f"the left walk runs out of sequence with {want} of {S} values: the gap is closed at the front", d, cands,
                ci, P=dict(m=1, chklen=2.5), used0=want, left_ended="edge")
        # the right walk stops at n - 2 with 5 values; n - end = 8 < chklen d = 40: top = 80 - 1 - 8 = 71 from the edge branch
        s0 = 300
        e0 = s0 + 15
        d, cands, ci = scene(kind, e0 + 1 + 5 + 2, (s0, e0), (), seed=21)
        add(f"right_short_{tag}", "slots", "the right walk stops at n - 2 with 5 values; top = 71 from the n - end < chklen d branch", d, cands, ci,
            P=dict(m=1, chklen=2.5), rcnt=5, top=71, edge_branch=True, right_ended="edge")
        d, cands, ci = scene(kind, 400, (384, 399), (), seed=22)
        add(f"edge_end_is_last_{tag}", "slots", "the candidate ends on n - 1: top = 80 - 1 - 1 = 78, the right walk visits nothing", d, cands, ci,
            P=dict(m=1, chklen=2.5), rcnt=0, top=78, edge_branch=True)
        # top = 0 from the edge branch needs capacity = n - end + 1 with n - end < chklen d: chklen d = 1.2 (d = 4, chklen 0.3), n - end = 1, capacity 2.
        # Its neighbourhood is one value against a candidate of four: always empty (flag 1), so it is judged by the restatement's rule
        d, cands, ci = scene(kind, 400, (396, 399), (), seed=23)
        add(f"edge_top_0_{tag}", "empty", "n - end = 1 < chklen d = 1.2, capacity 2: top = 0 from the edge branch; one value against a candidate of four", d,
            cands, ci, P=dict(m=1, chklen=0.3), top=0, edge_branch=True, flag=1)
        # d raised to m minmlen: a candidate of 10 bases with m = 101: d = 304
        d, cands, ci = scene(kind, 4000, (2000, 2009), (), seed=24)
        add(f"d_raised_{tag}", "slots", "10 bases, m = 101: d = (int)(101 x 3.01) = 304, top = 759, capacity 1520", d, cands, ci, d=304, capacity=1520, top=759)

        # ---- the seam between the left and the right part (split form: 16-value loads on either side of used0) ------------------------------------
        S = 200
        for u in list(range(0, 17)) + [31, 33]:
            s0 = 7 + 2 + u                                  # margin int(16 x 0.4 + 1) = 7: the walk visits start - 8 .. 2
            e0 = s0 + 15
            d, cands, ci = scene(kind, e0 + 600, (s0, e0), (), seed=30 + u)
            add(f"seam_{u}_{tag}", "seam", f"the left part has {u} values (the walk ran out of sequence), the candidate 16 bases", d, cands, ci,
                P=dict(m=1, chklen=S / 16.0, buffer=0.4), used0=u)
        # used0 = nref: the right walk takes nothing
        s0 = 700
        e0 = s0 + 15
        d, cands, ci = scene(kind, e0 + MARGIN + 2, (s0, e0), (), seed=50)
        add(f"seam_all_left_{tag}", "seam", "the right walk has no position to visit: the neighbourhood is the left part", d, cands, ci,
            P=dict(m=1, chklen=S / 16.0, buffer=0.4), rcnt=0)
        # chunk counts of the sliding sums: 4 nref / width on both sides of 5, 15 and 16, and at 4; width 64, nref = capacity - 2 - margin at the array's end
        for nref in (64 + 1, 79, 80, 239, 240, 255, 256, 400):
            cap = nref + 2 + 4
            n = 2000
            e0 = n - 10
            s0 = e0 - 63
            d, cands, ci = scene(kind, n, (s0, e0), (), seed=60 + nref)
            add(f"chunks_nref{nref}_{tag}", "chunks", f"width 64, nref {nref}: {min(16, 4 * nref // 64)} chunks", d, cands, ci, P=dict(m=1, chklen=cap / 128.0),
                nref=nref, chunks=min(16, 4 * nref // 64))
        # window counts: width 16, nref = capacity - 3 at the array's end
        for nwin in (1, 2, 3, 4, 63, 64, 65, 72, 1000, 16 * 1024, 16 * 1024 + 1):      # (72 = 9 chunks of 8: a multiple, and trailing chunks empty)
            cap = nwin + 16 + 3
            n = nwin + 600
            e0 = n - 5
            s0 = e0 - 15
            d, cands, ci = scene(kind, n, (s0, e0), (), seed=70 + nwin % 97)
            add(f"nwin_{nwin}_{tag}", "windows", f"width 16, {nwin} windows", d, cands, ci, P=dict(m=1, chklen=cap / 32.0), nwin=nwin)
        for width in (1, 2, 15, 17, 300):
            S = 100
            s0 = 2000
            e0 = s0 + width - 1
            d, cands, ci = scene(kind, 4600, (s0, e0), (), seed=80 + width)
            add(f"width_{width}_{tag}", "windows", f"width {width}, {S} slots a side" + (": more than there are windows" if width > S else ""), d, cands, ci,
                P=dict(m=1, minmlen=0.5, chklen=S / width if width in (1, 2) else (2.5 if width != 300 else 0.75)), width=width)
        # 16 x 16 384 windows and one more: a chunk's one full round of the sliding sums, and the start of a second
        for nwin in (16 * 16384, 16 * 16384 + 1):
            cap = nwin + 16 + 3
            n = nwin + 600
            e0 = n - 5
            s0 = e0 - 15
            d, cands, ci = scene(kind, n, (s0, e0), (), seed=90)
            add(f"nwin_{nwin}_{tag}", "windows", f"width 16, {nwin} windows: chunks of {((nwin + 15) // 16 + 3) & ~3}", d, cands, ci, P=dict(m=1, chklen=cap / 32.0),
                nwin=nwin)

        # ---- thinning (rsi.cpp:264-282): nref + nbody on both sides of the budget, small maxchkbp ---------------------------------------------------
        # chklen 4.5: a candidate of 200 has 1800 slots, 2000 in all; one of 201 has 1809, of which the left walk misses 9 (out of sequence): 2001
        s0 = 3 + 900 + 300
        e0 = s0 + 199
        d, cands, ci = scene(kind, e0 + 900 + 400, (s0, e0), (), seed=95)
        add(f"thin_budget_plus0_{tag}", "thinning", "nref 1800 + nbody 200 = the budget of 2000: nothing is thinned", d, cands, ci,
            P=dict(m=1, chklen=4.5, maxchkbp=200), thin=False, total=2000)
        s0 = 11 + 2 + (904 - 9)                            # margin int(201 x 0.05 + 1) = 11; 904 slots on the left
        e0 = s0 + 200
        d, cands, ci = scene(kind, e0 + 11 + 905 + 2, (s0, e0), (), seed=95)      # ... and the right walk stops at n - 2 with 905
        add(f"thin_budget_plus1_{tag}", "thinning", "nref 895 + 905 = 1800, nbody 201: one over the budget of 2000", d, cands, ci,
            P=dict(m=1, chklen=4.5, maxchkbp=200), thin=True, total=2001)
        S = 700
        s0 = MARGIN + 2 + 37
        e0 = s0 + 127
        d, cands, ci = scene(kind, e0 + S + 400, (s0, e0), (), seed=96)
        add(f"thin_seam_{tag}", "thinning", "thinned, with a left part of 37 values: every value through the indexed read", d, cands, ci,
            P=dict(m=1, chklen=S / 128.0, maxchkbp=50), thin=True, used0=37)
        # index products double(i) / double(nref) * double(size) whose exact value is an integer k and whose double is one step below it: the
        # reference reads slot k - 1.  Found by a search over (candidate length, slots a side, maxchkbp): (16, 75, 10) thins 150 values to 90
        # and has two such i, (16, 92, 10) thins 184 to 92 and has four; the CPU file proves them from the numbers
        for S, mx in ((75, 10), (92, 10), (78, 13)):
            s0 = 3 + S + 100
            e0 = s0 + 15
            d, cands, ci = scene(kind, e0 + S + 200, (s0, e0), (), seed=97 + S, base=(20, 41))
            add(f"thin_below_integer_{S}_{mx}_{tag}", "thinning", f"{2 * S} values thinned for a budget of {10 * mx}: an index product one double step below an integer",
                d, cands, ci, P=dict(m=1, chklen=S / 16.0, maxchkbp=mx), thin=True, below_integer=True)

        # ---- quantiles ------------------------------------------------------------------------------------------------------------------------
        S = 300
        s0 = 3 + S + 100
        for blen in (1, 2, 3):
            e0 = s0 + blen - 1
            d, cands, ci = scene(kind, e0 + S + 200, (s0, e0), (), seed=110 + blen)
            add(f"body_{blen}_{tag}", "quantiles", f"a candidate of {blen}: n / 4 = 0, the lower quartile stays the minimum", d, cands, ci,
                P=dict(m=1, minmlen=0.5, chklen=S / 4.0), nbody=blen)
        e0 = s0 + BODY - 1
        d, cands, ci = scene(kind, e0 + S + 200, (s0, e0), (), seed=114, body_values=15 if kind == DEL else 50)
        add(f"body_constant_{tag}", "quantiles", "a constant candidate: minimum, mean, maximum", d, cands, ci, P=sides(S), body_default=True)
        # ranks on a bucket's cumulated count and one short of it: 128 values, ranks 32 / 64 / 96
        lowv = 12 if kind == DEL else 50
        for name, counts in (("exact", (32, 32, 32, 32)), ("short", (31, 32, 32, 33)), ("over", (33, 32, 32, 31))):
            bv = np.repeat(np.array([lowv, lowv + 1, lowv + 3, lowv + 4]), counts)
            np.random.default_rng(5).shuffle(bv)
            d, cands, ci = scene(kind, e0 + S + 200, (s0, e0), (), seed=115, body_values=bv)
            add(f"body_ranks_{name}_{tag}", "quantiles", f"bucket counts {counts}: the cumulated count reaches the ranks 32 / 64 / 96 {name}ly", d, cands, ci,
                P=sides(S), counts=counts)
        # window means: a constant neighbourhood (range 0), and two values a window apart in mean by less than 0.01 and by exactly one bucket
        d, cands, ci = scene(kind, e0 + S + 200, (s0, e0), (), seed=116, base=(30, 31))
        add(f"means_constant_{tag}", "quantiles", "a constant neighbourhood: the means' range is 0, the three defaults", d, cands, ci, P=sides(S), ref_default=True)
        d, cands, ci = scene(kind, e0 + S + 200, (s0, e0), (), seed=117, base=(30, 31), sets=[(s0 - 50, 31)])
        add(f"means_narrow_{tag}", "quantiles", "one 31 among 30s, width 128: the means' range is 1 / 128 < 0.01", d, cands, ci, P=sides(S), ref_default=True)
        d, cands, ci = scene(kind, e0 + S + 200, (s0, e0), (), seed=118, base=(30, 31), sets=[(s0 - 50, 32)])
        add(f"means_one_pair_{tag}", "quantiles", "one 32 among 30s, width 128: the means' range is 1 / 64: three buckets, two of them hit", d, cands, ci,
            P=sides(S), ref_nbk=3)
        # means on a bucket edge: width 128, two runs of sixteen 31s among 30s, one in each part: the window sums take every value 3840 + m,
        # m = 0 .. 16, the means are 30 + m / 128 exactly, and for m = 16 (226 windows) (w - lo) / 0.01 + 0.5 is 13 in double arithmetic while
        # the quotient of the real numbers lies below (the double 0.01 is above 1 / 100): the bucket rests on the division's rounding, and the
        # upper quartile's rank falls into it.  A search over widths 64, 128, 256, minima 25 .. 36 and m < 200 finds no index one step BESIDE
        # an integer: dyadic differences always round onto it, and the float rounding of other widths' means is a million steps wide
        d, cands, ci = scene(kind, e0 + S + 200, (s0, e0), (), seed=118, base=(30, 31),
                             sets=[(s0 - 162 - k, 31) for k in range(16)] + [(e0 + 7 + 151 + k, 31) for k in range(16)])
        add(f"means_bucket_edge_{tag}", "quantiles", "window means 30 + m / 128, m = 0 .. 16: m = 16 sits on a bucket edge", d, cands, ci,
            P=sides(S), bucket_edge=(16,))

        # ---- the judgement's branches --------------------------------------------------------------------------------------------------------
        d, cands, ci = scene(kind, e0 + S + 200, (s0, e0), (), seed=119, body_values=26 if kind == DEL else 34)
        add(f"judged_rejected_{tag}", "judgement", "a candidate too close to the median: nu on the wrong side of 0, status -9, geno 0", d, cands, ci, P=sides(S),
            status=-9, geno=0)
        d, cands, ci = scene(kind, e0 + S + 200, (s0, e0), (), seed=120, body_values=50 if kind == DEL else 15)
        add(f"judged_wrong_type_{tag}", "judgement", "the candidate's median lies on the other side of RDmedian: status -9, geno stays 1", d, cands, ci,
            P=sides(S), status=-9, geno=1)

        # ---- decline flags -------------------------------------------------------------------------------------------------------------------
        lowv = 10 if kind == DEL else 50
        for span, flag in ((16382, 0), (16383, 2)):
            bv = np.full(BODY, lowv)
            bv[77] = lowv + span
            d, cands, ci = scene(kind, e0 + S + 200, (s0, e0), (), seed=121, body_values=bv)
            add(f"body_range_{span}_{tag}", "flags", f"the candidate's values span {span}: {span + 2} buckets against {HIST_BINS}", d, cands, ci, P=sides(S),
                flag=flag, int32_only=True)
        # the means' range: width 100, a window of mean lo and one of mean lo + 163.82 / 163.83: (hi - lo) / 0.01 + 2 truncates to 16384 / 16385
        lo = 0 if kind == DEL else 10
        for hundredths, flag in ((16382, 0), (16383, 4)):
            S = 400
            s0 = 3 + S + 100
            e0 = s0 + 99
            k164 = hundredths - 16300
            hi_vals = np.array([lo + 164] * k164 + [lo + 163] * (100 - k164))
            sets = [(s0 - 5 - 150 - i, int(v)) for i, v in enumerate(hi_vals)] + [(s0 - 5 - 300 - i, lo) for i in range(100)]
            d, cands, ci = scene(kind, e0 + S + 200, (s0, e0), (), seed=122, RDmedian=60.0, base=(55, 66), sets=sets,
                                 body_values=np.random.default_rng(6).integers(20, 31, 100) if kind == DEL else np.random.default_rng(6).integers(90, 110, 100))
            add(f"means_range_{hundredths}_{tag}", "flags", f"window means from {lo} to {lo} + {hundredths / 100}: {hundredths + 2} buckets against {HIST_BINS}", d,
                cands, ci, P=dict(m=1, chklen=S / 100.0), RDmedian=60.0, flag=flag)
        # more than 48 neighbours on a side: neighbours of 2 bases every 6 positions, 60 on each side
        # (a stretch behind a jump takes 3 values: the position next to the neighbour is never examined)
        for name, S, sidesel, flag in (("fills_first", 100, (1, 1), 0), ("fills_first_left", 100, (1, 0), 0), ("fills_first_right", 100, (0, 1), 0), ("left", 400, (1, 0), 8), ("right", 400, (0, 1), 8), ("both", 400, (1, 1), 8)):
            s0 = 3 + 1200
            e0 = s0 + BODY - 1
            lpos, rpos = s0 - MARGIN, e0 + MARGIN
            nbs = ([(lpos - 6 - 6 * k, lpos - 5 - 6 * k, 0) for k in range(60)] if sidesel[0] else []) + \
                  ([(rpos + 5 + 6 * k, rpos + 6 + 6 * k, 0) for k in range(60)] if sidesel[1] else [])
            d, cands, ci = scene(kind, rpos + 1300, (s0, e0), nbs, seed=123)
            add(f"chain_{name}_{tag}", "flags", f"60 neighbours on a side, {S} slots: " + ("the walk fills before the 48th" if not flag else "the 48 listed are used up"),
                d, cands, ci, P=sides(S), flag=flag, cut=(1 if sidesel[0] else 0) | (2 if sidesel[1] else 0))
        # flag 16: the host vouches for the left walk where avail >= 2 (top + 1) + 64
        S = 100
        for name, avail, nex, flag, bit in (("vouched_edge", 2 * S + 64, 0, 0, 4), ("not_vouched", 2 * S + 63, 0, 0, 0),
                                             ("vouched_short", 2 * S + 64, S + 65, 16, 4), ("vouched_just_fills", 2 * S + 64, S + 64, 0, 4)):
            s0 = avail + MARGIN + 2
            e0 = s0 + BODY - 1
            ex = [s0 - MARGIN - 1 - k for k in range(nex)]
            d, cands, ci = scene(kind, e0 + 600, (s0, e0), (), seed=124, extremes=ex)
            add(f"{name}_{tag}", "flags", f"avail = {avail} against 2 (top + 1) + 64 = {2 * S + 64}, {nex} extremes on the left", d, cands, ci, P=sides(S),
                flag_split=flag, cut=bit)
        # flag 1: the neighbourhood is no longer than the candidate
        d, cands, ci = scene(kind, 600, (100, 499), (), seed=125)
        add(f"empty_{tag}", "empty", "a candidate of 400 in an array of 600: fewer neighbourhood values than its own", d, cands, ci, P=dict(m=1, chklen=2.5),
            flag=1)
        # 2 chklen d = 2 S + 0.5 is no integer and the right walk fills all of capacity: the reference writes one slot too far
        S = 300
        s0 = 3 + S + 100
        e0 = s0 + BODY - 1
        d, cands, ci = scene(kind, e0 + S + 200, (s0, e0), (), seed=126)
        add(f"fraction_quarter_{tag}", "fraction", "chklen d = 300.25: capacity 600, the loop's bound 600.5", d, cands, ci, P=dict(m=1, chklen=300.25 / 128.0))
        d, cands, ci = scene(kind, e0 + S + 200, (s0, e0), (), seed=127)
        add(f"fraction_half_{tag}", "slots", "chklen d = 300.5: capacity 601 = the loop's bound, 300 slots on the left and 301 on the right", d, cands, ci,
            P=dict(m=1, chklen=300.5 / 128.0), capacity=601, top=299)

        # ---- deep int32 depth: the candidate's sum beyond 2^32, its sum of squares still below 2^53 (exact in a double) -----------------------------
        blen, lowv = (16384, 300_000) if kind == DEL else (8192, 800_000)
        S = blen * 5 // 2
        s0 = 3 + S + 900
        e0 = s0 + blen - 1
        rng = np.random.default_rng(128)
        # (the neighbourhood is constant 2^19: at this depth s2 / n - mu^2 of varying means cancels twelve digits and no order of summation
        # gives the reference's last bits; a power of two keeps every sum exact in any order)
        d, cands, ci = scene(kind, e0 + int(blen * 0.05 + 1) + S + 300, (s0, e0), (), seed=128, RDmedian=524_288.0, base=(524_288, 524_289),
                             body_values=lowv + rng.integers(0, 101, blen))
        add(f"deep_sums_{tag}", "deep", f"{blen} bases of about {lowv} among 2^19: the candidate's sum is beyond 2^32", d, cands, ci, P=dict(m=1),
            RDmedian=524_288.0, int32_only=True)

        # ---- the bin form: int32 bin medians, n < span_all / 2 -----------------------------------------------------------------------------------
        for nb_, blen in ((2000, 1), (2000, 3), (5000, 4), (20000, 60)):
            s0 = nb_ // 2
            e0 = s0 + blen - 1
            nbs = [(s0 - 40, s0 - 38, 0), (e0 + 30, e0 + 33, 0), (e0 + 60, e0 + 61, -9), (nb_ - 20, nb_ - 10, -9)]
            d, cands, ci = scene(kind, nb_, (s0, e0), nbs, seed=130 + blen, extremes=[s0 - 5, e0 + 7])
            add(f"bins_{nb_}_{blen}_{tag}", "bins", f"{nb_} bin medians, a segment of {blen} bins" + (": d raised to (int)3.01 + 1 = 4" if blen < 4 else ""), d,
                cands, ci, span_all=101 * nb_, d=max(blen, 4) if blen < 3.01 else blen)
        d, cands, ci = scene(kind, 2000, (1000, 1002), (), seed=135)
        add(f"neither_form_{tag}", "bins", "n = span_all / 2: neither form's rule raises d", d, cands, ci, span_all=4000, d=3)

        # ---- lists: 301 candidates of 20 bases 100 apart on one array; the GPU test runs 1, 300, 3, 301 and 1 of them ------------------------------
        n = 301 * 100 + 400
        rng = np.random.default_rng(140 + kind)
        d = rng.integers(25, 36, n).astype(np.int32)
        rows = []
        for k in range(301):
            a = 200 + 100 * k
            d[a:a + 20] = rng.integers(10, 20, 20) if kind == DEL else rng.integers(45, 61, 20)
            rows.append((a, a + 19, kind, -9 if k % 7 == 3 else 0))
        add(f"list_301_{tag}", "lists", "301 candidates on one array, every one tested against the list", d, np.array(rows), list(range(301)), P=dict(m=1, chklen=6.0),
            lists=(1, 300, 3, 301, 1))
        # a list too long for the mailbox slot: 640 candidates with 48 + 48 neighbours each
        n = 640 * 30 + 400
        d = rng.integers(25, 36, n).astype(np.int32)
        rows = []
        for k in range(640):
            a = 200 + 30 * k
            d[a:a + 8] = rng.integers(10, 20, 8) if kind == DEL else rng.integers(45, 61, 8)
            rows.append((a, a + 7, kind, 0))
        add(f"list_copied_{tag}", "lists", "640 candidates with full neighbour chains: jobs, chains and results exceed the mailbox slot", d, np.array(rows),
            list(range(640)), P=dict(m=1, chklen=2.5), copied=True)
    return C


def all_cases():
    global _cases
    if _cases is None:
        _cases = _build()
        assert len({c.name for c in _cases}) == len(_cases)
    return _cases


def get_case(name):
    return next(c for c in all_cases() if c.name == name)


_restated = {}


def restated(case):
    """index -> record, computed once per case and shared."""
    if case.name not in _restated:
        _restated[case.name] = {ci: restate(case, ci) for ci in case.index}
    return _restated[case.name]


# ---- range sums ----------------------------------------------------------------------------------------------------------------------------
def range_cases():
    """(name, depth, lo, hi): ranges for DeviceTester::range_sums (k_range_sums: one workgroup of 256 threads per range)."""
    rng = np.random.default_rng(0xCA5D)
    n = 120_000
    small = rng.integers(0, 256, n).astype(np.int32)
    out = []
    lo = [1000 + r for r in range(16) for _ in (1, 2, 255, 256, 257)]
    ln = [k for _ in range(16) for k in (1, 2, 255, 256, 257)]
    lo += [0, 0, n - 1, n - 257, 10_000, 0]
    ln += [1, 300, 1, 257, 100_000, n]
    out.append(("lengths_and_residues", small, np.array(lo), np.array(lo) + np.array(ln) - 1))
    out.append(("one_range", small, np.array([5]), np.array([5])))
    a = rng.integers(0, n - 400, 3000)
    out.append(("ranges_3000", small, a, a + rng.integers(0, 400, 3000)))
    full = np.full(n, 255, dtype=np.int32)                      # 100 000 x 255 = 25.5 M; a sum beyond 2^31 needs int32 depth
    out.append(("bytes_all_255", full, np.array([0, 7]), np.array([n - 1, 100_006])))
    big = rng.integers(2 ** 29, 2 ** 30, 50_000).astype(np.int32)
    out.append(("beyond_2p31_and_2p32", big, np.array([0, 3, 100]), np.array([1, 6, 49_999])))
    return out
