"""Inputs for the three list stages behind the scan, each alone: the block tests (areblockscnv, rsi.cpp:415-546: test_block_segments),
the merge (mergesegments, rsi.cpp:694-885: merge_neighbours) and everything behind the block tests (detectcnv, rsi.cpp:1860-1931, and
sd_filters, rsi.cpp:1753-1792: call_from_segments), at the edges of the shortcuts a device tester adds to them (host_calls.cpp): the block
batch, the batch of range sums, the tests launched ahead (Speculation) and the sparse status form.  tests/test_calls_cases.py on the CPU,
tests/test_calls_edges.py on the GPU through rsi_hot_debug_block_stage / _merge / _calls; the reference's answers:
tools/make_golden_calls.py -> golden/calls_edges.npz.

numpy only, seeded.  A case is a Case: name, stage ('block' / 'merge' / 'calls'), claim, depth (int32: bin medians for a block case, else
the compacted depth), status (block cases: the scan's status array), cands (a list of candidate dicts, FIELDS), noncode ((k, 2) regions,
calls cases), span_all, RDmedian, RDsd, P (m, minmlen, chklen, buffer, maxchkbp, p, merge) and expect, what the case claims about itself;
tests/test_calls_cases.py proves every claim from the restatement below.  Every builder runs for both kinds, `_del` and `_dup`.

The restatement follows the reference's serial loops line by line and takes every single neighbourhood test from cand_cases.restate.
Beside the serial answer it predicts what the shortcuts must do on the way to it: the road of every first-round block test, which tests
launched ahead survive same_plan, which means are answered from the batch of range sums -- and what a stale result would have given where
one must be refused.  detectcnv's own body (the bins -> bases loop, the stage order, the score, the N-region filter) exists in Python only:
the reference is asked stage by stage (tools/make_golden_calls.py), and the whole-run goldens pin the rest.

Depth is cand_cases' uniform 25 .. 35 around RDmedian 30; a deletion's own values are 10 .. 20, a duplication's 45 .. 60.

Not built (the reference has no defined behaviour there, or the situation cannot arise): a rejected segment that ends exactly ON the last
position the next test's left walk examined -- a listed neighbour's position is never the last one examined, the walk jumps from it; a call
whose expanded end EQUALS a region's start -- to_reference never returns a position inside a region, so a call meets a region only by spanning its junction, which is built; a bins -> bases clamp at 0 -- a segment's first bin is never negative, so
start m + m / 2 never is.
"""
import math
import os
from collections import namedtuple

import numpy as np

import cand_cases as cc
import sharpen_cases as sc

Case = namedtuple("Case", "name stage claim depth status cands noncode span_all RDmedian RDsd P expect")

DEL, DUP = cc.DEL, cc.DUP
BLOCK_BATCH_MIN = 24           # kBlockBatchMin
FIELDS = ("start", "end", "type", "geno", "status", "length", "score", "p1", "cnvmed", "cnvsd", "cnviqr", "refmed", "refsd", "refiqr")
INTS, FLOATS = FIELDS[:6], FIELDS[6:]
EXACT = INTS + cc.EXACT                      # compared bit for bit
CLOSE = cc.CLOSE + ("score",)                # at the project's rtol = 1e-6
DEFAULT_P = dict(cc.DEFAULT_P, p=0.05, merge=1)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "calls_edges.npz")
KINDS = cc.KINDS


def cand(start, end, typ, **kw):
    """A candidate as cnv_st() / Candidate leave it, with the caller's fields."""
    c = dict(start=int(start), end=int(end), type=int(typ), geno=0, status=0, length=0, score=0.0, p1=1.0, cnvmed=0.0, cnvsd=0.0, cnviqr=0.0,
             refmed=0.0, refsd=0.0, refiqr=0.0)
    c.update(kw)
    return c


def copy_list(L):
    return [dict(c) for c in L]


def _cands(L):
    return np.array([[c["start"], c["end"], c["type"], c["status"]] for c in L], dtype=np.int32).reshape(-1, 4)


def test_params(P):
    return {k: P[k] for k in ("m", "minmlen", "chklen", "buffer", "maxchkbp")}


# ---- one neighbourhood test of L[ci] (isitcnvwrap + isitcnv), from cand_cases' restatement -------------------------------------------------
def judge(depth, span_all, RDmedian, P, L, ci, log=None):
    """(the candidate as judged, cand_cases' record).  finish_judgement's rule for the fields a test leaves alone: p1 keeps its value when
    the observed type contradicts the candidate's (rsi.cpp:150-153 returns before it is set)."""
    case = cc.Case("", "", "", depth, int(span_all), float(RDmedian), test_params(P), _cands(L), [ci], {})
    R = cc.restate(case, ci)
    if log is not None:
        log.append(R)
    c = dict(L[ci])
    J = R["judged"]
    c.update(length=c["end"] - c["start"] + 1, type=J["type"], status=J["status"], geno=J["geno"])
    if not R["empty"]:
        c.update({k: J[k] for k in ("cnvmed", "cnvsd", "cnviqr", "refmed", "refsd", "refiqr")})
        if R["nu"] is not None:
            c["p1"] = J["p1"]
    return c, R


def plan_key(n, span_all, P, L, ci):
    """What same_plan compares: the plan of L[ci] against the list as it stands."""
    T = cc.plan(n, int(span_all), test_params(P), _cands(L), ci)
    iv = lambda ks: tuple((L[k]["start"], L[k]["end"]) for k in ks)
    return (L[ci]["start"], L[ci]["end"], L[ci]["type"], T["margin"], T["capacity"], T["top"], T["budget"], T["right_cap"], T["cut"],
            iv(T["left_chain"]), iv(T["right_chain"]))


def inside(R, n):
    """The reference's loops of this test stay inside its arrays."""
    lo, hi = cc.reads(R)
    return not R["empty"] and not R["past_capacity"] and (lo is None or lo >= 0) and (hi is None or hi < n)


def same(a, b):
    return all(a[k] == b[k] for k in FIELDS)


# ---- get_continuous_segments (rsi.cpp:291-327) and multisegments (rsi.cpp:368-410) -----------------------------------------------------------
def marked_runs(marks):
    """Runs of equal-sign marks at most one index apart; the last run is never emitted."""
    out, open_, first, last = [], False, 0, 0
    for i, v in enumerate(marks):
        if v == 0:
            continue
        if not open_:
            first = last = i
            open_ = True
            continue
        if float(v) * float(marks[last]) > 0 and i - last <= 1:
            last = i
            continue
        out.append((first, last))
        first = last = i
    return out


def nested_levels(seg, status, rec=None):
    s0, e0 = seg["start"], seg["end"]
    st = [int(status[i]) for i in range(s0, e0 + 1)]
    lo, hi = min(st), max(st)
    out = []
    for level in range(lo, hi):
        if level == 0:
            if rec is not None:
                rec["level0_skipped"] = True
            continue
        member = [1 if s != 0 and ((level < 0 and s < 0 and s >= level) or (level > 0 and s > 0 and s <= level)) else 0 for s in st]
        if level not in st:
            if rec is not None:
                rec.setdefault("absent", []).append(level)
            continue
        for a, b in marked_runs(member):
            out.append((max(a + s0, s0), min(b + s0, e0), level))
    return out


def sparse_ranges(status):
    """The sparse form a scan leaves (rsi_segments): the maximal runs of non-zero status as (first, last, position of the first value)."""
    out, at, i, n = [], 0, 0, len(status)
    while i < n:
        if status[i] == 0:
            i += 1
            continue
        j = i
        while j + 1 < n and status[j + 1] != 0:
            j += 1
        out.append((i, j, at))
        at += j - i + 1
        i = j + 1
    return out


def sparse_lookup_kind(ranges, i):
    """Where index i falls for IntSpan::at: 'inside', 'before' the first range, 'after' the last, 'between' two."""
    for a, b, _ in ranges:
        if a <= i <= b:
            return "inside"
    return "before" if i < ranges[0][0] else ("after" if i > ranges[-1][1] else "between")


# ---- areblockscnv (rsi.cpp:415-546) ------------------------------------------------------------------------------------------------------
def block_stage(case, tester=True):
    """The segments as the serial loop judges them, and rec: tests (every record, for the bounds), road per first-round test (what
    rsi_hot_debug_block_stage reports), stale[i] / serial[i] (the judgement against the list as it stood / as it stands), reach,
    rejected_end before test i, rescued, nested (per second-round segment: levels, absent, level0_skipped, chosen), reads (indices of the
    status array multisegments reads), info (the counters the hook must report)."""
    bins, status, P = case.depth, case.status, case.P
    a = (bins, case.span_all, case.RDmedian, P)
    T = copy_list(case.cands)
    N = len(T)
    rec = dict(tests=[], road=[], stale=[None] * N, serial=[None] * N, reach=[None] * N, serial_reach=[None] * N, rejected_before=[None] * N, rescued={}, nested={}, reads=[])
    sorted_ok = all(T[i - 1]["end"] < T[i]["start"] for i in range(1, N)) and all(c["status"] != -9 for c in T)
    batch = bool(tester) and sorted_ok and N >= BLOCK_BATCH_MIN
    rec["batch"], rec["sorted"] = batch, sorted_ok
    stale = [judge(*a, T, i, rec["tests"]) for i in range(N)] if batch else None
    rejected_end, hits = -1, 0
    for i in range(N):
        c, R = judge(*a, T, i, rec["tests"])
        rec["serial"][i], rec["rejected_before"][i] = dict(c), rejected_end
        rec["serial_reach"][i] = R["left_reach"]
        if batch:
            sc_, sR = stale[i]
            rec["stale"][i], rec["reach"][i] = sc_, sR["left_reach"]
            ok = sR["flags"][1] == 0
            if ok and not (sR["plan"]["cut"] & 1) and rejected_end < sR["left_reach"]:
                rec["road"].append(0)
                hits += 1
            else:
                rec["road"].append(4 if not ok else (3 if sR["plan"]["cut"] & 1 else 2))
        else:
            rec["road"].append(1)
        T[i] = c
        if c["status"] == -9 and c["end"] > rejected_end:
            rejected_end = c["end"]
    for i in range(N):
        if T[i]["status"] != -9:
            continue
        if (T[i]["type"] == DEL and T[i]["cnvmed"] < 0.7 * T[i]["refmed"]) or (T[i]["type"] == DUP and T[i]["cnvmed"] > 1.3 * T[i]["refmed"]):
            T[i]["geno"], T[i]["p1"] = 1, P["p"]
            rec["rescued"][i] = True
            continue
        rec["rescued"][i] = False
        original, chosen = dict(T[i]), dict(T[i])
        nrec = {}
        rec["reads"] += list(range(chosen["start"], chosen["end"] + 1))
        levels = [cand(s, e, chosen["type"], level=lv) for s, e, lv in nested_levels(chosen, status, nrec)]
        for j in range(len(levels) - 1, -1, -1):
            lv = levels[j].pop("level")
            T[i] = levels[j]
            levels[j], _ = judge(*a, T, i, rec["tests"])
            levels[j]["level"] = lv
        for j in range(len(levels) - 1, -1, -1):
            if levels[j]["geno"] == 0:
                continue
            if chosen["geno"] == 0:
                chosen = levels[j]
            if levels[j]["length"] > chosen["length"]:
                chosen = levels[j]
        if chosen["geno"] == 0:
            chosen = original
        nrec.update(levels=levels, chosen=dict(chosen), restored=chosen is original)
        rec["nested"][i] = nrec
        T[i] = {k: chosen[k] for k in FIELDS}
    rec["info"] = dict(block_batch_hits=hits, waits=1 if batch else 0, spec_hits=0, single_tests=0, host_fallbacks=0, sum_launches=0,
                       sum_reused=0, sum_redone=0, tests=0)
    return T, rec


# ---- mergesegments (rsi.cpp:694-885) -------------------------------------------------------------------------------------------------------
def new_counters():
    return dict(spec_hits=0, single_tests=0, host_fallbacks=0, block_batch_hits=0, waits=0, sum_launches=0, sum_reused=0, sum_redone=0, tests=0)


def _test(depth, RDmedian, P, T, i, K, rec, tester, spec=None, slot=-1, where=""):
    """test_bases: the test of T[i] in place; with a tester, which road it takes."""
    n = depth.size
    c, R = judge(depth, n, RDmedian, P, T, i, rec["tests"])
    if tester:
        K["tests"] += 1
        if spec is not None and slot >= 0 and spec["keys"][slot] == plan_key(n, n, P, T, i):
            K["spec_hits"] += 1
            rec["spec"].append((where, i, "hit", True))
        else:
            K["single_tests"] += 1
            K["waits"] += 1
            if spec is not None and slot >= 0:      # a result launched ahead is refused: what it would have given
                stale, _ = judge(depth, n, RDmedian, P, spec["lists"][slot], spec["index"][slot], rec["tests"])
                sk, k = spec["keys"][slot], plan_key(n, n, P, T, i)
                rec["spec"].append((where, i, "chains" if sk[:9] == k[:9] else "fields", same(stale, c)))
        if R["flags"][1] != 0:
            K["host_fallbacks"] += 1
    T[i] = c


def _mean(depth, lo, hi):
    return float(int(depth[lo:hi + 1].astype(np.int64).sum())) / float(hi - lo + 1)


def merge_stage(depth, L0, RDmedian, P, tester=True, K=None, rec=None):
    """The list after both passes, the counters and rec: tests, spec = (where, index, 'hit' / 'chains' / 'fields', stale result equals the
    serial one) per test that had a result launched ahead, sums = (pair, which of its three means came from the batch, the rule on the batch's sums or None without a slot, the
    serial rule) per near pair of the serial loop."""
    K = new_counters() if K is None else K
    rec = dict(tests=[], spec=[], sums=[], overlap=[], near=[]) if rec is None else rec
    L = copy_list(L0)
    a = (depth, RDmedian, P)
    for i in range(len(L) - 1):
        if L[i]["type"] != L[i + 1]["type"]:
            continue
        if not (max(L[i]["start"], L[i + 1]["start"]) < min(L[i]["end"], L[i + 1]["end"])):
            continue
        joined = dict(L[i], start=min(L[i]["start"], L[i + 1]["start"]), end=max(L[i]["end"], L[i + 1]["end"]))
        T = copy_list(L)
        T[i], T[i + 1] = dict(joined), dict(joined, status=-9)
        _test(*a, T, i, K, rec, tester)
        how = "union"
        if T[i]["geno"] == 0:
            T = copy_list(L)
            T[i + 1]["status"] = -9
            _test(*a, T, i, K, rec, tester)
            T[i]["status"], T[i + 1]["status"] = -9, 0
            _test(*a, T, i + 1, K, rec, tester)
            p_first, p_second = T[i]["p1"], T[i + 1]["p1"]
            how = "first"
            if T[i + 1]["p1"] < T[i]["p1"]:
                T[i] = dict(T[i + 1])
                how = "second"
            if T[i]["p1"] > P["p"]:
                L[i]["status"] = L[i + 1]["status"] = -9
                how = "both dropped"
            rec["overlap"].append((i, how, p_first, p_second, T[i]["geno"]))
        else:
            rec["overlap"].append((i, how, None, None, T[i]["geno"]))
        if T[i]["geno"] == 0:
            continue
        L[i], L[i + 1] = dict(T[i], status=-9), dict(T[i], status=0)
    L = [c for c in L if c["status"] != -9]
    if not P["merge"]:
        return L, K, rec

    def near_pair(i):
        if L[i]["type"] != L[i + 1]["type"] or L[i]["geno"] == 0 or L[i + 1]["geno"] == 0:
            return False
        gap = L[i + 1]["start"] - L[i]["end"]
        w1, w2 = L[i]["end"] - L[i]["start"], L[i + 1]["end"] - L[i + 1]["start"]
        return not (gap > w1 * P["chklen"] * 0.7 and gap > w2 * P["chklen"] * 0.7)

    npairs = max(0, len(L) - 1)
    ranges, sum_slot = [], [-1] * npairs
    if tester:
        for i in range(npairs):
            if near_pair(i):
                sum_slot[i] = len(ranges)
                ranges += [(L[i]["start"], L[i]["end"]), (L[i + 1]["start"], L[i + 1]["end"]), (L[i]["start"], L[i + 1]["end"])]
        if ranges:
            K["sum_launches"] += 1
            K["waits"] += 1

    def mean_of(slot, lo, hi, used):
        if slot >= 0 and ranges[slot] == (lo, hi):
            K["sum_reused"] += 1
            used.append(True)
        elif tester:
            K["sum_launches"] += 1
            K["sum_redone"] += 1
            K["waits"] += 1
            used.append(False)
        return _mean(depth, lo, hi)

    def rule(w1, w2, m1, m2, across, i):
        both = (m1 * w1 + m2 * w2) / (w1 + w2)
        if L[i]["type"] == DEL and across > both + 1.5 * L[i + 1]["refsd"] + 1.5 * L[i]["refsd"]:
            return False
        if L[i]["type"] == DUP and across < both - 1.5 * L[i + 1]["refsd"] - 1.5 * L[i]["refsd"]:
            return False
        return True

    def depth_rule(i, slot, used):
        w1, w2 = L[i]["end"] - L[i]["start"], L[i + 1]["end"] - L[i + 1]["start"]
        m1 = mean_of(slot, L[i]["start"], L[i]["end"], used)
        m2 = mean_of(-1 if slot < 0 else slot + 1, L[i + 1]["start"], L[i + 1]["end"], used)
        across = mean_of(-1 if slot < 0 else slot + 2, L[i]["start"], L[i + 1]["end"], used)
        return rule(w1, w2, m1, m2, across, i)

    def joined_list(i):
        T = copy_list(L)
        j = dict(L[i], end=L[i + 1]["end"])
        T[i], T[i + 1] = dict(j), dict(j, status=-9)
        return T

    spec, spec_slot = dict(keys=[], lists=[], index=[]), [-1] * npairs
    if tester:
        for i in range(npairs):
            if sum_slot[i] < 0 or not depth_rule(i, sum_slot[i], []):
                continue
            T = joined_list(i)
            spec_slot[i] = len(spec["keys"])
            spec["keys"].append(plan_key(depth.size, depth.size, P, T, i))
            spec["lists"].append(T)
            spec["index"].append(i)
        if spec["keys"]:
            K["waits"] += 1
    for i in range(len(L) - 1):
        if not near_pair(i):
            continue
        rec["near"].append(i)
        used = []
        passes = depth_rule(i, sum_slot[i] if tester else -1, used)
        stale = None
        if tester and sum_slot[i] >= 0:      # what the batch's sums would give for this pair, whether their ranges still hold or not:
            s = sum_slot[i]                  # a slot's sum divided by the length of the range that is asked for
            w1, w2 = L[i]["end"] - L[i]["start"], L[i + 1]["end"] - L[i + 1]["start"]
            asked = ((L[i]["start"], L[i]["end"]), (L[i + 1]["start"], L[i + 1]["end"]), (L[i]["start"], L[i + 1]["end"]))
            sums = [int(depth[ranges[s + k][0]:ranges[s + k][1] + 1].astype(np.int64).sum()) for k in range(3)]
            stale = rule(w1, w2, *(float(sums[k]) / float(asked[k][1] - asked[k][0] + 1) for k in range(3)), i)
        rec["sums"].append((i, tuple(used), stale, passes))
        if not passes:
            continue
        T = joined_list(i)
        _test(depth, RDmedian, P, T, i, K, rec, tester, spec, spec_slot[i], "merge")
        if T[i]["geno"] == 0:
            continue
        L[i], L[i + 1] = dict(T[i], status=-9), dict(T[i])
    L = [c for c in L if c["status"] != -9]
    return L, K, rec


# ---- detectcnv behind the block tests (rsi.cpp:1860-1931) and sd_filters (rsi.cpp:1753-1792) ---------------------------------------------------
def order_by_start(L):
    """sortcnvstartposition (rsi.cpp:549-577): start <= end, then a stable sort by start."""
    L = [dict(c, start=min(c["start"], c["end"]), end=max(c["start"], c["end"])) for c in L]
    return sorted(L, key=lambda c: c["start"])


def to_reference(noncode, p):
    """expand_coordinate (rsi.cpp:1524-1551) as host_calls.cpp restates it."""
    removed = 0
    for s, e in noncode:
        grown = removed + (e - s + 1)
        if p < e + 1 - grown:
            break
        removed = grown
    return p + removed


def sd_filters(raw, m, RDmedian, RDsd, rec=None):
    kept = []
    minlen = max(m * 2, 500)
    sd = RDsd / 1.2
    for c in raw:
        span = abs(c["end"] - c["start"])
        keep = not (span < 1000)
        rescue = False
        if c["type"] == DEL:
            if c["p1"] > 0.2 or c["refsd"] > 0.6 * sd or c["cnvsd"] > 1.3 * sd:
                keep = False
            if c["cnvsd"] * RDmedian > 2.5 * c["cnvmed"] * sd:
                keep = False
            if c["cnvmed"] < 0.66 * min(RDmedian, c["refmed"]) and c["cnvsd"] < sd and span > 800:
                keep = rescue = True
        if c["type"] == DUP:
            if c["p1"] > 0.05 or c["refsd"] > 0.6 * sd:
                keep = False
            if c["cnvsd"] * RDmedian > 2.0 * c["cnvmed"] * sd:
                keep = False
        if span < minlen:
            keep = False
        if rec is not None:
            rec.append((span, keep, rescue))
        if keep:
            kept.append(dict(c))
    return kept


def calls_stage(case, tester=True):
    """(blocks, raw, kept, counters, rec).  rec: tests, spec, sums (as merge_stage), sharpened (the list before the merge), merged (the
    list before the final tests), tested (that list after them, rejected entries included), sharpen (cand_cases-style reports), filters."""
    depth, P = case.depth, case.P
    n, m = depth.size, P["m"]
    K = new_counters()
    rec = dict(tests=[], spec=[], sums=[], overlap=[], near=[], sharpen=[], filters=[], dropped=[], judged=[])
    S = order_by_start(case.cands)
    blocks = copy_list(S)
    L = []
    for k, c in enumerate(S):
        if c["geno"] == 0 or c["start"] == c["end"]:
            rec["dropped"].append(k)
            continue
        c = dict(c, start=c["start"] * m + m // 2, end=c["end"] * m + m // 2)
        c["start"], c["end"] = max(c["start"], 0), min(c["end"], n - 1)
        c["length"] = c["end"] - c["start"] + 1
        L.append(c)
    rec["based"] = copy_list(L)
    for c in L:
        c["start"], c["end"], reps = sc.refine(depth, c["start"], c["end"], c["type"])
        rec["sharpen"].append(reps)
    if tester and L:
        K["waits"] += 1
    rec["before_order"] = copy_list(L)
    L = order_by_start(L)
    rec["sharpened"] = copy_list(L)
    L, K, rec = merge_stage(depth, L, case.RDmedian, P, tester, K, rec)
    L = order_by_start(L)
    rec["merged"] = copy_list(L)
    spec = None
    if tester:
        spec = dict(keys=[plan_key(n, n, P, L, i) for i in range(len(L))], lists=[copy_list(L)] * len(L), index=list(range(len(L))))
        if L:
            K["waits"] += 1
    raw = []
    nc = [tuple(int(x) for x in r) for r in case.noncode]
    for i in range(len(L)):
        nbins = float(L[i]["end"] - L[i]["start"] + 1) / float(m)
        _test(depth, case.RDmedian, P, L, i, K, rec, tester, spec, i if tester else -1, "final")
        rec["judged"].append(dict(L[i]))
        L[i]["score"] = (L[i]["cnvmed"] - case.RDmedian) * math.sqrt(nbins)
        r1, r2 = to_reference(nc, L[i]["start"]), to_reference(nc, L[i]["end"])
        if any(max(r1, s) <= min(r2, e) for s, e in nc):
            L[i]["status"] = -9
        if L[i]["status"] != -9:
            raw.append(dict(L[i]))
    rec["tested"] = copy_list(L)
    for c in raw:
        c["start"], c["end"] = to_reference(nc, c["start"]), to_reference(nc, c["end"])
    kept = sd_filters(raw, m, case.RDmedian, case.RDsd, rec["filters"])
    return blocks, raw, kept, K, rec


_restated = {}


def restated(case, tester=True):
    """Computed once per (case, tester) and shared.  block: (segments, rec); merge: (list, counters, rec); calls: calls_stage's tuple."""
    key = (case.name, bool(tester))
    if key not in _restated:
        if case.stage == "block":
            _restated[key] = block_stage(case, tester)
        elif case.stage == "merge":
            _restated[key] = merge_stage(case.depth, case.cands, case.RDmedian, case.P, tester)
        else:
            _restated[key] = calls_stage(case, tester)
    return _restated[key]


def all_tests(case):
    r = restated(case)
    return r[-1]["tests"]


# ---- building ------------------------------------------------------------------------------------------------------------------------------
def body_values(kind, rng, k):
    return rng.integers(10, 21, k) if kind == DEL else rng.integers(45, 61, k)


def shallow(kind):
    """A value a test rejects (nu on the wrong side of 0) and the second round does not rescue against a neighbourhood of 30."""
    return 24 if kind == DEL else 35


_cases = None


def _build():
    C = []

    def add(name, stage, claim, depth, cands, status=None, noncode=(), span_all=None, RDmedian=30.0, RDsd=6.0, P=None, **expect):
        PP = dict(DEFAULT_P)
        PP.update(P or {})
        depth = np.ascontiguousarray(depth, dtype=np.int32)
        assert depth.min() >= 0
        assert depth.size <= (4000 if stage == "block" else 300_000), name
        st = None if status is None else np.ascontiguousarray(status, dtype=np.int32)
        C.append(Case(name, stage, claim, depth, st, copy_list(cands), np.array(noncode, dtype=np.int32).reshape(-1, 2),
                      int(depth.size if span_all is None else span_all), float(RDmedian), float(RDsd), PP, expect))

    for kind, tag in KINDS:
        sign = -1 if kind == DEL else 1

        # ================================ block stage ==========================================================================================
        def bin_scene(nseg, seed, spacing=60, length=8, first=40, weak=(), weak_value=None, nb=None, moved=None):
            """nseg segments of `length` bins every `spacing` bins; the segments listed in `weak` carry a value a test rejects.  moved:
            {k: start} puts segment k elsewhere."""
            rng = np.random.default_rng(seed)
            nb_ = first + nseg * spacing + 60 if nb is None else nb
            d = rng.integers(25, 36, nb_).astype(np.int64)
            st = np.zeros(nb_, dtype=np.int64)
            segs = []
            for k in range(nseg):
                a = first + k * spacing if not moved or k not in moved else moved[k]
                b = a + length - 1
                d[a:b + 1] = (shallow(kind) if weak_value is None else weak_value) if k in weak else body_values(kind, rng, length)
                st[a:b + 1] = sign * 2
                segs.append(cand(a, b, kind, score=float(sign * 10)))
            return d, st, segs

        # 23 against 24 segments: the batch's threshold
        for nseg in (23, 24):
            d, st, segs = bin_scene(nseg, 200 + nseg)
            add(f"block_{nseg}_{tag}", "block", f"{nseg} sorted segments: " + ("no batch" if nseg < 24 else "one batch, every result used"), d, segs, st,
                span_all=101 * d.size, batch=nseg >= 24, hits=nseg if nseg >= 24 else 0)
        # unsorted, and a list that already holds a -9
        d, st, segs = bin_scene(26, 231)
        segs[3], segs[4] = segs[4], segs[3]
        add(f"block_unsorted_{tag}", "block", "26 segments, two of them out of order: the batch is refused", d, segs, st, span_all=101 * d.size, batch=False, hits=0)
        d, st, segs = bin_scene(26, 232)
        segs[7]["status"] = -9
        add(f"block_holds_rejected_{tag}", "block", "26 segments, one already rejected: the batch is refused", d, segs, st, span_all=101 * d.size, batch=False,
            hits=0)
        # a rejected segment just left of where the next test's left walk ended, and inside it.  Segments of 8 bins: margin 1, 20 slots on
        # the left.  Segment 10 is weak (rejected); segment 11 sits `gap` bins behind it: its stale walk (segment 10 jumped) takes the `gap - 1`
        # bins between them and the rest from behind segment 10; with gap = 22 it fills at the bin right of segment 10's end.
        for gap, name in ((22, "outside"), (21, "inside_by_one"), (12, "inside")):
            a10 = 40 + 10 * 60
            d, st, segs = bin_scene(26, 240 + gap, weak=(10,), weak_value=22 if kind == DEL else 35, moved={11: a10 + 7 + gap})
            add(f"block_reach_{name}_{tag}", "block", f"segment 10 is rejected, segment 11 starts {gap} bins behind its end", d, segs, st, span_all=101 * d.size,
                batch=True, rejected=10, probe=11, reach_case=name)
        # more than 48 segments to the left: the left chain is cut, the batch's result is not used
        d, st, segs = bin_scene(60, 250, spacing=40)
        add(f"block_cut_{tag}", "block", "60 segments: from index 49 on the left chain is cut at 48 entries", d, segs, st, span_all=101 * d.size, batch=True,
            cut_from=49)
        # a rejected segment at index 0 within reach of test 1: never skipped by the pointer, so the stale judgement equals the serial one,
        # and is refused all the same
        d, st, segs = bin_scene(26, 251, weak=(0,), moved={1: 40 + 8 + 10})
        add(f"block_rejected_first_{tag}", "block", "segment 0 is rejected, segment 1 starts 10 bins behind it: refused, though index 0 is never skipped", d, segs, st,
            span_all=101 * d.size, batch=True, rejected=0, probe=1, first=True)
        # the second round's rescue at 0.7 / 1.3 refmed: a neighbourhood of 31 .. 34 (DEL) / 25 .. 28 (DUP) around a constant segment
        for value, rescued in (((22, True), (23, False)) if kind == DEL else ((35, True), (34, False))):
            rng = np.random.default_rng(260 + value)
            d = rng.integers(31, 35, 400) if kind == DEL else rng.integers(25, 29, 400)
            st = np.zeros(400, dtype=np.int64)
            segs = []
            for a in (100, 200, 300):
                d[a:a + 8] = value if a == 200 else body_values(kind, rng, 8)
                st[a:a + 8] = sign * 2
                segs.append(cand(a, a + 7, kind, score=float(sign * 10)))
            add(f"block_rescue_{value}_{tag}", "block", f"a rejected segment of constant {value}: " + ("rescued" if rescued else "not rescued") + " by the 0.7 / 1.3 refmed rule",
                d, segs, st, span_all=101 * 400, rescued=rescued, probe=1)
        # nested levels.  Segment 1 of three is 22 bins: A (3 bins, level 1), a zero, B (5 bins, level 2), a zero, C (8 bins, level 4), a zero,
        # D (3 bins, level 5).  A level's runs are those of all levels up to it, the last run never emitted, and the loop stops one short of
        # the highest level (a deletion's 0, from the zeros inside): level 1 -> nothing; 2 -> A; 3 absent; 4 -> A, B; 5 (deletions only) ->
        # A, B, C.  With one bin of the other sign in C the range of levels crosses 0.  deep: the runs whose values pass a test.
        for name, deep, other_sign, expect in (("longest", ("A", "B"), False, dict(chosen="B", restored=False)),
                                                ("none", (), False, dict(chosen=None, restored=True)),
                                                ("level0", ("A",), True, dict(chosen="A", restored=False, level0=True))):
            rng = np.random.default_rng(270)
            nb_ = 700
            d = rng.integers(25, 36, nb_).astype(np.int64)
            st = np.zeros(nb_, dtype=np.int64)
            a = 300
            runs = dict(A=(a, a + 2, 1), B=(a + 4, a + 8, 2), C=(a + 10, a + 17, 4), D=(a + 19, a + 21, 5))
            d[a:a + 22] = shallow(kind) + (2 if kind == DEL else -2)
            for r, (s, e, lv) in runs.items():
                st[s:e + 1] = sign * lv
                if r in deep:
                    d[s:e + 1] = body_values(kind, rng, e - s + 1)
            if other_sign:
                st[a + 15] = -sign
            # segment 0 starts two bins in front of its marks, segment 2 ends two bins behind them: the sparse form is asked in front of its
            # first and behind its last range; both are weak, so the second round reads their status
            segs = [cand(98, 109, kind), cand(a, a + 21, kind), cand(600, 611, kind)]
            for s, e in ((100, 109), (600, 609)):
                st[s:e + 1] = sign * 2
            st[103] = sign * 3
            st[603] = sign * 3
            d[98:110] = shallow(kind)
            d[600:612] = shallow(kind)
            add(f"block_levels_{name}_{tag}", "block", f"nested levels of a rejected segment: runs A (level 1), B (2), C (4), D (5), deep: {deep or 'none'}", d, segs, st,
                span_all=101 * nb_, probe=1, runs=runs, sparse=True, **expect)

        # ================================ merge ================================================================================================
        def base_scene(n, seed, bodies, fills=()):
            """depth[n] uniform 25 .. 35; bodies = (start, end) filled with the kind's values; fills = (start, end, value or (lo, hi))."""
            rng = np.random.default_rng(seed)
            d = rng.integers(25, 36, n).astype(np.int64)
            for s, e in bodies:
                d[s:e + 1] = body_values(kind, rng, e - s + 1)
            for s, e, v in fills:
                d[s:e + 1] = rng.integers(v[0], v[1] + 1, e - s + 1) if isinstance(v, tuple) else v
            return d

        ok = dict(geno=1, status=1, p1=0.001, refsd=1.0)
        other = DUP if kind == DEL else DEL
        mild = (24, 29) if kind == DEL else (31, 36)            # a median on the candidate's side of 30 that a test rejects

        d = base_scene(20000, 300, [(8000, 8400), (8300, 8800)])
        add(f"merge_types_differ_{tag}", "merge", "two overlapping candidates of different type: left alone", d,
            [cand(8000, 8400, kind, **ok), cand(8300, 8800, other, **ok)], P=dict(merge=0), out=2, tests=0)
        add(f"merge_overlap_union_{tag}", "merge", "two overlapping candidates whose union passes: one candidate, the union", d,
            [cand(8000, 8400, kind, **ok), cand(8300, 8800, kind, **ok)], out=1, overlap=["union"], union=(8000, 8800))
        # the union fails, each is tested alone: the lower p1 wins
        d = base_scene(20000, 301, [(8000, 8300)], fills=[(8301, 9200, mild)])
        add(f"merge_overlap_first_wins_{tag}", "merge", "the union fails; the first alone passes, the second does not: both become the first", d,
            [cand(8000, 8300, kind, **ok), cand(8200, 9200, kind, **ok)], overlap=["first"], out=1, union=(8000, 8300))
        d = base_scene(20000, 302, [(8900, 9200)], fills=[(8000, 8899, mild)])
        add(f"merge_overlap_second_wins_{tag}", "merge", "the union fails; the second alone has the lower p1: both become the second", d,
            [cand(8000, 9000, kind, **ok), cand(8900, 9200, kind, **ok)], overlap=["second"], out=1, union=(8900, 9200))
        # both alone fail with p1 above P.p: both are dropped; with a constant neighbourhood both p1 are exactly 1 (equal p1: the first stays)
        d = base_scene(20000, 303, [], fills=[(8000, 9200, mild)])
        add(f"merge_overlap_both_dropped_{tag}", "merge", "the union fails and both alone have p1 above P.p: both are dropped", d,
            [cand(8000, 8700, kind, **ok), cand(8600, 9200, kind, **ok)], overlap=["both dropped"], out=0)
        d = np.full(20000, 30, dtype=np.int64)
        d[8000:9201] = 27 if kind == DEL else 33
        add(f"merge_overlap_equal_p1_{tag}", "merge", "a constant neighbourhood: both alone end with p1 = 1 exactly, equal: the first stays, and both are dropped", d,
            [cand(8000, 8700, kind, **ok), cand(8600, 9200, kind, **ok)], overlap=["both dropped"], out=0, equal_p1=True)
        # equal p1 at or below P.p: the tie rule of the strict p1 < p1 (the first stays).  Each candidate alone has its median on the other
        # side of 30 (the overlap, more than half of each, carries such values): the test ends on the type contradiction with geno 1 and
        # leaves p1 as the caller gave it, the same for both.  The union's median lies on the candidate's side (the two outer parts are the
        # majority there) and too close to 30: the union fails
        wrong = (31, 36) if kind == DEL else (24, 29)
        d = base_scene(20000, 310, [], fills=[(8000, 8399, mild), (8400, 8899, wrong), (8900, 9299, mild)])
        add(f"merge_overlap_tie_{tag}", "merge", "the union fails, both alone keep the caller's p1 = 0.001: equal, at most P.p, the first stays", d,
            [cand(8000, 8899, kind, **ok), cand(8400, 9299, kind, **ok)], overlap=["first"], out=1, union=(8000, 8899), tie=True)
        # a chain of three overlapping candidates
        d = base_scene(20000, 304, [(8000, 9300)])
        add(f"merge_overlap_chain_{tag}", "merge", "three candidates, each overlapping the next: one union of all three", d,
            [cand(8000, 8500, kind, **ok), cand(8400, 8900, kind, **ok), cand(8800, 9300, kind, **ok)], overlap=["union", "union"], out=1, union=(8000, 9300))
        # the gap rule: gap > 0.7 chklen w for BOTH widths leaves the pair alone; w = end - start
        for w1, w2 in ((400, 200), (200, 400)):
            for dg in (-1, 0, 1):
                gap = 700 + dg
                s2 = 8000 + w1 + gap
                d = base_scene(20000, 305, [(8000, 8000 + w1), (s2, s2 + w2)])
                add(f"merge_gap_{w1}_{w2}_{gap}_{tag}", "merge", f"widths {w1} and {w2}, gap {gap} against 0.7 x 2.5 x 400 = 700", d,
                    [cand(8000, 8000 + w1, kind, **ok), cand(s2, s2 + w2, kind, **ok)], near=dg <= 0)
        for which in (0, 1):
            d = base_scene(20000, 306, [(8000, 8400), (8500, 8900)])
            L = [cand(8000, 8400, kind, **ok), cand(8500, 8900, kind, **ok)]
            L[which]["geno"] = 0
            add(f"merge_geno0_{which}_{tag}", "merge", f"a near pair whose member {which} has geno 0: left alone", d, L, near=False, out=2)
        # the depth rule on both sides of its inequality: refsd chosen from the pair's exact means
        d = base_scene(20000, 307, [(8000, 8400), (8500, 8900)])
        m1, m2, across = _mean(d, 8000, 8400), _mean(d, 8500, 8900), _mean(d, 8000, 8900)
        diff = abs(across - (m1 * 400 + m2 * 400) / 800)
        for side, r in (("joins", diff / 3 * 1.001), ("apart", diff / 3 * 0.999)):
            add(f"merge_depth_rule_{side}_{tag}", "merge", f"the gap's depth moves the joint mean by {diff:.4f}: refsd {r:.5f} on each side", d,
                [cand(8000, 8400, kind, **dict(ok, refsd=r)), cand(8500, 8900, kind, **dict(ok, refsd=r))], rule=side == "joins", near=True)
        add(f"merge_off_{tag}", "merge", "P.merge = 0: near pairs are left alone", d,
            [cand(8000, 8400, kind, **dict(ok, refsd=9.0)), cand(8500, 8900, kind, **dict(ok, refsd=9.0))], P=dict(merge=0), out=2, tests=0)
        # three near candidates; the first pair merges, so the second pair's members changed: its three sums are taken again and the test
        # launched ahead for it is refused.  The gap between the first two carries values far on the other side of 30 (not extreme): the
        # merged candidate's mean differs from the second candidate's alone, and refsd of the third is set between the two rules
        far = 80 if kind == DEL else 5
        d = base_scene(30000, 308, [(10000, 10400), (10441, 10840), (10900, 11300)], fills=[(10401, 10440, far), (10841, 10899, far)])
        a = [(10000, 10400), (10441, 10840), (10900, 11300)]
        jd, _ = judge(d.astype(np.int32), 30000, 30.0, DEFAULT_P,
                      [cand(10000, 10840, kind, **ok), cand(10000, 10840, kind, **dict(ok, status=-9)), cand(10900, 11300, kind, **ok)], 0)

        def excess(lo1, hi1, lo2, hi2):
            w1, w2 = hi1 - lo1, hi2 - lo2
            return abs(_mean(d, lo1, hi2) - (_mean(d, lo1, hi1) * w1 + _mean(d, lo2, hi2) * w2) / (w1 + w2))
        true_x = excess(10000, 10840, 10900, 11300)
        w1, w2 = 10840 - 10000, 400                # the stale sums, divided by the lengths of the ranges asked for
        s = lambda lo, hi: float(int(d[lo:hi + 1].sum()))
        stale_x = abs(s(10441, 11300) / (11300 - 10000 + 1) - (s(10441, 10840) / (w1 + 1) * w1 + _mean(d, 10900, 11300) * w2) / (w1 + w2))
        r3 = (true_x + stale_x) / 2 / 1.5 - jd["refsd"]
        assert r3 > 0 and min(true_x, stale_x) < 1.5 * (r3 + jd["refsd"]) < max(true_x, stale_x)
        add(f"merge_chain_redone_{tag}", "merge", "three near candidates, the first pair merges: the second pair's sums and its test are redone", d,
            [cand(*a[0], kind, **dict(ok, refsd=50.0)), cand(*a[1], kind, **dict(ok, refsd=50.0)), cand(*a[2], kind, **dict(ok, refsd=r3))],
            redone_pair=1, stale_rule_differs=True)
        # four candidates: pair (0, 1) merges; the third's small refsd keeps the depth rule from joining it to them; pair (2, 3) keeps its members, so its sums are reused, but the neighbours its test jumps over
        # changed: the gap between 0 and 1 (values far from 30) is no longer walked through.  Its result launched ahead is refused by the
        # chains alone, and would have been another
        d = base_scene(30000, 309, [(10000, 10400), (10441, 10840), (11640, 12040), (12140, 12540)], fills=[(10401, 10440, far)])
        add(f"merge_chains_changed_{tag}", "merge", "pair (0, 1) merges; pair (2, 3)'s sums hold, its test launched ahead does not: the chains changed", d,
            [cand(10000, 10400, kind, **dict(ok, refsd=50.0)), cand(10441, 10840, kind, **dict(ok, refsd=50.0)),
             cand(11640, 12040, kind, **dict(ok, refsd=1.0)), cand(12140, 12540, kind, **dict(ok, refsd=50.0))],
            spec_refused_by="chains", stale_test_differs=True, reused_pair=2)

        # ================================ behind the blocks ====================================================================================
        tested = dict(geno=1, status=1, p1=0.001)
        m = 101

        def bins(a, b):                      # the bases a segment of bins a .. b becomes
            return a * m + m // 2, b * m + m // 2

        # clamps, dropped segments, the final tests' speculation; step-shaped bodies so that the edge refinement lands on the steps
        n = 60000
        segs = [cand(40, 52, kind, **tested), cand(70, 70, kind, **tested), cand(90, 99, kind, **dict(tested, geno=0)), cand(200, 212, kind, **tested),
                cand(400, 412, kind, **tested), cand(585, 594, kind, **tested)]
        d = base_scene(n, 320, [bins(40, 52), bins(200, 212), bins(400, 412), (bins(585, 594)[0], n - 1)])
        add(f"calls_clamp_drop_{tag}", "calls", "a segment whose end is clamped to n - 1, one of one bin and one with geno 0 (both dropped)", d, segs,
            noncode=[(0, 999), (30000, 30999)], clamped=True, dropped=[1, 2])
        # a final test that rejects candidate i, so that the plan of i + 1 changes: i in the middle, at index 0 and next to the last index
        for where, weak_at in (("middle", 1), ("first", 0), ("before_last", 2), ("last", 3)):
            pos = [(100, 112), (125, 137), (150, 162), (175, 187)]
            weakb = bins(*pos[weak_at])
            d = base_scene(n, 330 + weak_at, [bins(*p) for k, p in enumerate(pos) if k != weak_at],
                           fills=[(weakb[0], weakb[1], (22, 23) if kind == DEL else (35, 36))])
            segs = [cand(a, b, kind, **tested) for a, b in pos]
            add(f"calls_final_rejects_{where}_{tag}", "calls", f"the final test rejects candidate {weak_at} of four", d, segs, P=dict(merge=0), weak=weak_at)
        # to_reference at every junction; a call whose expanded end meets a region's start, and one base before it
        regs = [(0, 999), (5000, 5999), (20000, 20099)]
        d = base_scene(n, 340, [bins(100, 112), bins(140, 152), bins(175, 185)])
        add(f"calls_regions_{tag}", "calls", "three regions, the first from 0: coordinates go back onto the reference; the last call spans a junction", d,
            [cand(100, 112, kind, **tested), cand(140, 152, kind, **tested), cand(175, 185, kind, **tested)], noncode=regs, P=dict(merge=0), junctions=True,
            spanning=2)
        # sd_filters' spans.  Constant depth with a constant body between two steps: a candidate shorter than the body is carried onto the
        # steps exactly (start on the last base in front of the body, end on the first base behind it).  With m = 451 no candidate made of whole bins
        # has both steps within the refinement's reach: there the call ends on n - 1 (the clamp), which the refinement leaves alone
        def step_scene(lo, hi, size=n):
            d = np.full(size, 30, dtype=np.int64)
            d[lo:hi + 1] = 15 if kind == DEL else 50
            return d
        a0 = 198 * m + m // 2 - 20
        for span in (499, 500, 800, 801, 999, 1000):
            b1 = (a0 + span - 1 - 10 - m // 2) // m
            add(f"calls_span_{span}_{tag}", "calls", f"a constant body whose refined call has span {span}", step_scene(a0 + 1, a0 + span - 1),
                [cand(198, b1, kind, **tested)], RDsd=12.0, span=span)
        for span in (901, 902):                      # max(2 m, 500) = 902 with m = 451
            start = 40 * 451 + 225
            size = start + span + 1
            add(f"calls_minlen_{span}_{tag}", "calls", f"m = 451: a call of span {span} that ends on n - 1, against max(2 m, 500) = 902",
                step_scene(start, size - 1, size), [cand(40, 43, kind, **tested)], RDsd=12.0, P=dict(m=451), span=span, clamped=True)
        # to_reference and the N-region filter AT the junctions.  m = 1, so that a segment's bins are bases: a constant body between two steps
        # whose refined call starts on `first` and ends on `last` (the refinement lands on the last base in front of the body and on the
        # first behind it).  Compacted junctions of `regs`: 0, 4000 and 18000; position j - 1 expands to the base in front of the region, j to
        # the first base behind it.  A call that ends on j - 1 or starts on j is kept; one with j inside (first, last] spans the region
        for j in (4000, 18000):
            for edge in ("start", "end"):
                for off in (-1, 0, 1):
                    first, last = (j + off, j + off + 1200) if edge == "start" else (j + off - 1200, j + off)
                    add(f"calls_junction_{j}_{edge}_{'m1' if off < 0 else 'p' + str(off)}_{tag}", "calls",
                        f"m = 1: a call whose {edge} is refined onto {j} {off:+d}, junction {j}", step_scene(first + 1, last - 1),
                        [cand(first + 20, last - 20, kind, **tested)], noncode=regs, RDsd=12.0, P=dict(m=1), edges=(first, last), junction=j,
                        kept=not (first < j <= last))
        # the region that starts at 0: junction 0.  So close to the array's start the refinement returns at once: the call is its segment
        for first in (0, 1):
            add(f"calls_junction_0_start_p{first}_{tag}", "calls", f"m = 1: a call that starts on {first}, behind the region that starts at 0",
                step_scene(first, 1200), [cand(first, 1200, kind, **tested)], noncode=regs, RDsd=12.0, P=dict(m=1), edges=(first, 1200), junction=0,
                kept=True, unrefined=True)
        # the first call of the refinement leaves end < start (a bump inside both searches of a deletion, a dip for a duplication); the
        # reference's second call then indexes its vector out of range, so `refined` is not in the golden file for this case and the
        # restatement's rule judges it (sharpen_cases' group `crossed`); the list is put in order by the swap, and the reference answers
        # the stages behind it
        a0, b0, sg = (1400, 1450, 1) if kind == DEL else (1380, 1460, -1)
        add(f"calls_refined_crossed_{tag}", "calls", "m = 1: the edge refinement leaves end < start; start and end are swapped when the list is ordered",
            sc.stepped(3000, 60, [(a0, 30 * sg), (b0, -30 * sg)]), [cand(1350, 1449, kind, **tested)], RDmedian=60.0, RDsd=12.0, P=dict(m=1, merge=0),
            crossed_refine=True)
        # the refinement carries the first candidate's start to the right past the second's; the second, of the other type, keeps its start
        add(f"calls_starts_cross_{tag}", "calls", "the edge refinement carries the first start past the second: the list is put in order again", step_scene(10400, 12400),
            [cand(100, 118, kind, **tested), cand(101, 102, other, **tested)], P=dict(merge=0), crossed=True)
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
    return (1, 4) if int(case.depth.max()) <= 255 else (4,)


def junction_positions(noncode, n):
    """Compacted positions exactly at, and one either side of, every junction of to_reference."""
    out, removed = [], 0
    for s, e in noncode:
        removed += e - s + 1
        j = e + 1 - removed
        out += [p for p in (j - 1, j, j + 1) if 0 <= p < n]
    return sorted(set(out))


# ---- the golden file ---------------------------------------------------------------------------------------------------------------------
def pack(L):
    return (np.array([[c[k] for k in INTS] for c in L], dtype=np.int32).reshape(-1, len(INTS)),
            np.array([[c[k] for k in FLOATS] for c in L], dtype=np.float64).reshape(-1, len(FLOATS)))


def unpack(ints, floats):
    return [dict(**{k: int(v) for k, v in zip(INTS, a)}, **{k: float(v) for k, v in zip(FLOATS, b)}) for a, b in zip(ints, floats)]


def load_golden(path=GOLDEN):
    """name -> part -> list of candidate dicts (parts: 'out' for block and merge cases; 'merged', 'tested', 'kept' for calls cases) and
    'expand' -> int array for calls cases."""
    z = np.load(path)
    out = {}
    for key in z.files:
        if key.endswith("/i"):
            name, part, _ = key.rsplit("/", 2)
            out.setdefault(name, {})[part] = unpack(z[key], z[f"{name}/{part}/f"])
        elif key.endswith("/expand"):
            out.setdefault(key.rsplit("/", 1)[0], {})["expand"] = z[key]
    return out
