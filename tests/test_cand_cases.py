"""CPU: the cases of tests/cand_cases.py are what they claim to be, and the restatement of isitcnvwrap + isitcnv they are judged by equals
the compiled reference's answers (golden/cand_edges.npz): type, status, geno and the six quantile-derived columns bit for bit, p1 and cnvsd
at the project's rtol = 1e-6.  Nothing here touches the library's device code."""
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import cand_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXACT, CLOSE = cc.EXACT, cc.CLOSE


@pytest.fixture(scope="module")
def golden():
    return cc.load_golden()


def one(case):
    assert len(case.index) == 1, case.name
    return cc.restated(case)[case.index[0]]


def both(name):
    return [cc.get_case(f"{name}_{tag}") for _, tag in cc.KINDS]


def test_the_constants_are_the_librarys():
    src = lambda f: open(os.path.join(ROOT, "rsicnv_amd", "csrc", f)).read()
    kc, kh, hc, pl = src("kernels_cand.hip"), src("kernels.h"), src("host_calls.cpp"), src("pipeline.hip")
    assert "constexpr int kChainMax = 48;" in hc and cc.CHAIN_MAX == 48
    assert "constexpr unsigned kCandHistBins = 16384;" in kh and cc.HIST_BINS == 16384
    assert "constexpr int kCandChunks = 16;" in kh and cc.CHUNKS == 16
    assert re.search(r"constexpr int kTestThreads = 1024;", kc + kh + src("device_util.h")) and cc.THREADS == 1024
    assert "static constexpr int kPer = 16;" in kc and "static constexpr int kPer = 64;" in kc and cc.PER == {4: 16, 1: 64}
    assert cc.TRIP == {4: 16384, 1: 65536}
    assert "if (avail >= 2LL * (T.top + 1) + 64) *cut |= 4;" in hc
    assert "const long long fit = 4ll * g.nref / g.width;" in kc
    assert "return (((nwin + chunks - 1) / chunks) + 3) & ~3;" in kc and "return (((n + kCandChunks - 1) / kCandChunks) + 3) & ~3;" in kc
    assert "if (nbk > kCandHistBins) O.flags |= 2;" in kc and "if (nbk > kCandHistBins) O.flags |= 4;" in kc
    assert 'Timer t(ctx, split ? (wide ? "candidate_test_i32" : "candidate_test") : (wide ? "candidate_test_one_wg_i32" : "candidate_test_one_wg"));' in pl
    assert cc.trip_position(16383, 4) == (0, 1023, 15, 63, 15) and cc.trip_position(16384, 4) == (1, 0, 0, 0, 0)
    assert cc.trip_position(65535, 1) == (0, 1023, 63, 63, 15) and cc.trip_position(65536, 1) == (1, 0, 0, 0, 0)
    assert cc.trip_position(1024, 4) == (0, 64, 0, 0, 1) and cc.trip_position(4095, 1) == (0, 63, 63, 63, 0)
    assert [cc.kernel_name(s, f) for s, f in ((1, 1), (1, 0), (1, 3), (1, 2), (4, 1), (4, 0))] == \
        ["candidate_test", "candidate_test_one_wg", "candidate_test_i32", "candidate_test_one_wg_i32", "candidate_test", "candidate_test_one_wg"]


def test_restatement_equals_the_reference(golden):
    assert set(golden) == {c.name for c in cc.all_cases() if cc.in_golden(c)}
    n = 0
    for c in cc.all_cases():
        if not cc.in_golden(c):
            continue
        recs = cc.restated(c)
        assert len(golden[c.name]) == len(c.index), c.name
        for ci, g in zip(c.index, golden[c.name]):
            j = recs[ci]["judged"]
            for k in ("type", "status", "geno"):
                assert g[k] == j[k], (c.name, ci, k, g[k], j[k])
            for k in EXACT:
                assert g[k] == j[k], (c.name, ci, k, g[k], j[k])
            for k in CLOSE:
                assert np.isclose(g[k], j[k], rtol=1e-6, atol=1e-300), (c.name, ci, k, g[k], j[k])
            n += 1
    assert n > 2000


def test_no_decision_rests_on_the_tolerance():
    """The sign of nu is the sign of its numerator, a combination of grid values that are compared bit for bit; it is asserted away
    from 0 by far more than the last bits of a median taken as a mean could move it.  The spread's floor (1e-3) is taken either for a
    variance of exactly 0 (constant means: every sum exact in any order) or for one whose distance from 1e-6 is a hundred times what the
    order of the sums can move s2 / n - mu^2 by, n 2^-53 max^2."""
    floor_taken = 0
    for c in cc.all_cases():
        for ci, r in cc.restated(c).items():
            if r["empty"] or r["nu"] is None:
                continue
            assert abs(r["nu_num"]) > 1e-3 * r["nu_scale"], (c.name, ci, r["nu_num"])
            assert r["ref_var"] >= 0 and r["cnv_var"] >= 0, (c.name, ci)
            sd = math.sqrt(r["ref_var"])
            assert r["ref_var"] == 0.0 or r["nwin"] * 2.0 ** -53 * float(r["means"].max()) ** 2 < 1e-2 * abs(r["ref_var"] - 1e-6), (c.name, ci, r["ref_var"])
            floor_taken += sd < 1e-3
            assert math.isfinite(r["nu"]) and math.isfinite(r["judged"]["p1"]), (c.name, ci)
    assert floor_taken >= 2


def test_no_golden_case_leaves_an_array_and_no_walk_leaves_the_depth():
    """Asserted from the restatement, so that the golden generator never runs the reference into its Array's throw: a golden record has
    a neighbourhood longer than its candidate (isitcnv sizes and indexes the running mean with the difference) and takes no value past
    `capacity`; the other groups are exactly the records that do.  Every index of the depth that any walk reads lies inside it."""
    kinds = set()
    for c in cc.all_cases():
        for ci, r in cc.restated(c).items():
            lo, hi = cc.reads(r)
            assert (lo is None or lo >= 0) and (hi is None or hi < c.depth.size), (c.name, ci)
            assert r["plan"]["top"] >= -1 and r["plan"]["capacity"] >= 1, c.name
            if cc.in_golden(c):
                assert not r["empty"] and not r["past_capacity"], (c.name, ci)
            else:
                assert r["empty"] != r["past_capacity"], (c.name, ci)
                kinds.add((c.group, "empty" if r["empty"] else "past"))
                if r["empty"]:
                    assert r["flags"][0] & 1 and r["flags"][1] & 1 and r["judged"]["status"] == -9 and r["judged"]["geno"] == 0, c.name
    assert kinds == {("empty", "empty"), ("fraction", "past")}


def test_every_case_in_both_kinds_and_in_every_form_its_values_allow():
    names = {c.name for c in cc.all_cases()}
    for c in cc.all_cases():
        stem, tag = c.name.rsplit("_", 1)
        assert tag in ("del", "dup") and f"{stem}_{'dup' if tag == 'del' else 'del'}" in names, c.name
        assert all(int(c.cands[i, 2]) == (cc.DEL if tag == "del" else cc.DUP) for i in c.index), c.name
        fits = int(c.depth.max()) <= 255
        assert cc.forms(c) == ([(1, 1), (1, 0), (1, 3), (1, 2)] if fits and not c.expect.get("int32_only") else []) + [(4, 1), (4, 0)], c.name
        assert c.depth.size <= 300_000 and c.depth.min() >= 0
    wide = [c.name for c in cc.all_cases() if int(c.depth.max()) > 255]
    assert sorted(wide) == sorted([f"body_range_{s}_{t}" for s in (16382, 16383) for t in ("del", "dup")] + ["deep_sums_del", "deep_sums_dup"])


def test_deep_depth_sums_beyond_32_bits():
    for c in both("deep_sums"):
        r = one(c)
        assert r["body_s1"] > 2.0 ** 32 and r["body_s2"] < 2.0 ** 53 and int(r["body_s2"]) == int((c.depth[c.cands[0, 0]:c.cands[0, 1] + 1].astype(object) ** 2).sum()), c.name
        assert r["flags"] == {0: 0, 1: 0} and r["judged"]["status"] == 1 and r["body_nbk"] == 102 and r["ref_var"] == 0.0, c.name
        assert cc.forms(c) == [(4, 1), (4, 0)] and r["nwin"] > 4 * r["nbody"] - 10, c.name


def test_triggers_sit_where_they_were_built():
    seen = set()
    for c in cc.all_cases():
        if c.group != "triggers" or "trigger" not in c.expect:
            continue
        r, t = one(c), c.expect["trigger"]
        for side in ("left", "right"):
            st = r[side]["stretches"]
            assert len(st) == 2 and st[0]["trigger"] == t and st[0]["fill_t"] is None and st[0]["taken"] == t, (c.name, side)
            assert st[1]["trigger"] is None and st[1]["taken"] == c.expect["taken_each"] - t and r[side]["ended"] == "full", (c.name, side)
        assert r["used0"] == r["rcnt"] == c.expect["taken_each"] and r["flags"] == {0: 0, 1: 0}, c.name
        seen.add(t)
    assert seen == {0, 15, 16, 63, 64, 1023, 1024, 4095, 4096, 16383, 16384, 16389, 65535, 65536, 65541}
    # ... which is, in a trip of either storage: a trip's first and last position, a thread's, a wave's, and the second trip
    for sb in (4, 1):
        per, trip = cc.PER[sb], cc.TRIP[sb]
        pos = {t: cc.trip_position(t, sb) for t in seen}
        assert pos[trip - 1][:3] == (0, 1023, per - 1) and pos[trip][:3] == (1, 0, 0) and pos[trip + 5][0] == 1
        assert pos[per - 1][1:3] == (0, per - 1) and pos[per][1:3] == (1, 0)
        assert pos[64 * per - 1][3:] == (63, 0) and pos[64 * per][3:] == (0, 1)
    for c in both("two_triggers"):
        for side in ("left", "right"):
            st = one(c)[side]["stretches"]
            assert [s["trigger"] for s in st] == [100, 49, None] and st[0]["examined"] + st[1]["examined"] < cc.TRIP[4], c.name   # 49: the position next to a neighbour is not examined
    for c in both("first_extreme"):
        for side in ("left", "right"):
            assert [s["trigger"] for s in one(c)[side]["stretches"]] == [102, None], c.name
    for c in both("all_extreme"):
        r = one(c)
        for side in ("left", "right"):
            assert r[side]["jumps"] == 0 and len(r[side]["stretches"]) == 1, c.name
        # the walks went through both neighbours: 30 extremes dropped, the second neighbour's 21 values taken
        assert r["left"]["stretches"][0]["fill_t"] == 900 + 30 - 1 and len(r["plan"]["left_chain"]) == 2 and r["left_reach"] < c.cands[0, 0], c.name


def test_placement_and_rejected_neighbours():
    for c in both("starts_inside"):
        r = one(c)
        assert [s["trigger"] for s in r["left"]["stretches"]] == [0, None] and [s["trigger"] for s in r["right"]["stretches"]] == [0, None], c.name
        ci = c.index[0]
        assert c.cands[ci - 1, 0] <= c.cands[ci, 0] - r["plan"]["margin"] <= c.cands[ci - 1, 1], c.name
    for name in ("adjacent", "overlapping"):
        for c in both(name):
            r = one(c)
            assert [s["trigger"] for s in r["left"]["stretches"]] == [10, 0, None] and [s["trigger"] for s in r["right"]["stretches"]] == [10, 0, None], c.name
    for c in both("overlapping"):
        ci = c.index[0]
        assert c.cands[ci + 2, 0] < c.cands[ci + 1, 1] and c.cands[ci - 1, 0] < c.cands[ci - 2, 1], c.name
    for c in both("reach_the_ends"):
        r = one(c)
        assert c.cands[0, 0] == 0 and c.cands[-1, 1] == c.depth.size - 1, c.name
        assert r["left"]["jumps"] == 1 and r["right"]["jumps"] == 1 and r["left"]["ended"] == "edge" and r["right"]["ended"] == "edge", c.name
        assert r["used0"] < r["plan"]["top"] + 1 and r["left_reach"] == c.cands[0, 1] and r["right_reach"] == c.cands[-1, 0], c.name
    for c in both("rejected"):
        r = one(c)
        st = c.cands[:, 3].tolist()
        assert st == [-9, -9, 0, 0, 0, -9, -9] and (r["left"]["jumps"], r["right"]["jumps"]) == c.expect["jumps"] == (2, 2), c.name
        assert r["plan"]["left_chain"] == [2, 0] and r["plan"]["right_chain"] == [4, 6], c.name      # the middle -9 skipped, the ends never
    for c in both("rejected_only"):
        r = one(c)
        assert c.cands[:, 3].tolist() == [-9, 0, -9] and (r["left"]["jumps"], r["right"]["jumps"]) == (1, 1), c.name


def test_limits_values_on_both_sides():
    kinds = set()
    for c in cc.all_cases():
        if c.group != "limits":
            continue
        kind = int(c.cands[c.index[0], 2])
        lim, is_ext, not_ext = cc.limits(kind, c.RDmedian)
        lt = c.expect["limit_kind"]
        frac = lim - math.floor(lim)
        assert {"int": frac == 0, "half": frac == 0.5, "above": 0 < frac < 1e-9, "below": 1 - 1e-9 < frac < 1}[lt], (c.name, repr(lim))
        near = c.expect["near"]
        ext = cc.extreme(np.array(near), kind, c.RDmedian).tolist()
        assert True in ext and False in ext and abs(is_ext - not_ext) == 1, c.name
        if lt == "int":                      # the value ON the limit is kept: the comparisons are strict
            assert not cc.extreme(np.array([int(lim)]), kind, c.RDmedian)[0] and int(lim) in near, c.name
        r = one(c)
        dropped = sum(ext)
        for side in ("left", "right"):       # the planted values lie inside both walks, so `dropped` of them push the last slot out
            assert r[side]["stretches"][0]["fill_t"] == 300 + dropped - 1, (c.name, side)
        kinds.add((kind, lt))
    assert kinds == {(k, lt) for k in (cc.DEL, cc.DUP) for lt in ("int", "half", "above", "below")}


def test_slots():
    for S in (16384, 16385, 65536, 65537):
        for c in both(f"slots_{S}"):
            r = one(c)
            for side in ("left", "right"):
                st = r[side]["stretches"]
                assert len(st) == 1 and st[0]["fill_t"] == S - 1 and st[0]["taken"] == S == st[0]["room"], c.name
    assert cc.trip_position(16383, 4)[:3] == (0, 1023, 15) and cc.trip_position(16384, 4)[:3] == (1, 0, 0)      # a trip's last position, the next one's first
    assert cc.trip_position(65535, 1)[:3] == (0, 1023, 63) and cc.trip_position(65536, 1)[:3] == (1, 0, 0)
    for c in both("slots_midthread"):
        r = one(c)
        assert r["left"]["stretches"][0]["fill_t"] == r["right"]["stretches"][0]["fill_t"] == 1036, c.name
        assert cc.trip_position(1036, 4)[2] == 12 and cc.trip_position(1036, 1)[2] == 12
    for c in both("room_1"):
        r = one(c)
        assert (r["plan"]["capacity"], r["plan"]["top"], r["used0"], r["rcnt"], r["nbody"], r["nwin"]) == (2, 0, 1, 1, 1, 1), c.name
    for want in (0, 1, 39):
        for c in both(f"left_short_{want}"):
            r = one(c)
            assert r["used0"] == want < r["plan"]["top"] + 1 == 40 and r["left"]["ended"] == "edge" and r["left_reach"] == (2 if want else c.cands[0, 0] - 1), c.name
            assert r["rcnt"] == 80 - want and int(c.cands[c.index[0], 0]) - r["plan"]["margin"] > 2 - (want == 0), c.name
    for c in both("right_short"):
        r = one(c)
        assert r["plan"]["edge_branch"] and r["plan"]["top"] == 71 and r["rcnt"] == 5 and r["right"]["ended"] == "edge" and r["right_reach"] == c.depth.size - 2, c.name
    for c in both("edge_end_is_last"):
        r = one(c)
        assert r["plan"]["edge_branch"] and r["plan"]["top"] == 78 and r["rcnt"] == 0 and c.cands[0, 1] == c.depth.size - 1, c.name
        assert r["right_reach"] == int(c.cands[0, 1]) + r["plan"]["margin"], c.name
    for c in both("edge_top_0"):
        r = one(c)
        assert r["plan"]["edge_branch"] and r["plan"]["top"] == 0 and r["plan"]["capacity"] == 2 and r["empty"], c.name
    for c in both("d_raised"):
        T = one(c)["plan"]
        assert (T["d"], T["capacity"], T["top"], T["body_len"]) == (304, 1520, 759, 10), c.name
    for c in both("fraction_half"):
        r = one(c)
        assert r["plan"]["right_cap"] == 601.0 == r["plan"]["capacity"] and (r["used0"], r["rcnt"]) == (300, 301), c.name
    for c in both("fraction_quarter"):
        r = one(c)
        assert r["plan"]["right_cap"] == 600.5 and r["plan"]["capacity"] == 600 and r["past_capacity"] and (r["used0"], r["rcnt"]) == (300, 300), c.name


def test_seam_chunks_and_windows():
    mods = set()
    for c in cc.all_cases():
        if c.group != "seam" or "used0" not in c.expect:
            continue
        r = one(c)
        assert r["used0"] == c.expect["used0"] and r["nref"] == 400 and r["nbody"] == 16 and not r["thin"], c.name
        assert r["split"]["used0_mod16"] == c.expect["used0"] % 16, c.name
        mods.add(r["used0"])
    assert mods == set(range(17)) | {31, 33}
    for c in both("seam_all_left"):
        r = one(c)
        assert r["rcnt"] == 0 and r["used0"] == r["nref"] > 300, c.name
    assert one(cc.get_case("seam_0_del"))["used0"] == 0
    got = {}
    for c in cc.all_cases():
        if c.group == "chunks":
            r = one(c)
            assert r["nref"] == c.expect["nref"] and r["nbody"] == 64 and r["split"]["chunks"] == c.expect["chunks"], c.name
            got[r["nref"]] = r["split"]["chunks"]
    assert got == {65: 4, 79: 4, 80: 5, 239: 14, 240: 15, 255: 15, 256: 16, 400: 16}          # 4 nref / width on both sides of 5, 15 and 16
    wins = set()
    for c in cc.all_cases():
        if c.group == "windows" and "nwin" in c.expect:
            r = one(c)
            assert r["nwin"] == c.expect["nwin"] and r["nbody"] == 16, c.name
            wins.add(r["nwin"])
            if r["nwin"] >= 16 * 16384:          # all sixteen chunks: one full round of 16 x 1024 windows each, or one more window's worth
                assert r["split"]["chunks"] == 16 and r["split"]["sum_chunk_len"] == (16384 if r["nwin"] == 16 * 16384 else 16388), c.name
    assert wins == {1, 2, 3, 4, 63, 64, 65, 72, 1000, 16384, 16385, 262144, 262145}
    # trailing chunks without a window: 65 and 72 windows in chunks of 8 fill nine of the sixteen; 64 fill all sixteen with chunks of 4
    assert one(cc.get_case("nwin_65_del"))["split"]["sum_chunk_len"] == 8 and one(cc.get_case("nwin_1_del"))["split"]["sum_chunk_len"] == 4
    # how many of the sixteen chunks hold a window: a multiple of the chunk length (64 = 8 x 8, 16 384 = 16 x 1024) and not (65, 16 385, 1, 3)
    held = {}
    for c in cc.all_cases():
        if c.group == "windows" and "nwin" in c.expect and c.name.endswith("_del"):
            sp = one(c)["split"]
            assert sp["sum_chunks_with_windows"] <= sp["chunks"] and sp["hist_chunks_with_windows"] <= 16, c.name
            assert sp["chunks"] < 16 or (sp["sum_chunk_len"], sp["sum_chunks_with_windows"]) == (sp["hist_chunk_len"], sp["hist_chunks_with_windows"]), c.name
            held[c.expect["nwin"]] = (sp["chunks"], sp["sum_chunk_len"], sp["sum_chunks_with_windows"], c.expect["nwin"] % sp["sum_chunk_len"] == 0)
    # (chunks the job takes, their length, chunks that hold a window, nwin a multiple of the length)
    assert held[1] == (4, 4, 1, False) and held[3] == (4, 4, 1, False) and held[4] == (5, 4, 1, True)
    assert held[63] == (16, 4, 16, False) and held[64] == (16, 4, 16, True) and held[65] == (16, 8, 9, False) and held[72] == (16, 8, 9, True)
    assert held[1000] == (16, 64, 16, False) and held[16384] == (16, 1024, 16, True) and held[16385] == (16, 1028, 16, False)
    assert held[262144] == (16, 16384, 16, True) and held[262145] == (16, 16388, 16, False)
    for w in (1, 2, 15, 17, 300):
        for c in both(f"width_{w}"):
            r = one(c)
            assert r["nbody"] == w and (w != 300 or r["nwin"] < w), c.name


def test_thinning():
    for c in both("thin_budget_plus0"):
        r = one(c)
        assert r["nref_raw"] + 200 == 2000 == r["plan"]["budget"] and not r["thin"] and r["nref"] == 1800, c.name
    for c in both("thin_budget_plus1"):
        r = one(c)
        assert r["nref_raw"] + 201 == 2001 == r["plan"]["budget"] + 1 and r["thin"] and (r["nref"], r["nbody"]) == (1799, 200), c.name
    for c in both("thin_seam"):
        r = one(c)
        assert r["thin"] and r["used0"] == 37 and r["nref"] < r["nref_raw"] and r["plan"]["budget"] == 500, c.name
        jr, _ = r["thin_index"]
        assert (jr < 37).sum() > 5 and (jr >= 37).sum() > 300, c.name                      # indexed reads on both sides of the seam
    # the searched index products: exactly an integer k as a fraction, one double step below it as a double, so slot k - 1 is read;
    # and the two slots hold different values, so the record shows which was read
    for (S, mx), (nref, count) in {(75, 10): (90, 2), (92, 10): (92, 4), (78, 13): (117, 1)}.items():
        for c in both(f"thin_below_integer_{S}_{mx}"):
            r = one(c)
            size = r["nref_raw"]
            assert r["thin"] and (size, r["nref"]) == (2 * S, nref), c.name
            jr, _ = r["thin_index"]
            below = [i for i in range(nref) if (i * size) % nref == 0 and jr[i] == i * size // nref - 1]
            assert len(below) == count, (c.name, below)
            for i in below:
                k = i * size // nref
                p = float(i) / float(nref) * float(size)
                assert p < k and k - p <= math.ulp(float(k)) and Fraction(i) / nref * size == k, (c.name, i, repr(p))
            assert any(r["ref_raw"][i * size // nref - 1] != r["ref_raw"][i * size // nref] for i in below), c.name
            assert all(jr[i] == i * size // nref for i in range(nref) if i not in below), c.name      # everywhere else the floor of the fraction


def test_quantiles():
    for blen in (1, 2, 3):
        for c in both(f"body_{blen}"):
            r = one(c)
            assert r["nbody"] == blen and blen // 4 == 0, c.name
            if r["body_nbk"] is not None:        # rank 0 is never "first reached": the lower quartile stays the minimum
                assert r["body_walk"][0][0] is None and r["body_q"][0] == r["body_min"], c.name
            if blen == 1:
                assert r["body_nbk"] is None and r["body_q"] == (r["body_min"],) * 3, c.name
    for c in both("body_constant"):
        r = one(c)
        assert r["body_nbk"] is None and r["body_min"] == r["body_max"] == r["body_q"][1], c.name
    for name, hits in (("exact", (32, 64, 96)), ("short", (31, 63, 95)), ("over", (33, 65, 97))):
        for c in both(f"body_ranks_{name}"):
            at, cum = one(c)["body_walk"]
            assert tuple(int(cum[b]) for b in (0, 1, 3)) == hits, c.name
            assert at == ([0, 1, 3] if name != "short" else [1, 3, 4]), (c.name, at)         # one short of the rank: the next occupied bucket
    for name in ("means_constant", "means_narrow"):
        for c in both(name):
            r = one(c)
            assert r["ref_nbk"] is None and r["ref_q"][0] == float(r["means"].min()) and r["ref_q"][2] == float(r["means"].max()), c.name
            assert (r["means"].max() > r["means"].min()) == (name == "means_narrow"), c.name
    for c in both("means_one_pair"):
        r = one(c)
        assert r["ref_nbk"] == 3 and sorted(set(((r["means"].astype(np.float64) - r["ref_q"][0]) / 0.01 + 0.5).astype(int))) == [0, 2], c.name
    # means on a bucket edge: the double index is the integer itself (distance 0, within one step), the fraction's lies below it -- by less
    # than one step of the quotient --, so the bucket is the division's rounding; and the upper quartile's rank falls into that bucket
    for c in both("means_bucket_edge"):
        r = one(c)
        lo = r["ref_q"][0]
        m64 = r["means"].astype(np.float64)
        assert lo == 30.0 and sorted(set(np.round((m64 - lo) * 128).astype(int))) == list(range(17)) and np.all((m64 - lo) * 128 == np.round((m64 - lo) * 128)), c.name
        for m, bucket in zip(c.expect["bucket_edge"], (13,)):
            w = 30.0 + m / 128.0
            idx = (w - lo) / 0.01 + 0.5
            true = (Fraction(w) - Fraction(lo)) / Fraction(0.01) + Fraction(1, 2)
            assert idx == bucket and bucket - 1 < true < bucket and bucket - true < math.ulp((w - lo) / 0.01), (c.name, m, repr(idx))
            assert int((m64 == w).sum()) >= 2, c.name
        at, cum = r["ref_walk"]
        assert at[2] == 13 and cum[12] < r["nwin"] * 3 // 4 <= cum[13] and int((m64 == 30.125).sum()) == 226, (c.name, at)
    for c in both("judged_rejected"):
        j = one(c)["judged"]
        assert (j["status"], j["geno"]) == (-9, 0), c.name
    for c in both("judged_wrong_type"):
        r = one(c)
        assert (r["judged"]["status"], r["judged"]["geno"]) == (-9, 1) and r["nu"] is None, c.name


def test_decline_flags_on_both_sides():
    for span, flag in ((16382, 0), (16383, 2)):
        for c in both(f"body_range_{span}"):
            r = one(c)
            assert r["body_nbk"] == span + 2 and r["flags"] == {0: flag, 1: flag} and (r["body_nbk"] > cc.HIST_BINS) == bool(flag), c.name
    for h, flag in ((16382, 0), (16383, 4)):
        for c in both(f"means_range_{h}"):
            r = one(c)
            assert r["ref_nbk"] == h + 2 and r["flags"] == {0: flag, 1: flag} and int(c.depth.max()) <= 255, c.name
    # (the split form's right walk, not vouched for where the left chain is cut too, is given all of `capacity`: it uses its chain up where
    # the reference's walk stops before: a decline more, the same answer)
    for name, flag, split_flag in (("fills_first", 0, 8), ("fills_first_left", 0, 0), ("fills_first_right", 0, 0), ("left", 8, 8), ("right", 8, 8), ("both", 8, 8)):
        for c in both(f"chain_{name}"):
            r = one(c)
            assert r["plan"]["cut"] & 3 == c.expect["cut"] and r["flags"] == {0: flag, 1: split_flag}, c.name
            assert bool(r["plan"]["cut"] & 4) == (c.expect["cut"] == 2), c.name
            sides = [s for s, bit in (("left", 1), ("right", 2)) if c.expect["cut"] & bit]
            for s in sides:
                assert len(r["plan"][f"{s}_chain"]) == 48 and (r[s]["jumps"] >= 48) == bool(flag), (c.name, s)
    S = 100
    for name, bit, flag in (("vouched_edge", 4, 0), ("not_vouched", 0, 0), ("vouched_short", 4, 16), ("vouched_just_fills", 4, 0)):
        for c in both(name):
            r = one(c)
            assert r["plan"]["avail"] == 2 * S + 64 - (name == "not_vouched") and r["plan"]["cut"] == bit, c.name
            assert r["flags"] == {0: 0, 1: flag} and (r["used0"] < S) == bool(flag), c.name
    assert one(cc.get_case("vouched_short_del"))["used0"] == S - 1 and one(cc.get_case("vouched_just_fills_del"))["left"]["stretches"][0]["fill_t"] == 263
    for c in both("empty"):
        r = one(c)
        assert r["empty"] and r["nref"] < r["nbody"] and r["flags"] == {0: 1, 1: 1}, c.name
    # every flag a form can raise occurs, and so does a clean record next to it
    seen = {0: set(), 1: set()}
    for c in cc.all_cases():
        for r in cc.restated(c).values():
            for f in (0, 1):
                seen[f].add(r["flags"][f])
    assert seen[0] == {0, 1, 2, 4, 8} and seen[1] == {0, 1, 2, 4, 8, 16}


def test_bin_form_and_lists():
    for nb, blen in ((2000, 1), (2000, 3), (5000, 4), (20000, 60)):
        for c in both(f"bins_{nb}_{blen}"):
            r = one(c)
            assert c.depth.size == nb < c.span_all // 2 and c.span_all == 101 * nb and r["plan"]["d"] == c.expect["d"] == max(blen, 4), c.name
            assert r["left"]["jumps"] + r["right"]["jumps"] >= (2 if blen == 60 else 0) and c.P == cc.DEFAULT_P, c.name
    for c in both("neither_form"):
        assert c.depth.size == c.span_all // 2 and one(c)["plan"]["d"] == 3, c.name
    for c in both("list_301"):
        assert len(c.cands) == len(c.index) == 301 and c.expect["lists"] == (1, 300, 3, 301, 1), c.name
        recs = cc.restated(c)
        assert all(not r["empty"] and r["flags"] == {0: 0, 1: 0} for r in recs.values()), c.name
        assert sum(1 for r in recs.values() if r["left"]["jumps"] or r["right"]["jumps"]) > 250, c.name
    for c in both("list_copied"):
        recs = cc.restated(c)
        chains = sum(len(r["plan"]["left_chain"]) + len(r["plan"]["right_chain"]) for r in recs.values())
        # CandJob 72 bytes, a chain entry 8, CandOut 112: beyond the mailbox slot of 512 KB
        assert 640 * 72 + (chains + 1) * 8 + 640 * 112 > 512 * 1024, c.name
        assert {r["flags"][1] for r in recs.values()} == {0} and {r["plan"]["cut"] & 3 for r in recs.values()} == {1, 2, 3}, c.name


def test_range_cases():
    rc = {name: (d, lo, hi) for name, d, lo, hi in cc.range_cases()}
    d, lo, hi = rc["lengths_and_residues"]
    ln = hi - lo + 1
    assert {(int(a) % 16, int(k)) for a, k in zip(lo[:80], ln[:80])} == {(r, k) for r in range(16) for k in (1, 2, 255, 256, 257)}
    assert 100_000 in ln and lo.min() == 0 and hi.max() == d.size - 1 and d.max() <= 255
    assert len(rc["one_range"][1]) == 1 and len(rc["ranges_3000"][1]) == 3000
    d, lo, hi = rc["beyond_2p31_and_2p32"]
    sums = [int(d[a:b + 1].astype(np.int64).sum()) for a, b in zip(lo, hi)]
    assert sums[0] < 2 ** 31 < sums[1] < 2 ** 32 < sums[2] and d.max() > 255
