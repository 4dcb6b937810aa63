"""CPU: the cases of tests/filter_cases.py are what they claim to be, and the restatement of filterstatus they are judged by equals the
compiled reference's answers (golden/filter_edges.npz) bit for bit.  Nothing here touches the library's device code: the claims are proved
from the reference's loops restated in numpy (level_sums_host / choose_levels of pipeline_steps.h are NOT what the cases are judged by;
they have their own checks in tests/sanitize/host_harness.cpp) and from the library's constants restated next to them."""
import json
import os
import re

import numpy as np
import pytest

import filter_cases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "filter_edges.npz")
F32 = np.float32


@pytest.fixture(scope="module")
def restated():
    return {c.name: fc.filterstatus_numpy(c.T, c.status, c.dev) for c in fc.all_cases()}


@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN)
    names, off, d = json.loads(str(z["names"])), z["off"], z["cleared_diff"]
    return {n: np.cumsum(d[off[i]:off[i + 1]]) for i, n in enumerate(names)}


def kept_offsets(f, run):
    s, e = run
    return [int(k) for k in np.nonzero(f.status[s:e + 1])[0]]


def test_the_constants_are_the_librarys():
    """Stated here so that a change shows: the cases are placed by them."""
    assert (fc.THREADS, fc.RUNS_INLINE, fc.EAGER_BOUNDS, fc.FS_LIST_CAP, fc.MAX_L, fc.HARD_MAX_L) == (256, 200, 1024, 1 << 20, 10400, 1 << 22)
    src = os.path.join(ROOT, "rsicnv_amd", "csrc")
    kh = open(os.path.join(src, "kernels.h")).read()
    assert re.search(r"constexpr int kRunsInline = 200,", kh) and re.search(r"constexpr int kMaxScanL = 10400;", kh)
    ph = open(os.path.join(src, "pipeline.hip")).read()
    assert "constexpr uint32_t kEagerBounds = 1024;" in ph and "constexpr int32_t kFsListCap = 1 << 20;" in ph
    pi = open(os.path.join(src, "pipeline_internal.h")).read()
    assert "constexpr int kMaxL = kMaxScanL;" in pi and "constexpr int kHardMaxL = 1 << 22;" in pi
    kb = open(os.path.join(src, "kernels_bin.hip")).read()
    assert "done += kThreads;" in kb and "constexpr int kThreads = 256;" in kb
    assert "M > clist_cap" in open(os.path.join(src, "kernels_fs.hip")).read()         # 2^20 marked bins are still the device's


def test_every_case_is_well_formed(restated):
    for c in fc.all_cases():
        assert c.T.dtype == np.float32 and c.status.dtype == np.int32 and c.T.shape == c.status.shape, c.name
        assert -c.Lmax <= c.status.min() and c.status.max() <= c.Lmax and 1 <= c.Lmax <= fc.HARD_MAX_L, c.name
        assert c.claim and c.group in ("walks", "ties", "neighbours", "lists", "levels", "routes"), c.name
        unmarked = c.T[c.status == 0]
        assert (unmarked == fc.FILL).all(), c.name
        f = restated[c.name]
        if unmarked.size:
            # the float sum of k bins of 32.0 is 32 k exactly while k <= 2^24: the mean is 32.0 in closed form, and the restatement finds it
            assert unmarked.size <= 1 << 24 and f.has_level0 and f.m0 == F32(32.0), c.name
            assert F32(32.0 * unmarked.size) == 32.0 * unmarked.size
        if c.T.size <= 70000:
            assert fc.continuous_segments(c.status) == fc.continuous_segments_loop(c.status), c.name
        assert (f.status[f.status != c.status] == 0).all(), c.name                       # filterstatus only ever clears bins
    assert len(fc.all_cases()) == 43 and len(fc.golden_cases()) == 42


def test_restatement_equals_the_reference(restated, golden):
    assert set(golden) == {c.name for c in fc.golden_cases()}
    for c in fc.golden_cases():
        want = c.status.copy()
        want[golden[c.name]] = 0
        assert np.array_equal(restated[c.name].status, want), c.name


def test_the_last_run_is_never_trimmed_and_the_run_before_it_is(restated):
    """Every case that ends in the tail run [soft, solid, solid, soft]: both soft bins would go, were the run not the one the reference drops."""
    seen = 0
    for c in fc.all_cases():
        f = restated[c.name]
        if not f.trim or not c.expect["where"] or c.group == "levels" and c.name == "not_filtered":
            continue
        s, e = c.expect["where"][-1]
        if e - s != 3 or not np.array_equal(c.T[s:e + 1], np.array([30, 10, 10, 30], dtype=F32)):
            continue
        seen += 1
        assert np.array_equal(f.status[s:e + 1], c.status[s:e + 1]) and (c.status[s:e + 1] < 0).all(), c.name
        assert (s, e) not in f.runs and (not f.runs or f.runs[-1][1] < s), c.name
    assert seen >= 38
    c = fc.get_case("last_run_on_last_bin")
    f = restated[c.name]
    assert c.expect["where"][-1][1] == c.T.size - 1 and c.status[-1] < 0 and f.status[-1] == c.status[-1]
    assert kept_offsets(f, c.expect["where"][0]) == [2]                                  # ... and the run before it was trimmed
    c = fc.get_case("last_run_against_the_one_before")
    (s0, e0), (s1, e1) = c.expect["where"]
    assert s1 == e0 + 1 and c.status[e0] > 0 > c.status[s1]
    c = fc.get_case("one_run_only")
    assert restated[c.name].runs == [] and np.array_equal(restated[c.name].status, c.status) and np.count_nonzero(c.status) == 4
    c = fc.get_case("no_marked_bin")
    assert restated[c.name].runs == [] and not c.status.any()


def test_walks_stop_where_they_were_built_to(restated):
    lengths, left, right = [], set(), set()
    for c in fc.all_cases():
        if c.group != "walks":
            continue
        f = restated[c.name]
        runs = c.expect["where"][:-1]
        n = runs[0][1] - runs[0][0] + 1
        lengths.append(n)
        assert len(runs) == len(c.expect["patterns"]) and f.runs == runs, c.name             # the reference's runs are the ones laid out
        signs = set()
        for (s, e), (pat, kept) in zip(runs, c.expect["patterns"]):
            assert e - s + 1 == n
            got = kept_offsets(f, (s, e))
            signs.add((pat.split("_")[0], int(np.sign(c.status[s]))))
            if pat == "all_soft":
                assert got == [], (c.name, pat)                                               # left walk: all but the last; right walk: the last
            elif pat == "last_solid":
                assert got == [n - 1], (c.name, pat)                                          # left walk: all but the last, which stays
            elif pat.startswith("one_"):
                k, = kept
                assert got == [k], (c.name, pat)                                              # the walks meet: L alone stays
                left.add((n, k))
                right.add((n, n - 1 - k))
            else:
                a, b = kept
                assert got == list(range(a, b + 1)) and b - a >= 2, (c.name, pat)             # soft bins between two solid ones stay
                assert (c.T[s + a + 1:s + b] == (fc.DEL_SOFT if c.status[s] < 0 else fc.DUP_SOFT)).all()
        gaps = {runs[i + 1][0] - runs[i][1] - 1 for i in range(len(runs) - 1)}
        assert gaps <= {0, 1, 2} and (n < 2 or gaps == {0, 1, 2}), c.name
        assert {sg for _, sg in signs} == {-1, 1}, c.name
    assert tuple(lengths) == fc.WALK_LENGTHS == (1, 2, 3, 255, 256, 257, 258, 511, 512, 513, 1025, 5000)
    # the first kept bin at each of these offsets from the left end and from the right end, on both sides of a step of 256 positions
    for k in (0, 1, 254, 255, 256, 257):
        assert any(kk == k for _, kk in left) and any(kk == k for _, kk in right), k
    assert {(513, k) for k in (0, 1, 254, 255, 256, 257, 511, 512)} <= left and {(513, k) for k in (0, 1, 255, 256, 257, 258, 511, 512)} <= right
    assert all((n, n - 1) in left and (n, 0) in left for n in fc.WALK_LENGTHS) and all((n, n - 2) in left for n in fc.WALK_LENGTHS if n >= 2)


def test_ties_and_the_double_threshold(restated):
    for name, edge, soft in (("tie_del_28", 28.0, np.nextafter(F32(28.0), F32(99))), ("tie_dup_36", 36.0, np.nextafter(F32(36.0), F32(0)))):
        c = fc.get_case(name)
        f = restated[name]
        (s, e), (s2, e2) = c.expect["where"][:2]
        assert [kept_offsets(f, r) for r in c.expect["where"][:2]] == c.expect["kept"] == [[2, 3, 4, 5], []]
        assert c.T[s + 2] == c.T[s + 5] == F32(edge) and c.T[s + 3] == soft and (c.T[s2:e2 + 1] == soft).all()
        assert float(f.m0) - c.dev == 28.0 and float(f.m0) + c.dev == 36.0
    for name, v, dev, sign in (("double_threshold_dup", F32(32.1), 0.1, 1), ("double_threshold_del", F32(31.7), 0.3, -1)):
        c = fc.get_case(name)
        f = restated[name]
        s, e = c.expect["where"][0]
        assert c.dev == dev and c.T[s] == v and kept_offsets(f, (s, e)) == [2]
        thr = 32.0 + sign * dev                                                                # (double)m0 + dev, as the kernel is given it
        in_double = float(v) < thr if sign > 0 else float(v) > thr
        in_float = v < F32(thr) if sign > 0 else v > F32(thr)
        assert in_double and not in_float, name                                               # a comparison done in float keeps the bin


def test_neighbours_levels_and_a_nan(restated):
    for c in fc.all_cases():
        if c.group != "neighbours":
            continue
        f = restated[c.name]
        parts = c.expect["where"][:-1]
        assert f.runs == parts, c.name
        assert [kept_offsets(f, r) for r in parts] == c.expect["kept"], c.name
        assert f.trim
    for name in ("adjacent_del_dup", "adjacent_dup_del"):
        (s0, e0), (s1, e1) = fc.get_case(name).expect["where"][:2]
        assert s1 == e0 + 1
    st = fc.get_case("adjacent_del_dup").status
    assert st[fc.get_case("adjacent_del_dup").expect["where"][0][0]] < 0 < fc.get_case("adjacent_dup_del").status[fc.get_case("adjacent_dup_del").expect["where"][0][0]]
    c = fc.get_case("single_bin_runs")
    assert all(s == e for s, e in c.expect["where"][:-1]) and all(b[0] == a[0] + 1 for a, b in zip(c.expect["where"][:5], c.expect["where"][1:6]))
    assert fc.get_case("run_from_bin_0").status[0] < 0 and fc.get_case("all_soft_from_bin_0").status[0] > 0
    c = fc.get_case("levels_3_and_7")
    s, e = c.expect["where"][0]
    assert set(c.status[s:e + 1]) == {-3, -7}
    c = fc.get_case("nan_stops_a_walk")
    s, e = c.expect["where"][0]
    assert np.isnan(c.T[s + 100]) and np.count_nonzero(np.isnan(c.T)) == 1
    assert fc.expected_info(c, restated[c.name])[3] == fc.ROUTE_DECLINED


def test_run_lists_on_both_sides_of_every_boundary(restated):
    info = {c.name: fc.expected_info(c, restated[c.name]) for c in fc.all_cases()}
    got = {k: info[f"runs_{k}"][:3] for k in (1, 2, 200, 201, 511, 512, 513, 3000)}
    # 200 runs are the last that ride in the kernel arguments; 511 runs and the dropped one are 1024 boundary entries, the last that
    # come back in the mailbox
    assert got == {1: [1, 1, 0], 2: [2, 1, 0], 200: [200, 1, 0], 201: [201, 0, 0], 511: [511, 0, 0], 512: [512, 0, 1], 513: [513, 0, 1],
                   3000: [3000, 0, 1]}
    for k in got:
        c = fc.get_case(f"runs_{k}")
        assert len(fc.continuous_segments(c.status)) == k == c.expect["runs"]
        assert not np.array_equal(restated[c.name].status, c.status)
    assert info["no_marked_bin"][:3] == [0, 1, 0] and info["one_run_only"][:3] == [0, 1, 0]


def test_level_choice(restated):
    c = fc.get_case("level_gap")
    f = restated[c.name]
    assert sorted(set(c.status)) == c.expect["levels"] == [-5, -3, 0, 2]
    lo, hi, cnt, mean = fc.level_means(c.T, c.status)
    assert mean[0] == F32(30.0) and not mean[0] < 28.0 and cnt[1] == 0 and mean[1] == 0.0           # level -5 is not below, the absent -4 is
    assert (f.leveldel, f.leveladd, f.trim) == (-4, 2, True)
    assert [kept_offsets(f, r) for r in c.expect["where"][:2]] == c.expect["kept"]
    c = fc.get_case("not_filtered")
    f = restated[c.name]
    assert f.has_level0 and not f.trim and f.leveldel == 1 and np.array_equal(f.status, c.status)
    assert ((c.T < 36) & (c.status > 0)).any()                                                # there was something to trim
    c = fc.get_case("no_unmarked_bin")
    f = restated[c.name]
    assert not f.has_level0 and (c.status == -1).all() and np.array_equal(f.status, c.status)
    assert fc.expected_info(c, f) == [-1, -1, -1, 0, 0, 0, 0, 0, 0]


def test_routes(restated):
    info = {c.name: fc.expected_info(c, restated[c.name]) for c in fc.all_cases()}
    assert info["negative_bin"][3] == fc.ROUTE_DECLINED and (fc.get_case("negative_bin").T < 0).sum() == 1
    assert np.count_nonzero(fc.get_case("marked_at_cap").status) == fc.FS_LIST_CAP and info["marked_at_cap"][3] == fc.ROUTE_DEVICE
    assert np.count_nonzero(fc.get_case("marked_beyond_cap").status) == fc.FS_LIST_CAP + 1 and info["marked_beyond_cap"][3] == fc.ROUTE_DECLINED
    assert info[f"lmax_{fc.MAX_L}"][3] == fc.ROUTE_DEVICE and info[f"lmax_{fc.MAX_L + 1}"][3] == fc.ROUTE_LONG
    for L in (fc.MAX_L, fc.MAX_L + 1):
        c = fc.get_case(f"lmax_{L}")
        assert c.Lmax == L and c.status.min() == -L and c.status.max() == L
    for c in fc.all_cases():
        if c.group == "routes":
            f = restated[c.name]
            assert f.trim and np.count_nonzero(f.status != c.status) >= 10, c.name             # the result is checked behind every route
            if "kept" in c.expect:
                assert [kept_offsets(f, r) for r in c.expect["where"][:-1]] == c.expect["kept"], c.name
    assert {i[3] for i in info.values()} == {0, 1, 2}
    c = fc.get_case("marked_beyond_cap")
    depths = [kept_offsets(restated[c.name], r)[0] for r in c.expect["where"][:8]]
    assert depths == [0, 1, 255, 256, 257, 5000, 70000, 131070]
