"""CPU: every case of tests/scan_cases.py sits where it was built to sit, proved from the reference's arithmetic restated there, and
the restatement of rsistatus (tests/scan_restatement.py) gives the reference's status (golden/scan_edges.npz) on every one."""
import json
import math
import os

import numpy as np
import pytest

import scan_cases as sc
from scan_restatement import rsistatus_numpy

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scan_edges.npz")
GROUPS = ("ties", "tiles", "median", "trim", "marks", "stop", "routes", "exact_b")


def load_golden():
    z = np.load(GOLDEN)
    names, off, st = json.loads(str(z["names"])), z["off"], z["status"]
    return {n: st[off[k]:off[k + 1]] for k, n in enumerate(names)}


@pytest.fixture(scope="module")
def golden():
    return load_golden()


@pytest.fixture(scope="module")
def median(oracle_cls):
    return oracle_cls().exact_median


_ANALYSIS = {}


def analysis(name, median):
    """first_marks and resolve of a case, once."""
    if name not in _ANALYSIS:
        c = sc.get_case(name)
        fd, fu, stat = sc.first_marks(c, median)
        _ANALYSIS[name] = (fd, fu, stat) + sc.resolve(fd, fu, c.Lmax)
    return _ANALYSIS[name]


def test_the_golden_file_has_every_reference_case(golden):
    assert sorted(golden) == sorted(c.name for c in sc.all_cases() if c.ref)
    assert os.path.getsize(GOLDEN) <= 379 * 1024        # no larger than the largest golden file of this kind (bam_edges.npz)
    for c in sc.all_cases():
        if c.ref:
            assert golden[c.name].size == c.T.size


@pytest.mark.parametrize("group", GROUPS)
def test_restatement_equals_the_reference(group, golden, median):
    for name in sc.case_names(group):
        c = sc.get_case(name)
        st, esc = rsistatus_numpy(c.T, c.medint, c.RDmedian, c.tmedian, c.tlamda, c.Lmax, median, bounded=True)
        assert esc == 0, f"{name}: {esc} walks leave the array"      # what kept the reference inside the array
        assert np.array_equal(st, golden[name]), f"{name}: {np.count_nonzero(st != golden[name])} bins differ"
        if group in ("median", "trim", "stop") and c.T.size <= 4000:      # the default mode is the same function where no walk leaves
            assert np.array_equal(rsistatus_numpy(c.T, c.medint, c.RDmedian, c.tmedian, c.tlamda, c.Lmax, median), st), name


@pytest.mark.parametrize("group", ("ties", "tiles", "median", "trim", "stop"))
def test_first_marks_then_stop_equals_the_sequential_sweeps(group, golden, median):
    """The form the kernels compute in -- first lengths without the stop rule, then the stop levels from the per-L counts and DEL before
    DUP -- gives the reference's status: the second derivation every claim below is read from."""
    for name in sc.case_names(group):
        st = analysis(name, median)[3]
        assert np.array_equal(st, golden[name]), name


def test_ties_sit_on_the_threshold(golden):
    seen = set()
    for name in sc.case_names("ties"):
        c = sc.get_case(name)
        L, sweep, exp = c.expect["L"], c.expect["sweep"], golden[name]
        want = np.zeros(c.T.size, dtype=np.int32)
        steps = []
        for s, hit in zip(c.expect["starts"], c.expect["hit"]):
            score = sc.ref_score(c.T[s:s + L], c.tmedian)
            assert (score <= -c.tlamda if sweep == 0 else score >= c.tlamda) == hit, (name, s, score)
            if hit:
                want[s:s + L] = -L if sweep == 0 else L
            steps.append(float(c.T[s]))
        # the three windows differ in one bin by one float step each
        a, b, cc = (np.float32(x) for x in steps)
        away = np.float32(np.inf if sweep == 0 else -np.inf)
        assert np.nextafter(a, away) == b and np.nextafter(a, -away) == cc
        for s in c.expect["starts"][1:]:
            assert np.array_equal(c.T[s + 1:s + L], c.T[c.expect["starts"][0] + 1:c.expect["starts"][0] + L])
        assert np.array_equal(exp, want), name          # the reference marks the two hitting windows and nothing else
        assert (c.Lmax <= sc.THR_INLINE_L) == (L != 224)
        seen.add((L, sweep, c.tmedian))
    assert len(seen) == 2 * 2 * len(sc.TIE_LENGTHS)
    # the example worked by hand: 35, 35, 35, 35 + 2^-17 hits through the float mean's tie to even, 2^-18 more does not
    w = np.full(4, 35.0)
    w[3] += 2.0 ** -17
    assert sc.ref_score(w, 40.0) <= -10.0
    w[3] += 2.0 ** -18
    assert sc.ref_score(w, 40.0) > -10.0


def test_tiles_and_ends_reach_what_they_name(median, golden):
    for name in sc.case_names("tiles"):
        c = sc.get_case(name)
        fd, fu, stat = analysis(name, median)[:3]
        assert stat["escapes"] == 0
        if name.startswith("tile_"):
            long_form = "_long_" in name
            if long_form:
                assert stat["full_lanes"] >= 2 * 30, (name, stat["full_lanes"])     # lanes that hit at every length, in both sweeps
            else:
                assert c.expect["event_len"] < c.Lmax
                # through the halo, in both directions, on both edges and in both sweeps: a hit centred in one tile marks only bins of
                # the next (the event starts on the tile's first bin) or of the previous one (it ends on the tile's last bin)
                edge, family = c.expect["edge"], c.expect["family"]
                if edge == 256:
                    assert stat["cross_fwd"][1 - family] > 0, (name, stat["cross_fwd"])      # family 1: the DEL from 256; 0: the DUP from 1024
                if edge == 255:
                    assert stat["cross_back"][family] > 0, (name, stat["cross_back"])        # family 0: the DEL up to 255; 1: the DUP up to 1023
            assert (golden[name][c.T.size - 60:c.T.size - 45] < 0).all()              # the last, partial tile
        if name.startswith("ends_"):
            k = int(name[-1])
            exp = golden[name]
            # no window contains bin 0 or bin nb - 1 (rsi.cpp:1204), and a walk only moves inwards: they are never marked
            first, last = max(k, 1), min(c.T.size - 1 - k, c.T.size - 2)
            assert (exp[:first] == 0).all() and exp[first] < 0 and exp[last] > 0 and (exp[last + 1:] == 0).all(), name
    # every placement the issue names, but the one that cannot exist (264 bins ending on bin 255 ... 257)
    placed = {(c.Lmax, "_long_" in c.name, c.expect["edge"], c.expect["family"]) for c in map(sc.get_case, sc.case_names("tiles")) if c.name.startswith("tile_")}
    for Lmax in (20, 99, 224):
        for long_form in (False, True):
            assert {e for L, lf, e, f in placed if L == Lmax and lf == long_form} == {255, 256, 257}
            if Lmax < 224:
                assert {(e, f) for L, lf, e, f in placed if L == Lmax and lf == long_form} == {(e, f) for e in (255, 256, 257) for f in (0, 1)}
    assert not any(L == 224 and lf and f == 0 for L, lf, e, f in placed) and 255 - (224 + 40) + 1 < 0
    assert all(sc.get_case(n).T.size == 3300 for n in sc.case_names("tiles") if n.startswith("tile_"))   # an interior detection workgroup: 1024 ... 2047
    assert {sc.get_case(n).T.size for n in sc.case_names("tiles") if n.startswith("small_")} == {1, 2, 3, 4, 255, 256, 257, 1024, 1025}
    assert {sc.get_case(n).Lmax for n in sc.case_names("tiles") if sc.get_case(n).Lmax == sc.get_case(n).T.size} == {1, 2, 3, 4, 255, 257}


def test_median_cases_sit_on_the_limits(median, golden):
    for rd in (40.0, 41.0, 30.5):
        c = sc.get_case(f"median_limits_rd{rd}")
        ld, lu = rd * 0.75, rd * 1.25
        assert c.expect["medians"] == [math.floor(ld), math.floor(ld) + 1, math.ceil(ld) - 1, math.ceil(ld),
                                       math.floor(lu), math.floor(lu) + 1, math.ceil(lu) - 1, math.ceil(lu)]
        assert (ld == int(ld)) == (rd == 40.0)
        exp = golden[c.name]
        for k, v in enumerate(c.expect["medians"]):
            a = 60 + 110 * k
            marked = bool((exp[a:a + 12] != 0).any())
            assert marked == (v <= ld if k < 4 else v >= lu), (c.name, v)
    c = sc.get_case("median_pairs")
    exp = golden[c.name]
    for sweep, a, L, mid in c.expect["spots"]:
        lim = 30.0 if sweep == 0 else 50.0
        w = c.medint[a:a + L]
        assert np.count_nonzero(w <= lim if sweep == 0 else w >= lim) == L // 2 and median(w) == mid
    assert {round(m - (30.0 if s == 0 else 50.0), 1) for s, _, _, m in c.expect["spots"]} == {-0.5, 0.0, 0.5}
    assert analysis(c.name, median)[2]["straddles"] >= c.expect["min_straddles"]
    c = sc.get_case("median_mid_lane")
    i, pairs = c.expect["lane"], {}
    for L, want in c.expect["beyond"].items():
        w = c.medint[i - L // 2:i - L // 2 + L]
        assert np.count_nonzero(w <= 30) == want
        if want == L // 2:
            pairs[L] = (int(w[w <= 30].max()), int(w[w > 30].min()))
    assert sorted(pairs) == [4, 10, 12] and len(set(pairs.values())) == 3       # straddles at 4, 10 and 12, each with another pair
    hits = sc.score_hits(c.T, c.tmedian, c.tlamda, c.Lmax)[0]
    assert all((L, i) in hits for L in (4, 6, 8, 10, 12))                          # and the lane is a score hit at each
    for rd in (40.0, 41.0, 30.5):
        c = sc.get_case(f"median_random_rd{rd}")
        assert analysis(c.name, median)[2]["straddles"] >= 100, c.name


def test_trim_cases_walk_where_they_say(median, golden):
    for name in sc.case_names("trim"):
        c = sc.get_case(name)
        stat = analysis(name, median)[2]
        assert stat["escapes"] == 0
        if name.startswith("trim_outside"):
            assert stat["outside"] >= c.expect["min_outside"] and stat["empty"] >= c.expect["min_empty"], (name, stat)
        else:
            # from the arrays: each kind of bin -- only the value predicate, only the median predicate, the value exactly tmedian -- is
            # the first bin of some event, the last bin of some event, and lies inside one
            at = {"first": set(), "last": set(), "inside": set()}
            for sweep, a, ln in c.expect["events"]:
                lim = 30.0 if sweep == 0 else 50.0
                T, m = c.T[a:a + ln].astype(np.float64), c.medint[a:a + ln]
                vstop = ~(T > c.tmedian) if sweep == 0 else ~(T < c.tmedian)
                mstop = ~(m > lim) if sweep == 0 else ~(m < lim)
                kind = np.where(T == c.tmedian, 3, np.where(vstop & ~mstop, 1, np.where(~vstop & mstop, 2, 0)))
                assert (kind[T == c.tmedian] == 3).all() and mstop[T == c.tmedian].all()
                at["first"].add(int(kind[0])); at["last"].add(int(kind[-1])); at["inside"] |= set(int(k) for k in kind[3:-3])
                # and windows that passed the median test start on the event's first bin and end on its last: the walks of those hits
                # begin on these very bins, at the end of the window that a run of hits gains
                assert a in stat["win_starts"] and a + ln - 1 in stat["win_ends"], (name, a)
            assert all(v >= {1, 2, 3} for v in at.values()), (name, at)
            # the reference's two walks in sequence both move: the value walk alone, the median walk alone, and both at one end of one hit
            assert stat["value_moved"] > 100 and stat["median_moved"] > 100 and stat["both_moved"] > 20, (name, stat["both_moved"])
            assert (golden[name] != 0).any()
    dists = sorted(int(n.split("_d")[1]) for n in sc.case_names("trim") if n.startswith("trim_outside"))
    halo = 20 // 2 + 1
    assert any(0 < d < halo for d in dists) and any(d > halo + sc.TILE for d in dists)     # inside the halo, and beyond an interior tile's


def test_mark_cases_cover_lengths_and_levels(median):
    for off in (0, 21, 43):
        c = sc.get_case(f"marks_lengths_o{off}")
        _, _, stat = sc.first_marks(c, median)
        assert stat["lengths"] >= set(range(1, 2 * 64 + 4)), sorted(set(range(1, 132)) - stat["lengths"])
        assert len(stat["aligns"]) == 64 and sc.kcap_for(c.Lmax) == 6
    # the derived cap of the mark levels per Lmax: a change of the LDS layout shows here
    assert sc.KCAP_LMAX == {1: 0, 3: 1, 7: 2, 15: 3, 31: 4, 63: 5, 64: 6, 1563: 6, 1564: 5, 1752: 4, 1980: 3, 2270: 2, 2644: 1, 3148: 0}
    for Lmax, k in sc.KCAP_LMAX.items():
        assert sc.kcap_for(Lmax) == k and Lmax <= sc.SCAN_LDS_L
        if Lmax > 64:
            assert sc.kcap_for(Lmax - 1) == k + 1 or Lmax == 1563
    assert {sc.kcap_for(L) for L in sc.KCAP_LMAX} == set(range(7))
    assert sc.kcap_for(3800) == 0 and sc.kcap_for(3801) == 6
    fd, fu, stat = sc.first_marks(sc.get_case("marks_nested"), median)[:3]
    assert len(set(fd[200:330])) >= 4 and fd[300] == 1 and fd[252] == 1 and fd[210] >= 25      # the smallest length wins bin by bin


def test_stop_cases_sit_on_the_fifth(median):
    for sweep in (0, 1):
        for Lmax in (2, 20):
            c = sc.get_case(f"fifth_{'dup' if sweep else 'del'}_L{Lmax}")
            st, ldel, ldup, both, marked = analysis(c.name, median)[3:]
            nb = c.T.size
            assert nb % 5 == 0 and marked[sweep] == {1: nb // 5, 2: nb // 5 + 1} == c.expect["marked"]     # exactly a fifth, then ONE bin more
            assert (ldel, ldup)[sweep] == 2
            assert st[20] == (2 if sweep else -2) and st[21] == 0 and (st[50:58] == 0).all()      # what only L >= 5 sees stays unmarked
            if sweep:
                assert np.count_nonzero(st < 0) == 150 and ldel == Lmax                       # the deletion's bins do not count; DEL never stops
    for nb in (4000, 40_000):
        c = sc.get_case(f"both_alternating_nb{nb}")
        st, ldel, ldup, both, marked = analysis(c.name, median)[3:]
        assert (ldel, ldup) == c.expect["stops"] and both >= c.expect["both_min"]
        assert (both > sc.BOTH_CAP) == (nb == 40_000)
        assert np.array_equal(st[1:-1], np.where(np.arange(nb) % 2 == 0, -1, 1)[1:-1]) and st[0] == 0 and st[-1] == 0   # no window is centred on the end bins
    c = sc.get_case("both_del_wins")
    st, ldel, ldup, both, marked = analysis(c.name, median)[3:]
    assert (ldel, ldup) == c.expect["stops"] and both >= 50 and all(st[100 + 35 * j + 1] == -3 for j in range(50))


def test_route_cases_straddle_the_switches(golden):
    L = [sc.get_case(n).Lmax for n in sc.case_names("routes")]
    assert L == [223, 224, 3800, 3801, 10_400, 10_401, 13_127, 13_128]
    assert sc.THR_INLINE_L == 223 and sc.SCAN_LDS_L == 3800 and sc.MAX_L == 10_400
    assert sc.detect_runs(13_127) and not sc.detect_runs(13_128)
    for n in sc.case_names("routes") + [n for n in sc.case_names("marks") if n.startswith("kcap")]:
        c = sc.get_case(n)
        exp, s, tl = golden[n], c.expect["tie_start"], c.expect["tie_L"]
        assert c.Lmax <= c.T.size <= c.Lmax + 600
        if tl <= c.Lmax and c.Lmax >= 9:
            assert (exp[s:s + tl] == -tl).all() and exp[s - 1] == 0 and exp[s + tl] == 0, n      # the tie window is marked by its own length
            assert (exp < 0).sum() > tl and (exp > 0).any()


def test_exactness_cases(median):
    for n in sc.case_names("exact_a"):
        c = sc.get_case(n)
        for detect in (True, False):
            assert sc.inexact_expected(c.T, c.Lmax, detect) == c.expect["inexact"], (n, detect)
    # the counter is non-zero somewhere: a kernel that stopped counting fails
    assert sum(sc.get_case(n).expect["inexact"] for n in sc.case_names("exact_a")) >= 80
    # every other case reports none
    for c in sc.all_cases():
        if c.group not in ("exact_a", "exact_b"):
            assert sc.inexact_expected(c.T, c.Lmax, True) == 0 and sc.inexact_expected(c.T, c.Lmax, False) == 0, c.name
    names = sc.case_names("exact_b")
    assert len(names) == 3 * sc.EXACT_B_PICKS
    for n in names:
        c = sc.get_case(n)
        (L, pos), mref, mex = c.expect["window"], c.expect["mref"], c.expect["mex"]
        # the reference's own float mean of that window, by its own sliding sum from the chromosome's start
        y = c.T.astype(np.float64)
        s = 0.0
        for v in y[:L]:
            s += v
        for first in range(1, pos - L // 2 + 1):
            s = s - y[first - 1] + y[first + L - 1]
        assert float(np.float32(s / L)) == mref
        assert float(np.float32(math.fsum(y[pos - L // 2:pos - L // 2 + L]) / L)) == mex and mex != mref
        root = math.sqrt(float(L))
        hit_ref, hit_exact = (mref - c.tmedian) * root <= -c.tlamda, (mex - c.tmedian) * root <= -c.tlamda
        assert hit_ref != hit_exact, n                                            # the two decisions differ
        assert -((min(mref, mex) - c.tmedian) * root) == c.tlamda                 # and the one that hits, hits by equality
        # the sufficient test flags these bins, with or without the detection pass; the former range test saw nothing
        assert sc.inexact_expected(c.T, c.Lmax, True) > 0 and sc.inexact_expected(c.T, c.Lmax, False) > 0
        a = np.abs(c.T)
        assert ((a == 0) | ((a >= 2.0 ** -10) & (a < 2.0 ** 20))).all()


def test_escape_cases_against_the_bounded_mode(median):
    for n in sc.case_names("escapes"):
        c = sc.get_case(n)
        st, esc = rsistatus_numpy(c.T, c.medint, c.RDmedian, c.tmedian, c.tlamda, c.Lmax, median, bounded=True)
        fd, fu, stat, st2 = analysis(n, median)[:4]
        assert esc >= c.expect["min_escapes"] and np.array_equal(st, st2) and (st[300:310] < 0).all()
        # no stop rule ends a sweep here, so the sweeps with and without it count the same walks
        assert esc == stat["escapes"]
        assert not c.ref
    # the default mode is unchanged: the forward walk raises where the bounded one counts
    c = sc.get_case("escape_end")
    with pytest.raises(IndexError):
        rsistatus_numpy(c.T, c.medint, c.RDmedian, c.tmedian, c.tlamda, c.Lmax, median)
