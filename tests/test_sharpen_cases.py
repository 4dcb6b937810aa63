"""CPU: the cases of tests/sharpen_cases.py are what they claim to be, and the restatement of optimize_with_derivative they are judged
by equals the compiled reference's answers (golden/sharpen_edges.npz) coordinate for coordinate, after one call and after two.  Nothing
here touches the library's device code.  (oracle/rsi_oracle.cpp exposes no refinement of its own to compare with.)"""
import json
import os
import re

import numpy as np
import pytest

import sharpen_cases as sh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "sharpen_edges.npz")


@pytest.fixture(scope="module")
def restated():
    """name -> (after one call, after two, reports per job: [first call, second call])."""
    out = {}
    for c in sh.all_cases():
        once, _ = sh.refine_jobs(c, 1)
        twice, reps = sh.refine_jobs(c, 2)
        out[c.name] = (once, twice, reps)
    return out


@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN)
    names, off = json.loads(str(z["names"])), z["off"]
    return {n: (z["once"][off[i]:off[i + 1]], z["twice"][off[i]:off[i + 1]]) for i, n in enumerate(names)}


def test_the_constants_are_the_librarys():
    assert (sh.CHUNKS, sh.TILE, sh.WS_MIN_JOBS) == (16, 256, 256)
    kc = open(os.path.join(ROOT, "rsicnv_amd", "csrc", "kernels_cand.hip")).read()
    assert "constexpr int kEdgeChunks = 16;" in kc and "const int reach = len / 4 > 250 ? len / 4 : 250;" in kc
    assert "for (int t0 = i0; t0 < i1; t0 += kThreads)" in kc
    assert re.search(r"constexpr int kThreads = 256;", open(os.path.join(ROOT, "rsicnv_amd", "csrc", "kernels.h")).read() + kc +
                     open(os.path.join(ROOT, "rsicnv_amd", "csrc", "device_util.h")).read())
    assert "const int cap = std::max(256, 2 * nj);" in open(os.path.join(ROOT, "rsicnv_amd", "csrc", "pipeline.hip")).read()
    assert [sh.reach_of(x) for x in (1, 999, 1000, 1003, 1004, 8192, 8200, 0, -99)] == [250, 250, 250, 250, 251, 2048, 2050, 250, 250]
    assert sh.piece_of(31, 0, 500) == (0, 0) and sh.piece_of(32, 0, 500) == (1, 0) and sh.piece_of(479, 0, 500) == (14, 0)
    assert sh.piece_of(480, 0, 500) == (15, 0) and sh.piece_of(499, 0, 500) == (15, 0)
    assert sh.piece_of(1026, 0, 4100) == (3, 0) and sh.piece_of(1027, 0, 4100) == (3, 1) and sh.piece_of(1028, 0, 4100) == (4, 0)
    assert [sh.ws_jobs_after(b, k) for b, k in ((0, 1), (256, 256), (256, 257), (514, 3))] == [256, 256, 514, 514]


def test_restatement_equals_the_reference(restated, golden):
    assert set(golden) == {c.name for c in sh.all_cases() if c.group != "crossed"}
    for c in sh.all_cases():
        if c.group == "crossed":
            continue
        once, twice, _ = restated[c.name]
        assert np.array_equal(once, golden[c.name][0]), c.name
        assert np.array_equal(twice, golden[c.name][1]), c.name


def test_no_golden_case_leaves_the_vector_and_no_case_leaves_the_array(restated):
    """Asserted from the restatement, so that the golden generator never runs the reference into undefined behaviour; and every index
    of the depth that any call reads -- the crossed cases' second call included -- lies inside it (optimize asserts it per call)."""
    for c in sh.all_cases():
        _, _, reps = restated[c.name]
        inside = [sh.stays_inside(r) for r in reps]
        if c.group == "crossed":
            assert not inside[c.expect["crossed_job"]] and sum(inside) == len(inside) - 1, c.name
        else:
            assert all(inside), c.name
        for r in reps:
            for call in r:
                if call["lo"] is not None:
                    assert 0 <= call["lo"] and call["hi"] < c.depth.size, c.name


def test_lengths_and_reach(restated):
    seen = []
    for c in sh.all_cases():
        if c.group != "lengths":
            continue
        (s, e, t), = c.jobs
        assert e - s + 1 == c.expect["length"] and restated[c.name][2][0][0]["reach"] == c.expect["reach"], c.name
        assert restated[c.name][2][0][0]["early"] is None and (restated[c.name][0] != c.jobs[:, :2]).any(), c.name     # refined, and it moves
        seen.append(int(e - s + 1))
    assert seen == [1, 2, 15, 16, 17, 31, 32, 33, 999, 1000, 1003, 1004, 8192, 8200]
    assert sh.get_case("len_8192").depth.size == 50_000 and (2 * sh.reach_of(8200) + 15) // 16 == 257 > sh.TILE == (2 * sh.reach_of(8192) + 15) // 16


def test_range_checks_a_base_on_each_side(restated):
    n = sh.get_case("from_eq_2len").depth.size
    for name, lhs, rhs, early in (("from_eq_2len", "from", 200, None), ("from_eq_2len_m1", "from", 199, "start"),
                                  ("to_eq_n_m2len", "to", n - 200, None), ("to_eq_n_m2len_p1", "to", n - 199, "end")):
        c = sh.get_case(name)
        (s, e, t), = c.jobs
        assert e - s + 1 == 100 and (s - 250 if lhs == "from" else e + 250) == rhs, name
        first = restated[name][2][0][0]
        assert first["early"] == early == c.expect["early"], name
        assert (restated[name][1] != c.jobs[:, :2]).any() == (early is None), name       # refined and moved, or returned unchanged


def test_extrema_sit_where_they_were_built(restated):
    groups = set()
    for c in sh.all_cases():
        if c.group not in ("seams", "index0", "equal", "zero"):
            continue
        once, twice, reps = restated[c.name]
        groups.add(c.group)
        assert np.array_equal(once, twice), c.name                 # the claim is about the first call; the second moves nothing
        if "win" not in c.expect:
            assert np.array_equal(twice, c.jobs[:, :2]) and c.expect["unmoved"], c.name
            for r in reps:
                if r[0]["early"] is None:
                    assert all(w[2] == 0 and w[4] == -1 and len(w[3]) == w[1] for w in r[0]["win"]), c.name     # every dd is 0
            continue
        first = reps[0][0]
        w = c.expect["win"]
        base, span, ext, attain, imax = first["win"][w]
        (s, e, t), = c.jobs
        if "attain" in c.expect:
            assert attain == c.expect["attain"] and imax == attain[0] and ext != 0, (c.name, attain[:6])
            assert once[0][w] == (first["nstart"] + imax if imax > 0 else c.jobs[0][w]), c.name
        if "zero_other" in c.expect:         # the other search's extremum is exactly 0, everything else of the other sign: nothing moves
            ob, osp, oext, oatt, oimax = first["win"][1 - w]
            assert (oext == 0) == c.expect["zero_other"] and oimax == -1 and len(oatt) < osp and once[0][1 - w] == c.jobs[0][1 - w], c.name
            assert oext == 0 or (oext > 0) == (first["win"][w][2] > 0), c.name        # ... or only values of the sign that does not count
        if c.expect.get("unmoved"):
            assert np.array_equal(once, c.jobs[:, :2]), c.name
        if c.expect.get("ext") == 0:
            assert ext == 0 and imax == -1 and 0 < len(attain) < span and once[0][0] == s, c.name
        if "pieces" in c.expect:
            pa, pb = (sh.piece_of(i, base, span)[0] for i in attain)
            assert {"same_piece": pa == pb, "two_pieces": pb > pa + 1, "neighbour_pieces": pb == pa + 1}[c.expect["pieces"]], c.name
    assert groups == {"seams", "index0", "equal", "zero"}
    # each seam of the 500-entry searches on both sides, in both searches, for both types; the window's last index; the tile seam
    seam = {(c.expect["win"], c.expect["attain"][0] - (599 if c.expect["win"] else 0), int(c.jobs[0][2])) for c in sh.all_cases() if c.group == "seams" and c.depth.size == 5000}
    assert seam == {(w, i, t) for w in (0, 1) for i in (31, 32, 479, 480, 499) for t in (sh.DEL, sh.DUP)}
    assert [c.expect["attain"][0] for c in sh.all_cases() if c.name.startswith("tile_idx")] == [1026, 1027, 1028]
    assert sh.get_case("index0_and_5_del").expect["attain"] == [0, 5]


def test_types_values_and_lists(restated):
    for c in sh.all_cases():
        once, twice, reps = restated[c.name]
        untyped = c.jobs[:, 2] > 1
        assert np.array_equal(twice[untyped], c.jobs[untyped, :2]), c.name           # an untyped candidate is never moved
    for which in ("start", "end"):
        moved = set()
        for step in ("down", "up"):
            c = sh.get_case(f"types_{which}_{step}")
            assert c.jobs[:, 2].tolist() == [sh.DEL, sh.DUP, sh.UNTYPED]
            once = restated[c.name][0]
            moved |= {int(t) for (s, e, t), (a, b) in zip(c.jobs, once) if (a != s if which == "start" else b != e)}
        assert moved == {sh.DEL, sh.DUP}, which
    c = sh.get_case("depth_2p30")
    assert int(c.depth.max()) == 2 ** 30 + 30 and sh.storages(c) == (4,) and (restated[c.name][1] != c.jobs[:, :2]).any()
    assert max(abs(w[2]) for r in restated[c.name][2] for w in r[0]["win"]) > 2 ** 31       # dd beyond 32 bits
    c = sh.get_case("depth_254_255")
    assert set(np.unique(c.depth)) == {254, 255} and sh.storages(c) == (1, 4) and (restated[c.name][1] != c.jobs[:, :2]).any()
    assert [len(sh.get_case(f"jobs_{k}").jobs) for k in (1, 256, 257, 3)] == [1, 256, 257, 3]
    c = sh.get_case("jobs_mixed")
    _, twice, reps = restated[c.name]
    kinds = ["untyped" if t > 1 else ("unchanged" if r[0]["early"] else "refined") for (s, e, t), r in zip(c.jobs, reps)]
    assert kinds == ["refined", "unchanged", "untyped"] * 10
    assert all((twice[i] != c.jobs[i, :2]).any() for i in range(0, 30, 3))
    rnd = [c for c in sh.all_cases() if c.group == "random"]
    lens = [int(e - s + 1) for c in rnd for s, e, t in c.jobs]
    assert len(lens) == 300 and min(lens) >= 20 - 160 and max(lens) > 2500
    assert all(sh.storages(c) == (1, 4) for c in sh.all_cases() if c.name != "depth_2p30")


def test_crossed_cases_cross_in_the_first_call(restated):
    names = [c.name for c in sh.all_cases() if c.group == "crossed"]
    assert len(names) == 4
    changed = 0
    for name in names:
        c = sh.get_case(name)
        once, twice, reps = restated[name]
        k = c.expect["crossed_job"]
        assert once[k][1] < once[k][0] and reps[k][1]["oob"] and reps[k][1]["early"] is None, name
        assert reps[k][1]["win"][0][1] < 2 * reps[k][1]["reach"], name              # fewer entries than the searches want
        changed += int((twice[k] != once[k]).any())
    assert changed > 0        # the rule "the entries that exist" decides something
