"""CPU: the cases of tests/segment_cases.py are what they claim to be, and the restatement of get_rsi_segments they are judged by equals
the compiled reference's answers (golden/segment_edges.npz) bit for bit.  Nothing here touches the library's device code: the claims are
proved from the reference's loop restated in numpy and from the library's host decisions restated next to it.  (oracle/rsi_oracle.cpp
exposes no get_rsi_segments of its own to compare with; pipeline_steps.h's segment_pairs_per_item is checked against hand-computed values
by tests/sanitize/host_harness.cpp, and its restatement here against the same values.)"""
import json
import os
import re

import numpy as np
import pytest

import segment_cases as sg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "segment_edges.npz")


def bits(x):
    return np.asarray(x, dtype=np.float64).view(np.int64)


@pytest.fixture(scope="module")
def restated():
    return {c.name: sg.get_rsi_segments_numpy(c.T, c.status, c.tmedian) for c in sg.all_cases()}


@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN)
    names, off = json.loads(str(z["names"])), z["off"]
    return {n: tuple(z[k][off[i]:off[i + 1]] for k in ("start", "end", "type", "score")) for i, n in enumerate(names)}


def test_the_constants_are_the_librarys():
    """Stated here so that a change shows: the cases are placed by them."""
    assert (sg.THREADS, sg.ROUND, sg.BEST_LDS, sg.RUNS_INLINE, sg.ITEMS_INLINE, sg.MAILBOX_MAX_COPY) == (256, 4, 6144, 200, 150, 524288)
    kh = open(os.path.join(ROOT, "rsicnv_amd", "csrc", "kernels.h")).read()
    assert re.search(r"constexpr int kRunsInline = 200, kItemsInline = 150;", kh)
    assert re.search(r"constexpr int kBestLds = 6144;", kh)
    ph = open(os.path.join(ROOT, "rsicnv_amd", "csrc", "pipeline_internal.h")).read()
    assert re.search(r"kMailboxMaxCopy = size_t\(512\) << 10", ph)
    kb = open(os.path.join(ROOT, "rsicnv_amd", "csrc", "kernels_bin.hip")).read()
    assert "for (int L0 = it.Lbeg; L0 < it.Lend; L0 += 4)" in kb and "j += kThreads" in kb


def test_pairs_per_item_by_hand():
    """len (len + 1) / 2 pairs a run over 150 - 2 runs items of room (8 at least), between 8192 and 65 536; 65 536 on a shared chip."""
    assert sg.pairs_per_item([(0, 99)], lonely=False) == 65536
    assert sg.pairs_per_item([(0, 99)]) == 8192                  # 5050 / 148 + 1 = 35: the floor
    assert sg.pairs_per_item([(10, 2009)]) == 13521              # 2 001 000 / 148 = 13 520.27
    assert sg.pairs_per_item([(0, 8191)]) == 65536               # 33 558 528 / 148: the ceiling
    assert sg.pairs_per_item([(100 * k, 100 * k + 39) for k in range(80)]) == 8201   # 65 600 / 8 + 1
    assert sg.pairs_per_item([]) == 8192
    assert sg.segment_items([(5, 9)], 8) == [(0, 5, 1, 3), (0, 5, 3, 6)]          # 5 + 4 pairs, then 3 + 2 + 1
    assert sg.segment_items([(0, 2), (7, 7)], 1 << 13) == [(0, 3, 1, 4), (1, 1, 1, 2)]


def test_every_case_is_well_formed():
    names = set()
    for c in sg.all_cases():
        assert c.name not in names
        names.add(c.name)
        assert sg.exact_condition(c), c.name
        assert sg.continuous_segments(c.status) == c.runs, c.name     # the runs handed to the device are the ones the reference emits
        assert c.status[-1] != 0 and c.runs[-1][1] < c.T.size - 1, c.name   # ... and the last run is the one it drops
        assert all(e - s + 1 <= sg.MAX_RUN for s, e in c.runs), c.name
        assert c.claim and c.group in ("lengths", "ties", "nothing", "lists", "type", "nb_like"), c.name
    assert len(names) == 65


def test_restatement_equals_the_reference(restated, golden):
    assert set(golden) == {c.name for c in sg.all_cases()}
    for c in sg.all_cases():
        r = restated[c.name]
        gs, ge, gt, gsc = golden[c.name]
        assert [x[0] for x in r] == list(gs) and [x[1] for x in r] == list(ge) and [x[2] for x in r] == list(gt), c.name
        assert np.array_equal(bits([x[3] for x in r]), bits(gsc)), c.name


def test_run_lengths_on_both_sides_of_every_seam():
    single = sorted(c.expect["lengths"][0] for c in sg.all_cases() if c.group == "lengths" and len(c.runs) == 1)
    assert single == [1, 2, 3, 4, 5, 7, 8, 9, 255, 256, 257, 6142, 6143, 6144]
    # a round takes four lengths: 3, 4, 5 and 7, 8, 9 end in, at and behind one; offsets per length against the 256 threads
    for c in sg.all_cases():
        if c.group == "lengths":
            assert [e - s + 1 for s, e in c.runs] == c.expect["lengths"], c.name
            if c.expect.get("adjacent"):
                (s0, e0), (s1, e1) = c.runs
                assert s1 == e0 + 1 and c.status[e0] * c.status[s1] < 0, c.name
    # the prefix has len + 1 entries: 6143 bins are the last that are staged
    assert [sg.expected_info(sg.get_case(f"len_{n}"))[4] for n in (6142, 6143, 6144)] == [0, 0, 1]
    assert sg.expected_info(sg.get_case("pair_6143_6144"))[4] == 1


def test_ties_sit_where_they_were_built(restated):
    for c in sg.all_cases():
        if c.group != "ties":
            continue
        (s, e), = c.runs
        a, b, ty, score, attain = restated[c.name][0]
        want = sorted(c.expect["attain"])
        assert sorted(attain) == want, (c.name, attain[:6])
        assert (b - a + 1, a - s) == want[0], c.name            # the first in (L, offset) order wins
        assert score != 0
        if "same_thread" in c.expect:
            (_, j0), (_, j1) = want
            assert (j0 % sg.THREADS == j1 % sg.THREADS) == c.expect["same_thread"], c.name
        if "split" in c.expect:
            ppi = c.pairs_per_item or sg.pairs_per_item(c.runs)
            items = sg.segment_items(c.runs, ppi)
            owner = [next(i for i, (_, _, lb, le) in enumerate(items) if lb <= L < le) for L in c.expect["split"]]
            assert owner[0] != owner[1], (c.name, items[:3])
    assert {c.pairs_per_item for c in sg.all_cases() if "split" in c.expect} == {0, 8192, 65536}
    assert sg.pairs_per_item(sg.get_case("tie_L1_L64_items_0_int").runs) == 8192      # what a run chooses for 1200 bins
    apart = sorted(abs(c.expect["attain"][1][1] - c.expect["attain"][0][1]) for c in sg.all_cases() if c.name.startswith("tie_offsets") and c.name.endswith("int"))
    assert apart == [100, 256, 400]
    for stem in ("first_offset", "last_offset", "whole_run", "first_and_last", "tie_L1_L4", "tie_L1_L64", "tie_offsets_100"):
        assert {c.tmedian for c in sg.all_cases() if c.name.startswith(stem)} >= {10.0, 10.5}, stem


def test_nothing_scores(restated):
    seen = set()
    for c in sg.all_cases():
        if c.group != "nothing":
            continue
        (s, e), = c.runs
        a, b, ty, score, attain = restated[c.name][0]
        assert (a, b) == (s, e) and attain == [] and score == 0, c.name
        assert ty == (sg.DUP if c.status[s] > 0 else sg.DEL), c.name
        assert bool(np.signbit(score)) == (ty == sg.DEL), c.name      # the reference stores -optscore: -0.0
        seen.add((e - s + 1, ty))
    assert seen == {(1, sg.DEL), (1, sg.DUP), (300, sg.DEL), (300, sg.DUP)}


def test_list_forms_on_both_sides_of_every_boundary():
    info = {c.name: sg.expected_info(c) for c in sg.all_cases()}
    # an item per run at least: 150 runs are the last whose lists ride in the kernel arguments; kRunsInline (200) is never the
    # boundary of this stage, 200 and 201 runs both go the pointer way
    assert [info[f"runs_{k}"][:3] for k in (150, 151, 200, 201)] == [[150, 150, 1], [151, 151, 0], [200, 200, 0], [201, 201, 0]]
    assert [info[f"items_{k}"][:3] for k in (150, 151)] == [[1, 150, 1], [1, 151, 0]]
    assert info["mailbox_at_limit"][:5] == [16, 16, 1, 1, 16] and info["mailbox_beyond"][:5] == [17, 17, 1, 0, 16]
    assert sum(e - s + 1 for s, e in sg.get_case("mailbox_at_limit").runs) * 4 == sg.MAILBOX_MAX_COPY
    assert sum(e - s + 1 for s, e in sg.get_case("mailbox_beyond").runs) * 4 == sg.MAILBOX_MAX_COPY + 4
    assert {i[2] for i in info.values()} == {0, 1} and {i[3] for i in info.values()} == {0, 1}


def test_types_and_levels(restated):
    for c in sg.all_cases():
        if c.group != "type":
            continue
        for (s, e), (a, b, ty, score, attain) in zip(c.runs, restated[c.name]):
            assert ty == (sg.DUP if c.status[s] > 0 else sg.DEL), c.name
        mixed = [(run, seg) for run, seg in zip(c.runs, restated[c.name]) if len(set(c.status[run[0]:run[1] + 1])) == 3]
        assert len(mixed) == 1, c.name
        (s, e), (a, b, _, _, _) = mixed[0]
        assert len(set(c.status[a:b + 1])) == 1 and (a > s or b < e), c.name      # the segment covers part of the run's levels
    for name in ("mailbox_at_limit", "mailbox_beyond"):
        c = sg.get_case(name)
        assert {abs(int(v)) for v in c.status[c.runs[0][0]:c.runs[0][1] + 1]} == {1, 7, 40}
        assert len({(a - s, b - a) for (s, e), (a, b, _, _, _) in zip(c.runs[:2], restated[name][:2])}) == 2   # neighbours differ


def test_the_bulk(restated):
    runs = sum(len(c.runs) for c in sg.all_cases() if c.group == "nb_like")
    assert runs == 300
    lens = [e - s + 1 for c in sg.all_cases() if c.group == "nb_like" for s, e in c.runs]
    assert min(lens) <= 3 and max(lens) >= 390
