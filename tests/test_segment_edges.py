"""GPU: the segment search alone (rsi_hot_debug_segments: k_run_prefix, k_best_subsegment, segment_items / segments_from_best around
them -- the function the scan calls behind its second pass) on every case of tests/segment_cases.py, against the reference's
get_rsi_segments (golden/segment_edges.npz) bit for bit, scores included, with the road taken (info[]) against what the restated
constants say it must be.  One context for everything, small and large cases in turn, a whole chromosome in between."""
import json
import os
import time

import numpy as np
import pytest

import golden_util as gu
import segment_cases as sg

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "segment_edges.npz")


@pytest.fixture(scope="module")
def hot():
    from rsicnv_amd import api
    h = api.RsiHot(0)
    yield h
    h.close()


@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN)
    names, off = json.loads(str(z["names"])), z["off"]
    return {n: tuple(z[k][off[i]:off[i + 1]] for k in ("start", "end", "type", "score")) for i, n in enumerate(names)}


def alternating(cases):
    """Small and large in turn: a context whose buffers a large case has grown runs a small one next, and back."""
    by_size = sorted(cases, key=lambda c: (c.T.size, c.name))
    order = []
    while by_size:
        order.append(by_size.pop(0))
        if by_size:
            order.append(by_size.pop())
    return order


def run_cases(hot, golden, cases):
    spent, forms = {}, set()
    for c in alternating(cases):
        gs, ge, gt, gsc = golden[c.name]          # a case without a golden answer is a failure, not a skip
        t0 = time.perf_counter()
        s, e, ty, sc, info = hot.debug_segments(c.T, c.status, sg.run_list(c), c.tmedian, 0.0, c.pairs_per_item)
        spent[c.group] = spent.get(c.group, 0.0) + time.perf_counter() - t0
        where = f"{c.name} ({c.claim}): info {list(info)}"
        assert list(info[:7]) == sg.expected_info(c), where
        assert np.array_equal(s, gs) and np.array_equal(e, ge), f"{where}: first difference at segment {np.nonzero((s != gs) | (e != ge))[0][:5]}"
        assert np.array_equal(ty, gt), where
        assert np.array_equal(sc.view(np.int64), gsc.view(np.int64)), f"{where}: scores differ at {np.nonzero(sc.view(np.int64) != gsc.view(np.int64))[0][:5]}"
        forms.add((int(info[2]), int(info[3]), int(info[4] > 0)))
    print("seconds per group:", {g: round(t, 3) for g, t in sorted(spent.items())})
    return forms


def test_every_case_then_a_chromosome_then_every_case(hot, hotlib, golden):
    cases = sg.all_cases()
    forms = run_cases(hot, golden, cases)
    # read, not inferred: lists inline and behind pointers, status through the mailbox and copied, prefixes staged and not
    assert {f[0] for f in forms} == {0, 1} and {f[1] for f in forms} == {0, 1} and {f[2] for f in forms} == {0, 1}, forms
    gu.check_hip_against_golden(hot, hotlib, "poisson_nb_m101")       # a normal run on the context the hook has used ...
    run_cases(hot, golden, [c for c in cases if c.group in ("ties", "nothing", "type") or c.name in ("runs_151", "len_6144")])   # ... and back


def test_the_half_tlamda_filter_and_bad_run_lists(hot):
    from rsicnv_amd import api
    c = sg.get_case("tie_L1_L4_int")                  # one run, score 4
    assert hot.debug_segments(c.T, c.status, sg.run_list(c), c.tmedian, 8.0)[3].tolist() == [4.0]      # |score| < tlamda / 2 is strict
    s, e, ty, sc, info = hot.debug_segments(c.T, c.status, sg.run_list(c), c.tmedian, float(np.nextafter(8.0, 9.0)))
    assert sc.size == 0 and info[5] == 0 and info[0] == 1
    nb = c.T.size
    for bad in ([(5, 4)], [(-1, 3)], [(0, nb)], [(10, 20), (20, 30)], [(30, 40), (10, 20)]):
        with pytest.raises(api.RsiError) as err:
            hot.debug_segments(c.T, c.status, np.array(bad, dtype=np.int32), c.tmedian)
        assert err.value.code == -2, bad
    assert hot.debug_segments(c.T, c.status, np.zeros((0, 2), dtype=np.int32), c.tmedian)[4][0] == 0     # no runs: no segments
    assert hot.debug_segments(c.T, c.status, sg.run_list(c), c.tmedian)[3].tolist() == [4.0]              # and the context is fine
