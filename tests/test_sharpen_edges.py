"""GPU: the edge refinement alone (rsi_hot_debug_sharpen: DeviceTester::sharpen, both launches of k_sharpen_edges, the context's own
workspace) on every case of tests/sharpen_cases.py, coordinate for coordinate against the reference's optimize_with_derivative called
twice (golden/sharpen_edges.npz) -- for the group `crossed`, where the reference leaves its vector, against the restatement's rule --
with the depth kept as bytes and as int32 wherever it fits a byte.  One context for everything, small and large cases in turn, the job
lists in the order that regrows the workspace, a whole chromosome in between."""
import json
import os
import time

import numpy as np
import pytest

import golden_util as gu
import sharpen_cases as sh

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sharpen_edges.npz")


@pytest.fixture(scope="module")
def hot():
    from rsicnv_amd import api
    h = api.RsiHot(0)
    yield h
    h.close()


@pytest.fixture(scope="module")
def expected():
    """name -> [k, 2] start / end after both calls: the golden file's, the restatement's for `crossed`.  Computed once and shared."""
    z = np.load(GOLDEN)
    names, off = json.loads(str(z["names"])), z["off"]
    out = {n: z["twice"][off[i]:off[i + 1]] for i, n in enumerate(names)}
    for c in sh.all_cases():
        if c.group == "crossed":
            out[c.name] = sh.refine_jobs(c, 2)[0]
    return out


def alternating(cases):
    by_size = sorted(cases, key=lambda c: (c.depth.size * 1000 + len(c.jobs), c.name))
    order = []
    while by_size:
        order.append(by_size.pop(0))
        if by_size:
            order.append(by_size.pop())
    return order


def run_case(hot, expected, c, spent, ws=None):
    exp = expected[c.name]                     # a case without an expected answer is a failure, not a skip
    for storage in sh.storages(c):
        t0 = time.perf_counter()
        s, e, info = hot.debug_sharpen(c.depth, storage, c.jobs[:, 0], c.jobs[:, 1], c.jobs[:, 2])
        spent[c.group] = spent.get(c.group, 0.0) + time.perf_counter() - t0
        got = np.stack([s, e], axis=1)
        bad = np.nonzero((got != exp).any(axis=1))[0]
        assert bad.size == 0, (f"{c.name} ({c.claim}), storage {storage}: {bad.size} of {len(c.jobs)} jobs differ, first {bad[:5]}: "
                               f"jobs {c.jobs[bad[:3]].tolist()} got {got[bad[:3]].tolist()} expected {exp[bad[:3]].tolist()}, info {list(info)}")
        assert info[2] == 1, c.name            # the job list rode in the mailbox
        if ws is not None:                     # the workspace before and after, read from the context
            assert (info[0], info[1]) == (ws[0], sh.ws_jobs_after(ws[0], len(c.jobs))), (c.name, list(info), ws)
            ws[0] = int(info[1])


def test_every_case_then_a_chromosome_then_every_case(hot, hotlib, expected):
    cases = sh.all_cases()
    spent, ws = {}, [0]
    lists = [sh.get_case(f"jobs_{k}") for k in (1, 256, 257, 3)]
    run_case(hot, expected, lists[0], spent, ws)                     # a new context: the workspace is laid out for 256 jobs
    assert ws == [256]
    for c in alternating([c for c in cases if c not in lists]):
        run_case(hot, expected, c, spent, ws)
    assert ws == [256]
    for c in lists[1:]:                                              # 256 jobs fit; 257 regrow and clear it; 3 jobs run in the regrown one
        run_case(hot, expected, c, spent, ws)
    assert ws == [514]
    run_case(hot, expected, sh.get_case("jobs_mixed"), spent, ws)
    print("seconds per group:", {g: round(t, 3) for g, t in sorted(spent.items())})
    gu.check_hip_against_golden(hot, hotlib, "poisson_nb_m101")      # a normal run on the context the hook has used ...
    again = [c for c in cases if c.group in ("seams", "index0", "equal", "crossed", "values") or c.name in ("jobs_257", "len_8200", "len_1")]
    for c in alternating(again):                                     # ... and back
        run_case(hot, expected, c, {})


def test_bad_arguments(hot):
    from rsicnv_amd import api
    c = sh.get_case("depth_2p30")
    for storage in (1, 2):                     # a depth beyond a byte in byte storage; a storage that does not exist
        with pytest.raises(api.RsiError) as err:
            hot.debug_sharpen(c.depth, storage, c.jobs[:, 0], c.jobs[:, 1], c.jobs[:, 2])
        assert err.value.code == -2
    c = sh.get_case("constant")
    s, e, _ = hot.debug_sharpen(c.depth, 1, c.jobs[:, 0], c.jobs[:, 1], c.jobs[:, 2])
    assert np.array_equal(s, c.jobs[:, 0]) and np.array_equal(e, c.jobs[:, 1])
