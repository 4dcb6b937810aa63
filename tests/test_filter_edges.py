"""GPU: filterstatus alone (rsi_hot_debug_filterstatus: the scan pass's own last launch, then the function the scan calls behind its first
pass -- level sums, choose_levels, runs_from_export, prepare_runs, k_trim_runs) on every case of tests/filter_cases.py, against the
reference's filterstatus (golden/filter_edges.npz) bit for bit, with the road taken (info[]) against what the restated constants say it
must be.  One context for everything, small and large cases in turn, then the cases again."""
import json
import os
import time

import numpy as np
import pytest

import filter_cases as fc

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "filter_edges.npz")


@pytest.fixture(scope="module")
def hot():
    from rsicnv_amd import api
    h = api.RsiHot(0)
    yield h
    h.close()


@pytest.fixture(scope="module")
def expected():
    """Per case: the status the reference leaves (the restatement's for the one case the reference cannot run) and the restatement's
    account of how it got there.  Computed once."""
    z = np.load(GOLDEN)
    names, off, d = json.loads(str(z["names"])), z["off"], z["cleared_diff"]
    cleared = {n: np.cumsum(d[off[i]:off[i + 1]]) for i, n in enumerate(names)}
    out = {}
    for c in fc.all_cases():
        f = fc.filterstatus_numpy(c.T, c.status, c.dev)
        want = c.status.copy()
        if c.name == "no_unmarked_bin":
            assert np.array_equal(f.status, c.status)
        else:
            want[cleared[c.name]] = 0          # a case without a golden answer is a failure, not a skip
        out[c.name] = (want, fc.expected_info(c, f))
    return out


def alternating(cases):
    """Small and large in turn: a context whose buffers a large case has grown runs a small one next, and back."""
    by_size = sorted(cases, key=lambda c: (c.T.size, c.name))
    order = []
    while by_size:
        order.append(by_size.pop(0))
        if by_size:
            order.append(by_size.pop())
    return order


def run_cases(hot, expected, cases):
    spent, forms = {}, set()
    for c in alternating(cases):
        want, info_want = expected[c.name]
        t0 = time.perf_counter()
        got, info = hot.debug_filterstatus(c.T, c.status, c.Lmax, c.dev)
        spent[c.group] = spent.get(c.group, 0.0) + time.perf_counter() - t0
        where = f"{c.name} ({c.claim}): info {list(info)}"
        assert list(info[:9]) == info_want, f"{where}, expected {info_want}"
        assert np.array_equal(got, want), f"{where}: first differences at bins {np.nonzero(got != want)[0][:8]}"
        if info_want[5] and info_want[0] > 0:
            # what came back is the trimmed copy, not the pass's untrimmed status (which is the input)
            assert not np.array_equal(got, c.status), where
        forms.add(tuple(int(v) for v in info[1:4]))
    print("seconds per group:", {g: round(t, 3) for g, t in sorted(spent.items())})
    return forms


def test_every_case_twice_on_one_context(hot, expected):
    cases = fc.all_cases()
    forms = run_cases(hot, expected, cases)
    # read, not inferred: run lists inline and behind pointers, boundary entries eager and copied, all three level-sums routes
    assert {f[0] for f in forms} >= {0, 1} and {f[1] for f in forms} >= {0, 1} and {f[2] for f in forms} == {0, 1, 2}, forms
    run_cases(hot, expected, cases)


def test_bad_arguments_leave_the_context_usable(hot, expected):
    from rsicnv_amd import api
    c = fc.get_case("walk_len_3")
    for T, st, Lmax in ((c.T, c.status, 0), (c.T, c.status, (1 << 22) + 1), (c.T, np.where(c.status < 0, -100, c.status), 99),
                        (c.T, np.where(c.status > 0, 100, c.status), 99)):
        with pytest.raises(api.RsiError) as err:
            hot.debug_filterstatus(T, st, Lmax, c.dev)
        assert err.value.code == -2
    got, info = hot.debug_filterstatus(c.T, c.status, c.Lmax, c.dev)
    assert np.array_equal(got, expected[c.name][0]) and list(info[:9]) == expected[c.name][1]
