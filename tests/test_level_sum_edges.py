"""GPU: filterstatus' level sums alone (rsi_hot_debug_level_sums: k_fs_chunk_sums, k_fs_chunk_fns, k_fs_level_sums) on every case of
tests/level_sum_cases.py, against the sequential float32 accumulation in index order: counts equal, sums equal bit for bit, no tolerance.
What each case was built for is proved on the CPU (tests/test_level_sum_cases.py).  One context for everything, small and large cases
in turn, then the cases again; a fresh context for the one large case."""
import time

import numpy as np
import pytest

import level_sum_cases as lc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hot():
    from rsicnv_amd import api
    h = api.RsiHot(0)
    yield h
    h.close()


@pytest.fixture(scope="module")
def expected():
    """Per case the yardstick's sums and counts.  Computed once."""
    return {c.name: lc.level_sums(c.T, c.status, c.Lmax) for c in lc.all_cases()}


def alternating(cases):
    """Small and large in turn: a context whose buffers a large case has grown runs a small one next, and back."""
    by_size = sorted(cases, key=lambda c: (c.T.size, c.name))
    order = []
    while by_size:
        order.append(by_size.pop(0))
        if by_size:
            order.append(by_size.pop())
    return order


def check(hot, c, want):
    got_s, got_c = hot.debug_level_sums(c.T, c.status, c.Lmax)
    where = f"{c.name} [{c.group}] ({c.claim})"
    if c.expect.get("declined"):
        assert got_c[c.Lmax] == -1, where          # the other outputs are unspecified
        return
    exp_s, exp_c = want
    assert np.array_equal(got_c, exp_c), f"{where}: counts differ at levels {np.nonzero(got_c != exp_c)[0][:8] - c.Lmax}"
    assert np.array_equal(got_s.view(np.uint32), exp_s.view(np.uint32)), \
        f"{where}: " + str([(l - c.Lmax, float(a), float(b)) for l, (a, b) in enumerate(zip(got_s, exp_s)) if a.view(np.uint32) != b.view(np.uint32)][:5])


def run_cases(hot, expected, cases):
    spent, failed = {}, []
    for c in alternating(cases):
        t0 = time.perf_counter()
        try:
            check(hot, c, expected[c.name])
        except AssertionError as e:                # every case runs: the list of those that fail is what a reader wants
            failed.append(str(e))
        spent[c.group] = spent.get(c.group, 0.0) + time.perf_counter() - t0
    print("seconds per group:", {g: round(t, 3) for g, t in sorted(spent.items())})
    assert not failed, f"{len(failed)} of {len(cases)} cases:\n" + "\n".join(failed)


def test_every_case_twice_on_one_context(hot, expected):
    cases = lc.all_cases()
    assert {c.group for c in cases} == {"crossing", "landing", "order", "several", "start", "overflow", "marked"}
    run_cases(hot, expected, cases)
    run_cases(hot, expected, cases)


def test_premise_on_a_fresh_context():
    """23 000 005 unmarked bins whose float sum stays at 2^24: from chunk 11 084 on neither candidate binade fits and every chunk is staged."""
    from rsicnv_amd import api
    c = lc.premise_case()
    want = lc.level_sums(c.T, c.status, c.Lmax)
    assert float(want[0][c.Lmax]) == c.expect["unmarked"]
    h = api.RsiHot(0)
    try:
        check(h, c, want)
    finally:
        h.close()


def test_status_outside_the_level_range_is_refused(hot, expected):
    from rsicnv_amd import api
    c = lc.get_case("marked_lmax_2")
    low, high = c.status.copy(), c.status.copy()
    low[np.nonzero(c.status)[0][0]] = -3
    high[np.nonzero(c.status)[0][-1]] = 3
    for st in (low, high):
        with pytest.raises(api.RsiError) as err:
            hot.debug_level_sums(c.T, st, c.Lmax)
        assert err.value.code == -2
    check(hot, c, expected[c.name])                # the context is still usable
