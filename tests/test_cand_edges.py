"""GPU: the neighbourhood test of a candidate alone (rsi_hot_debug_candidate_tests: plan_test, DeviceTester::test over k_candidate_test or
k_cand_gather / k_cand_sums / k_cand_hist, finish_judgement, the host walk where the device declines) on every case of tests/cand_cases.py,
in every storage and form the case's values allow, record by record:

  the plan, flags, nref, nbody, nwin, both reaches, the candidate's minimum, maximum, sum and sum of squares and all six quantiles bit for
  bit against the restatement of the reference's loops (tests/cand_cases.py, which tests/test_cand_cases.py pins to the compiled reference);
  the two float moments of the window means against the exactly rounded sums of the restatement's means, within (nwin - 1) 2^-53 sum|term|;
  byte against int32 storage bit for bit in everything;
  the judged candidate against the reference's own answer (golden/cand_edges.npz), whichever road judged it, and the road is the predicted one.

One exception to "bit for bit", stated where it is compared: where the means' range is below 0.01 but not 0 the reference's median IS the
mean of the means, summed in index order; the device divides its own sum, so that one value is held to the moments' bound.  (Constant
means whose sums are exact in any order are compared bit for bit.)

Neither the reference nor libref.so is read here."""
import time

import numpy as np
import pytest

import cand_cases as cc

pytestmark = pytest.mark.gpu
PLAN = ("capacity", "top", "margin", "cut")
GROUPS = sorted({c.group for c in cc.all_cases()} - {"lists"})


@pytest.fixture(scope="module")
def hot():
    from rsicnv_amd import api
    h = api.RsiHot(0)
    h.set_timing(1)          # rsi_hot_kernel_times names what ran
    yield h
    h.close()


@pytest.fixture(scope="module")
def golden():
    return cc.load_golden()


def call(hot, c, storage, form, index=None):
    return hot.debug_candidate_tests(c.depth, storage, c.span_all, c.RDmedian, c.cands, c.index if index is None else index, form, **c.P)


def expected_judgement(c, golden, k, ci):
    """The golden file's record; for the groups the reference has no behaviour in, the restatement's rule."""
    return golden[c.name][k] if cc.in_golden(c) else cc.restated(c)[ci]["judged"]


def check_record(c, ci, storage, form, got, want_j):
    r = cc.restated(c)[ci]
    T, split = r["plan"], form & 1
    tag = (c.name, c.claim, ci, storage, form)
    assert tuple(int(got[k]) for k in PLAN) == tuple(T[k] for k in PLAN), tag
    assert (int(got["nleft"]), int(got["nright"])) == (len(T["left_chain"]), len(T["right_chain"])), tag
    flags = r["flags"][split]
    assert int(got["flags"]) == flags, (tag, int(got["flags"]), flags)
    assert int(got["road"]) == (1 if flags else 0), tag                      # a record the device served never goes to the host walk
    if not flags & 24:       # (a used-up chain or a short vouched walk: the device's neighbourhood is not the reference's, by design)
        assert (int(got["nref"]), int(got["nbody"]), int(got["nwin"])) == (r["nref"], r["nbody"], r["nwin"]), tag
        assert int(got["left_reach"]) == r["left_reach"], (tag, int(got["left_reach"]), r["left_reach"])
        # the right walk's reach: the one-workgroup form and the vouched split form walk with the slots the left side leaves; the split
        # form otherwise gives its right walk all of `capacity` and legitimately walks on
        rr = r["right_reach"] if not split or (T["cut"] & 4) else r["right_reach_free"]
        assert int(got["right_reach"]) == rr, (tag, int(got["right_reach"]), rr)
    if not flags & 25:
        assert (int(got["body_min"]), int(got["body_max"])) == (r["body_min"], r["body_max"]), tag
        assert (float(got["body_s1"]), float(got["body_s2"])) == (r["body_s1"], r["body_s2"]), tag
        if not flags & 2:
            assert tuple(got["body_q"].tolist()) == tuple(r["body_q"]), (tag, got["body_q"], r["body_q"])
        assert abs(float(got["ref_s1"]) - r["ref_s1"]) <= r["ref_s1_bound"], (tag, float(got["ref_s1"]), r["ref_s1"], r["ref_s1_bound"])
        assert abs(float(got["ref_s2"]) - r["ref_s2"]) <= r["ref_s2_bound"], (tag, float(got["ref_s2"]), r["ref_s2"], r["ref_s2_bound"])
        if not flags & 4:
            q = got["ref_q"].tolist()
            if r["ref_nbk"] is None:     # range below 0.01: minimum, mean, maximum; the mean from the device's own sum
                assert (q[0], q[2]) == (r["ref_q"][0], r["ref_q"][2]), tag
                if r["constant_means"]:      # every sum is exact in any order: the same bits
                    assert q[1] == r["ref_q"][1], (tag, q[1], r["ref_q"][1])
                assert abs(q[1] - r["ref_s1"] / r["nwin"]) <= r["ref_s1_bound"] / r["nwin"] + 2.0 ** -52 * abs(q[1]), tag
            else:
                assert tuple(q) == tuple(r["ref_q"]), (tag, q, r["ref_q"])
    # the judged candidate
    for k in ("type", "status", "geno"):
        assert int(got[k]) == want_j[k], (tag, k, int(got[k]), want_j[k])
    if r["empty"]:
        return
    for k in cc.EXACT:
        if k == "refmed" and r["ref_nbk"] is None and not r["constant_means"] and not flags:
            assert abs(float(got[k]) - want_j[k]) <= 2 * r["ref_s1_bound"] / r["nwin"] + 2.0 ** -51 * abs(want_j[k]), (tag, k)
        else:
            assert float(got[k]) == want_j[k], (tag, k, float(got[k]), want_j[k])
    for k in cc.CLOSE:
        assert np.isclose(float(got[k]), want_j[k], rtol=1e-6, atol=1e-300), (tag, k, float(got[k]), want_j[k])


def same_bits(a, b, skip=()):
    return all(a[k].tobytes() == b[k].tobytes() for k in a.dtype.names if k not in skip)


def run_case(hot, c, golden, spent, index=None, copied=False, on_info=None):
    index = c.index if index is None else index
    where = {ci: k for k, ci in enumerate(c.index)}
    got = {}
    for storage, form in cc.forms(c):
        t0 = time.perf_counter()
        recs, info = call(hot, c, storage, form, index)
        spent[c.group] = spent.get(c.group, 0.0) + time.perf_counter() - t0
        ran = {k for k, _ in hot.kernel_times() if k.startswith("candidate_test")}
        assert ran == {cc.kernel_name(storage, form)}, (c.name, storage, form, ran)
        assert info[0] == 1 and (info[1], info[2]) == ((0, 1) if copied else (1, 0)), (c.name, list(info))
        if on_info:
            on_info(storage, form, info)
        for k, ci in enumerate(index):
            check_record(c, ci, storage, form, recs[k], expected_judgement(c, golden, where[ci], ci))
        got[storage, form] = recs
    # the width of the depth and of the gathered values changes no bit (a record without a neighbourhood carries nothing but its counts)
    full = np.array([not cc.restated(c)[ci]["empty"] for ci in index])
    for split in (1, 0):
        base = got[4, split]
        for storage, form in cc.forms(c):
            if form & 1 == split and (storage, form) != (4, split):
                assert same_bits(got[storage, form][full], base[full]), (c.name, storage, form)
    return got


def alternating(cases):
    by_size = sorted(cases, key=lambda c: (c.depth.size, c.name))
    order = []
    while by_size:
        order.append(by_size.pop(0))
        if by_size:
            order.append(by_size.pop())
    return order


@pytest.mark.parametrize("group", GROUPS)
def test_group_in_every_form_twice(hot, golden, group):
    """One context for all groups; inside a group small and large cases in turn; everything twice."""
    cases = alternating([c for c in cc.all_cases() if c.group == group])
    spent = {}
    for _ in range(2):
        for c in cases:
            run_case(hot, c, golden, spent)
    print(f"{group}: {len(cases)} cases, {2 * sum(len(cc.forms(c)) for c in cases)} hook calls, {spent[group]:.3f} s")


def list_index(c, k):
    return c.index[:k] if k != 3 else [c.index[7], c.index[150], c.index[300]]


def test_lists_grow_and_shrink_on_one_context(golden):
    """A new context: job lists of 1, 300, 3, 301 and 1 jobs in that order, in all six forms, for both kinds; then every other case of the
    file; then the lists again.  The per-job records and folded histograms of the split form are grown, then reused with a capacity no
    list has asked for, and must have been left zero by every launch: every record is compared as everywhere else."""
    from rsicnv_amd import api
    h = api.RsiHot(0)
    h.set_timing(1)
    try:
        spent = {}

        def capacities(c, k):
            def look(storage, form, info):
                if form & 1:             # CandMid is 464 bytes a job, a folded histogram 65 536
                    mid0, mid1, hist0, hist1 = (int(x) for x in info[3:7])
                    assert mid1 >= k * 464 and hist1 >= k * 65536, (c.name, k, list(info))
                    assert (mid1 == mid0) == (mid0 >= k * 464) and (hist1 == hist0) == (hist0 >= k * 65536), (c.name, k, list(info))
            return look
        for rnd in range(2):
            for c in (cc.get_case("list_301_del"), cc.get_case("list_301_dup")):
                for k in c.expect["lists"]:
                    run_case(h, c, golden, spent, index=list_index(c, k), on_info=capacities(c, k))
            if rnd == 0:
                for c in alternating([c for c in cc.all_cases() if c.group != "lists"]):
                    run_case(h, c, golden, spent)
        print("seconds:", {g: round(t, 3) for g, t in sorted(spent.items())}, "total", round(sum(spent.values()), 3))
    finally:
        h.close()


@pytest.mark.parametrize("name", ["list_301_del", "list_301_dup"])
def test_every_record_alone_and_inside_the_list(hot, name):
    """In each of the six forms: a record tested alone has the bits it has inside the list of 301."""
    c = cc.get_case(name)
    t0 = time.perf_counter()
    for storage, form in cc.forms(c):
        inside, _ = call(hot, c, storage, form)
        for ci in c.index:
            recs, _ = call(hot, c, storage, form, [ci])
            assert same_bits(recs[0:1], inside[ci:ci + 1]), (c.name, ci, storage, form)
    print(f"{name}: {len(cc.forms(c)) * 302} hook calls, {time.perf_counter() - t0:.3f} s with the comparisons")


@pytest.mark.parametrize("name", ["list_copied_del", "list_copied_dup"])
def test_a_list_too_long_for_the_mailbox(hot, golden, name):
    spent = {}
    for _ in range(2):
        run_case(hot, cc.get_case(name), golden, spent, copied=True)
    print(f"{name}: {spent}")


def test_range_sums(hot):
    for name, d, lo, hi in cc.range_cases():
        want = np.array([int(d[a:b + 1].astype(np.int64).sum()) for a, b in zip(lo, hi)], dtype=np.int64)
        for storage in ((1, 4) if int(d.max()) <= 255 else (4,)):
            got, info = hot.debug_range_sums(d, storage, lo, hi)
            assert np.array_equal(got, want), (name, storage, np.nonzero(got != want)[0][:5])
            assert info[0] == 1 and info[1] == 1, (name, list(info))
            assert {k for k, _ in hot.kernel_times()} == {"range_sums"}


def test_bad_arguments_leave_the_context_usable(hot, golden):
    from rsicnv_amd import api
    c = cc.get_case("seam_7_del")
    good = (c.depth, 1, c.span_all, c.RDmedian, c.cands, c.index, 1)

    def refused(*a, **kw):
        with pytest.raises(api.RsiError) as err:
            hot.debug_candidate_tests(*a, **kw)
        assert err.value.code == -2

    other = c.cands.copy()
    other[0, 2] = 2
    refused(c.depth, 1, c.span_all, c.RDmedian, other, c.index, 1, **c.P)                      # a type the reference exits on
    wide = c.depth.copy()
    wide[5] = 256
    refused(wide, 1, c.span_all, c.RDmedian, c.cands, c.index, 1, **c.P)                       # beyond a byte under storage 1
    refused(c.depth, 2, c.span_all, c.RDmedian, c.cands, c.index, 1, **c.P)                    # a storage that does not exist
    refused(c.depth, 1, c.span_all, c.RDmedian, c.cands, [1], 1, **c.P)                        # an index outside the list
    refused(c.depth, 1, c.span_all, c.RDmedian, c.cands, c.index, 4, **c.P)                    # a form that does not exist
    outside = c.cands.copy()
    outside[0, 1] = c.depth.size
    refused(c.depth, 1, c.span_all, c.RDmedian, outside, c.index, 1, **c.P)                    # a candidate that ends behind the array
    refused(c.depth, 1, c.span_all, c.RDmedian, c.cands, c.index, 1, **dict(c.P, chklen=0.0))  # no capacity
    refused(c.depth, 1, c.span_all, c.RDmedian, c.cands, c.index, 1, **dict(c.P, chklen=0.01))
    for lo, hi in (([5], [4]), ([0], [c.depth.size]), ([-1], [3])):
        with pytest.raises(api.RsiError) as err:
            hot.debug_range_sums(c.depth, 1, lo, hi)
        assert err.value.code == -2
    recs, _ = hot.debug_candidate_tests(*good, **c.P)
    check_record(c, c.index[0], 1, 1, recs[0], golden[c.name][0])
