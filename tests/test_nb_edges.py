"""GPU: the NB transform alone (rsi_hot_debug_nb_transform: k_nb_raw, nb_reference_levels, k_nb_scale_mm -- the function a run calls) on
every case of tests/nb_cases.py against the restatement that tests/test_nb_cases.py pins to the reference, on the raw values and on the
scaled ones.  The bar (nb_cases.py): the same float outside hard inputs -- inputs whose double lies within 8 units of its last place of a
midpoint between two floats -- and at most one float step on them.  The only arithmetic the device does not share with the reference is
the double log (glibc there, OCML here); the hard list (golden/nb_edges.npz) is where a difference would show, and the count is printed."""
import os
import time

import numpy as np
import pytest

import nb_cases as nc

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nb_edges.npz")


def bits(x):
    return np.asarray(x, dtype=np.float32).view(np.int32)


@pytest.fixture(scope="module")
def hot():
    from rsicnv_amd import api
    h = api.RsiHot(0)
    yield h
    h.close()


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def check(hot, c, f=None):
    """One case through the hook; returns (bins whose raw value differs, bins whose scaled value differs), each within the bar."""
    f = f or nc.transform(c.binsum, c.m, c.ncompact, c.RDmedian, c.r)
    raw, T, info = hot.debug_nb_transform(c.binsum, c.m, c.ncompact, c.RDmedian, c.r)
    where = f"{c.name} ({c.claim})"
    d_raw, d_T = nc.float_steps(raw, f.raw), nc.float_steps(T, f.T)
    assert (d_raw[~f.hard_raw] == 0).all(), f"{where}: raw differs on ordinary bins {np.nonzero((d_raw != 0) & ~f.hard_raw)[0][:8]}"
    assert (d_raw <= 1).all(), f"{where}: raw differs by more than a float step at {np.nonzero(d_raw > 1)[0][:8]}"
    assert (d_T[~f.hard_T] == 0).all(), f"{where}: T differs on ordinary bins {np.nonzero((d_T != 0) & ~f.hard_T)[0][:8]}"
    assert (d_T <= 1).all(), f"{where}: T differs by more than a float step at {np.nonzero(d_T > 1)[0][:8]}"
    # info speaks of the arrays that came back: the raw minimum, the plan from T's min / max / non-finite values, t0 and t2
    finite = raw[~np.isnan(raw)]
    assert info[0] == bits(finite.min() if finite.size else raw[0]), where
    flags, buckets, ymin = nc.plan(T)
    assert (int(info[1]), int(info[2])) == (flags, buckets) and info[3] == bits(ymin), f"{where}: plan {list(info[1:4])}, expected {(flags, buckets, bits(ymin))}"
    assert info[4] == 0, where                                        # the min/max record is clear for the next user
    assert nc.float_steps(info[5:6].view(np.float32), T[0:1])[0] == 0 and nc.float_steps(info[6:7].view(np.float32), T[2:3])[0] == 0, where
    return np.nonzero(d_raw)[0], np.nonzero(d_T)[0]


def alternating(cases):
    """Small and large in turn: a context whose buffers a large case has grown runs a small one next, and back."""
    by_size = sorted(cases, key=lambda c: (c.binsum.size, c.name))
    order = []
    while by_size:
        order.append(by_size.pop(0))
        if by_size:
            order.append(by_size.pop())
    return order


def test_sizes_places_and_ends(hot, golden):
    cases = nc.all_cases() + [c for c, _ in nc.stored_cases(golden)]
    spent, flags = 0.0, set()
    for c in alternating(cases):
        f = nc.transform(c.binsum, c.m, c.ncompact, c.RDmedian, c.r)
        t0 = time.perf_counter()
        check(hot, c, f)
        spent += time.perf_counter() - t0
        flags.add(nc.plan(f.T)[0])
    assert flags == {0, 2, 8}                                         # a plan; non-finite values (degenerate); too wide a range (deep_coverage)
    print(f"{len(cases)} cases, {spent:.3f} s in the hook and the comparison")
    for c, T_ref in nc.stored_cases(golden):                          # and against the reference's own array
        raw, T, info = hot.debug_nb_transform(c.binsum, c.m, c.ncompact, c.RDmedian, c.r)
        assert np.array_equal(bits(T), bits(T_ref)), c.name


def test_the_domain_sweep(hot):
    differing = 0
    for c in nc.sweep_cases():
        a, b = check(hot, c)
        differing += a.size + b.size
    print(f"sweep: {8 << 16} inputs, {differing} differ")
    assert differing == 0                                             # test_nb_cases.py: the sweep holds no hard input


def test_the_hard_list(hot, golden):
    hard = nc.hard_cases(golden)
    differ = []
    for c, t in hard:
        a, b = check(hot, c)
        assert set(a) <= {0, 1, 2, 3, 7} and set(b) <= {3, 7}, c.name
        if a.size:
            differ.append(c.name)
    print(f"hard inputs: {len(hard)} stored, the device's float differs from libm's on {len(differ)}: {differ}")


def test_bad_arguments_leave_the_context_usable(hot):
    from rsicnv_amd import api
    c = nc.get_case("nb_8_last")
    for b, m, ncompact, r in ((c.binsum[:2], c.m, 2 * c.m, c.r), (c.binsum, c.m, 9 * c.m, c.r), (c.binsum, c.m, 8 * c.m - 1, c.r), (c.binsum, 0, 8, c.r),
                              (c.binsum, c.m, c.ncompact, 0.0)):
        with pytest.raises(api.RsiError) as err:
            hot.debug_nb_transform(b, m, ncompact, c.RDmedian, r)
        assert err.value.code == -2
    check(hot, c)
