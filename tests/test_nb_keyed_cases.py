"""CPU: the idea behind the keyed form of the NB transform (k_nb_keys) -- the transformed bins' minimum, the two 0.01 grids, their bucket
counts and the walks to the median and the MAD follow from the histogram of the bin sums -- held to the array forms with ==:
nb_keyed_cases.keyed against nb_cases.transform / nb_cases.plan / grid_restatement.pair on every case tests/test_nb_keyed.py gives the
device."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nb_keyed_cases as kc   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = kc.all_cases()


def test_the_cases_cover_what_they_claim():
    names = {c.name for c in CASES}
    assert {f"nb_{n}" for n in (8, 9, 1023, 1024, 1025, 4097)} <= names and "nb_7_no_route" in names
    forms = {c.form for c in CASES}
    assert forms == {1, 0, -1}
    for c in CASES:
        inside = c.binsum.min() >= 0 and c.binsum[3:].max(initial=0) < c.K
        route = c.K <= kc.KEY_LIMIT and c.binsum.size >= 8
        assert c.form == (-1 if not route else 1 if inside else 0), c.name
    c = next(c for c in CASES if c.name == "k_at_limit")
    assert c.K == kc.KEY_LIMIT and (c.binsum >= 16384).mean() > 0.5 and c.binsum.max() == c.K - 1 and c.binsum.min() == 0
    c = next(c for c in CASES if c.name == "all_distinct")
    assert np.unique(c.binsum).size == c.binsum.size
    c = next(c for c in CASES if c.name == "mask_one_key_whole")
    assert set(c.binsum[c.mask != 0]) == {2777} and not (c.binsum[c.mask == 0] == 2777).any()


def test_the_limit_is_the_librarys():
    ps = open(os.path.join(ROOT, "rsicnv_amd", "csrc", "pipeline_steps.h")).read()
    kh = open(os.path.join(ROOT, "rsicnv_amd", "csrc", "kernels.h")).read()
    assert "constexpr int64_t kNbKeyLimit = 1 << 15;" in ps and "constexpr int64_t kNbKeyMax = 1 << 15;" in kh
    assert kc.KEY_LIMIT == 1 << 15 and kc.gr.CAP == 1 << 20


RUN = [c for c in CASES if c.form != -1]   # the others never reach a kernel


@pytest.mark.parametrize("case", RUN, ids=[c.name for c in RUN])
def test_keyed_equals_arrays(case):
    k = kc.keyed(case.binsum, case.m, case.RDmedian, case.r, case.mask)
    T, tmin, out, rec = kc.arrays(case.binsum, case.m, case.RDmedian, case.r, case.mask)
    assert np.array_equal(k.T.view(np.uint32), T.view(np.uint32))
    assert np.float32(k.tmin).tobytes() == np.float32(tmin).tobytes() or (np.isnan(k.tmin) and np.isnan(tmin))
    assert k.records[:2] == rec
    if out is None:
        assert k.out is None and k.records[0] == kc.NONFINITE
    else:
        assert tuple(k.out) == tuple(out)


def test_the_flags_all_occur():
    seen = set()
    for c in RUN:
        k = kc.keyed(c.binsum, c.m, c.RDmedian, c.r, c.mask)
        seen.add(k.records[0])
        if c.name == "mask_moves_the_median":
            full = kc.keyed(c.binsum, c.m, c.RDmedian, c.r, None)
            assert round((k.out[0] - full.out[0]) / 0.01) >= 1      # another bucket
    assert {0, kc.EMPTY, kc.NONFINITE, kc.DEGENERATE, kc.TOO_WIDE} <= seen
