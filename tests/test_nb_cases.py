"""CPU: the cases of tests/nb_cases.py are what they claim to be, and the restatement of the NB transform they are judged by equals the
compiled reference's answers (golden/nb_edges.npz) bit for bit on the cases built from a depth array.  Nothing here touches the library's
device code.  The restatement evaluates sqrt and log with Python's math module, the machine's libm: the one the reference links."""
import math
import os
import re
import struct

import numpy as np
import pytest

import nb_cases as nc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "nb_edges.npz")
F32 = np.float32


def bits(x):
    return np.asarray(x, dtype=np.float32).view(np.int32)


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def restated():
    return {c.name: nc.transform(c.binsum, c.m, c.ncompact, c.RDmedian, c.r) for c in nc.all_cases()}


def test_the_constants_are_the_librarys():
    assert (nc.THREADS, nc.PER_BLOCK, nc.GRID_CAP, nc.HARD_D) == (256, 1024, 512, 8)
    kb = open(os.path.join(ROOT, "rsicnv_amd", "csrc", "kernels_bin.hip")).read()
    assert "constexpr int kThreads = 256;" in kb and "constexpr int kMaxGrid = 256 * 2;" in kb
    assert "int grid = grid_for(nb, kThreads * 4);" in kb and re.search(r"k_nb_scale_mm, dim3\(bounded_grid\(nb, kThreads \* 4, 512\)\)", kb)
    assert [nc.grid(n) for n in (3, 1024, 1025, 131073, 523264, 523265, 524289)] == [1, 1, 2, 129, 511, 512, 512]


def test_restatement_equals_the_reference(golden):
    stored = nc.stored_cases(golden)
    assert [c.name for c, _ in stored] == ["rd_poisson_30", "rd_gampois_40", "rd_poisson_8", "rd_gampois_100", "rd_three_bins"]
    sizes = []
    for c, T_ref in stored:
        assert c.binsum.size == T_ref.size == c.expect["rd"].size // c.m <= 2300 and c.m <= 31, c.name
        assert c.RDmedian * 2 == int(c.RDmedian * 2) and np.isfinite(T_ref).all(), c.name        # a 0.01-grid median of integers
        f = nc.transform(c.binsum, c.m, c.ncompact, c.RDmedian, c.r)
        assert np.array_equal(bits(f.T), bits(T_ref)), (c.name, np.nonzero(bits(f.T) != bits(T_ref))[0][:8])
        assert not f.hard_T.any(), c.name                                                       # the stored answers hang on no midpoint
        sizes.append(c.binsum.size)
    assert min(sizes) == 3 and {c.ncompact % c.m == 0 for c, _ in stored} == {True, False}
    c, _ = stored[0]
    f = nc.transform(c.binsum, c.m, c.ncompact, c.RDmedian, c.r)
    assert (c.binsum[40:43] == 0).all() and list(np.nonzero(f.raw == f.tmin)[0]) == [40, 41, 42] and (f.T[40:43] == 0).all()


def test_sizes_and_where_the_minimum_sits(restated):
    seen = {}
    for c in nc.all_cases():
        if c.group != "sizes":
            continue
        nb, f = c.binsum.size, restated[c.name]
        assert c.ncompact // c.m == nb and (nb - 1) * c.m + c.m - 1 <= c.ncompact - 1, c.name     # whole bins: the i2 clamp never fires
        bins, place = c.expect["min_bins"], c.expect["place"]
        assert list(np.nonzero(f.raw == f.tmin)[0]) == bins and np.isfinite(f.T).all(), c.name
        g = nc.grid(nb)
        if place == "last_workgroup":
            assert bins[0] // nc.THREADS == g - 1 and 3 <= bins[0] < nb - 1, c.name
        if place == "second_stride":
            assert bins[0] >= g * nc.THREADS and bins[0] < nb - 1, c.name                        # no thread's first bin
        if place == "several":
            assert len(bins) >= 3, c.name
        if place in ("bin0", "bin1", "bin2"):
            b = bins[0]
            assert f.T[b] != 0 and bits(f.T[b]) == bits(f.T[:3])[b], c.name                       # counted in the minimum, then overwritten
        else:
            assert (f.T[[b for b in bins if b > 2]] == 0).all(), c.name
        assert bits(f.t0) == bits(f.T[0]) and bits(f.t2) == bits(f.T[2]) and f.T[2] == F32(c.RDmedian), c.name
        assert not f.hard_T.any(), c.name
        assert np.unique(c.binsum).size <= 3001, c.name                                         # the expected array is a table lookup
        seen.setdefault(nb, set()).add(place)
    assert tuple(sorted(seen)) == nc.SIZES == (3, 4, 8, 255, 256, 257, 1023, 1024, 1025, 131071, 131072, 131073, 524287, 524288, 524289)
    for lo, hi in ((3, 1025), (131071, 131073), (524287, 524289)):
        got = set().union(*(p for nb, p in seen.items() if lo <= nb <= hi))
        assert got == set(nc.PLACES), (lo, got)
    assert seen[3] == {"bin0", "bin1", "bin2", "last"} and "second_stride" in seen[1023] and "second_stride" in seen[1025]
    rem = {(c.ncompact % c.m == 0) for c in nc.all_cases() if c.group == "sizes"}
    assert rem == {True, False}


def test_sums_and_r_at_their_ends(restated):
    c = nc.get_case("zero_sum_bin")
    f = restated[c.name]
    assert c.binsum[333] == 0 and list(np.nonzero(f.raw == f.tmin)[0]) == [333] and f.T[333] == 0
    c = nc.get_case("deep_coverage")
    assert c.binsum.max() == (1 << 31) * 101 - 1 and c.binsum.min() > (1 << 30) * 101 and np.isfinite(restated[c.name].T).all()
    assert all(float(int(s)) == int(s) for s in c.binsum)                                       # exact as doubles
    assert nc.get_case("r_one").r == 1.0 and nc.get_case("r_million").r == 999999.5
    for name in ("r_one", "r_million", "deep_coverage"):
        T = restated[name].T
        assert np.isfinite(T).all() and T[3:].min() == 0 and T.max() > 0, name


def test_the_degenerate_case_has_no_median_level_to_divide_by(restated):
    c = nc.get_case("degenerate")
    f = restated[c.name]
    dele, med, dup = f.levels
    assert struct.unpack("<q", struct.pack("<d", med))[0] & ((1 << 29) - 1) == 0              # the double is a float ...
    assert med == float(f.tmin) and c.RDmedian * c.m == c.binsum[0]                            # ... the minimum: med_nbt = 0
    assert np.isnan(f.T[3:]).all() and f.T[0] == -np.inf and f.T[1] == np.inf and np.isnan(f.T[2])
    assert nc.plan(f.T) == (2, 0, F32(0)) and not f.hard_raw.any()


def test_hard_inputs_are_too_rare_to_hide_anything():
    """Every sum 0 .. 2^16 - 1 at eight (RDmedian, MAD, m): at most one input in a million may claim the one-step exemption (3e-8 expected)."""
    cases = nc.sweep_cases()
    assert len(cases) == 8 and all((2 * med).is_integer() and (2 * mad).is_integer() for med, mad, _ in nc.SWEEP)
    hard = total = 0
    for c in cases:
        assert np.array_equal(c.binsum, np.arange(1 << 16))
        for s in range(nc.SWEEP_SUMS):
            hard += nc.is_hard(nc.nbt(float(s), float(c.m), c.r))
        total += nc.SWEEP_SUMS
    assert total == 8 << 16 and hard * 10 ** 6 <= total, hard
    t = nc.nbt(3000.0, 101.0, 7.5)
    mid = struct.unpack("<d", struct.pack("<q", (struct.unpack("<q", struct.pack("<d", t))[0] & ~((1 << 29) - 1)) | (1 << 28)))[0]
    ulp = math.ulp(mid)
    assert nc.is_hard(mid) and nc.is_hard(mid + 8 * ulp) and nc.is_hard(mid - 8 * ulp) and not nc.is_hard(mid + 9 * ulp) and not nc.is_hard(mid - 9 * ulp)
    assert F32(mid - ulp) != F32(mid + ulp)                                                      # the float changes across the midpoint


def test_the_hard_list(golden):
    hard = nc.hard_cases(golden)
    assert 20 <= len(hard) <= 64 and int(golden["hard_found"][0]) >= len(hard)
    side = []
    for c, t in hard:
        total = int(c.binsum[3])
        assert c.m == 101 and 5.0 <= c.RDmedian <= 100.0 and 0 < total < 1 << 16 and c.r >= 1.0, c.name
        mine = nc.nbt(float(total), 101.0, c.r)
        assert mine == t and nc.is_hard(t), c.name                                              # the stored answer is this libm's
        side.append((struct.unpack("<q", struct.pack("<d", t))[0] & ((1 << 29) - 1)) - (1 << 28))
        f = nc.transform(c.binsum, c.m, c.ncompact, c.RDmedian, c.r)
        assert list(np.nonzero(f.raw == f.tmin)[0]) == [4] and c.binsum[4] == 0 and not f.hard_raw[4], c.name    # the known minimum is not hard
        assert list(np.nonzero(f.hard_raw)[0]) == c.expect["hard_bins"] and list(np.nonzero(f.hard_T)[0]) == [3, 7], c.name
    assert min(side) < 0 < max(side) and max(abs(s) for s in side) <= nc.HARD_D
