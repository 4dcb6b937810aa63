"""CPU: the cases of tests/level_sum_cases.py are what they say they are.  The yardstick (numpy's float32 accumulation) against an explicit
loop and against the exact integer model on every case, and every claim of every `expect` proved from the two restatements, never from the
library: where the sum changes binade, how the additions round on both sides of a crossing, that exchanging two neighbours changes the
bits, the road the last workgroup takes, and that the prefixes the roads rest on are exact in double."""
import math
from fractions import Fraction

import numpy as np
import pytest

import level_sum_cases as lc

F32 = np.float32


def test_the_restated_constants_and_what_follows_from_them():
    assert lc.CHUNK == 2048 and lc.BATCH_BINS == 524288
    assert lc.QUEUE == 512 and lc.QUEUE - lc.STEP == 448          # a queue of more than 448 entries is drained before the next step
    assert lc.LOAD == 8 * lc.STEP
    assert (2 * lc.MAX_L + 1) * 4 == 83204                        # k_fs_chunk_fns' dynamic LDS at the largest Lmax: 81 KB
    assert -(-(2 * lc.MAX_L + 1) // 4) * 4 - (2 * lc.MAX_L + 1) == 3   # the last level workgroup: one wave with a level, three idle
    assert -(-(2 * 1 + 1) // 4) * 4 - (2 * 1 + 1) == 1                 # Lmax = 1: one idle wave
    assert float(lc.X_MAX) * 2 > float(np.finfo(F32).max)         # two accepted values can overflow
    assert lc.bin_of(1, 255, 7) == 2 * lc.CHUNK - 1


def test_the_exact_model_rounds_as_ieee_says():
    # 2^24 + 1 is a tie and goes to the even 2^24; 2^24 + 2 + 1 is a tie and goes up to the even 2^24 + 4
    s, k = lc.exact_sums([1 << 24, 1, 2, 1], 0)
    assert s == [1 << 24, 1 << 24, (1 << 24) + 2, (1 << 24) + 4] and k == [lc.EXACT, lc.TIE, lc.EXACT, lc.TIE]
    # from 2^25 the last place is 4: + 1 goes down, + 3 goes up, + 2 is a tie that goes up from the odd 2^25 + 4 and stays at the even 2^25 + 8
    s, k = lc.exact_sums([1 << 25, 1, 3, 2, 2, 4], 0)
    assert s == [1 << 25, 1 << 25, (1 << 25) + 4, (1 << 25) + 8, (1 << 25) + 8, (1 << 25) + 12]
    assert k == [lc.EXACT, lc.DOWN, lc.UP, lc.TIE, lc.TIE, lc.EXACT]
    # subnormals add exactly; the largest finite float plus half its last place is a tie that goes up: +inf; a little less stays
    assert lc.exact_sums([3, 5, (1 << 23) - 8], -149)[0] == [3, 8, 1 << 23]
    big = ((1 << 24) - 1) << 253
    assert lc.exact_sums([big, 1 << 252], -149)[0] == [big, lc.INF]
    assert lc.exact_sums([big, (1 << 252) - 1], -149)[0] == [big, big]
    # against Fractions, rounded by comparison of distances
    rng = np.random.default_rng(5)
    x = (rng.integers(1, 1 << 24, 300) * 2.0 ** rng.integers(-20, 20, 300)).astype(F32)
    sums, _ = lc.exact_sums(lc.to_units(x, -60), -60)
    s = Fraction(0)
    for v, got in zip(x, sums):
        t = s + Fraction(float(v))
        e = math.frexp(float(t))[1]
        e -= Fraction(2) ** (e - 1) > t                                   # floor(log2 t) + 1, whatever the conversion to double did
        ulp = Fraction(2) ** (e - 24)
        lo = (t // ulp) * ulp
        s = lo if t - lo < ulp / 2 or (t - lo == ulp / 2 and (lo / ulp) % 2 == 0) else lo + ulp
        assert Fraction(got) * Fraction(2) ** -60 == s


def _unmarked(c):
    return c.T[c.status == 0]


def _model(c, q):
    """The exact model over the case's whole array (a marked bin adds nothing): sums and kinds per bin."""
    units = lc.to_units(np.where(c.status == 0, c.T, F32(0.0)), q)
    return units, *lc.exact_sums(units, q)


@pytest.fixture(scope="module")
def models():
    cache = {}

    def get(c):
        if c.name not in cache:
            cache[c.name] = _model(c, c.expect["q"])
        return cache[c.name]
    return get


ACCEPTED = [c for c in lc.all_cases() if not c.expect.get("declined")]


@pytest.mark.parametrize("c", ACCEPTED, ids=lambda c: c.name)
def test_yardstick_is_the_loop_and_the_exact_model(c, models):
    for l in np.unique(c.status):
        x = c.T[c.status == l]
        y = lc.sequential_sums(x)
        assert np.array_equal(y.view(np.uint32), lc.loop_sums(x).view(np.uint32))
        q = c.expect.get("q", -149)
        if l == 0 and "road" in c.expect:                                 # the model's run over the whole array, shared with the road test
            full = models(c)[1]
            sums = [full[i] for i in np.nonzero(c.status == 0)[0]]
        else:
            sums, _ = lc.exact_sums(lc.to_units(np.abs(x), q), q)         # abs: -0.0 is 0 to the model, whose sums start at +0 like the loop's
        m = np.array([lc.units_to_f32(s, q) for s in sums], dtype=F32)
        assert np.array_equal(y.view(np.uint32), m.view(np.uint32)), (c.name, int(l))
    s, n = lc.level_sums(c.T, c.status, c.Lmax)
    assert n.sum() == c.T.size and not lc.declined(c.T)
    assert int(np.abs(c.status).max()) <= c.Lmax <= lc.MAX_L and int(np.count_nonzero(c.status)) <= lc.LIST_CAP


@pytest.mark.parametrize("c", [c for c in lc.all_cases() if c.expect.get("declined")], ids=lambda c: c.name)
def test_declined_cases_hold_one_value_the_device_cannot_take(c):
    bad = ~((c.T >= 0) & (c.T <= lc.X_MAX))
    assert bad.sum() == 1 and lc.declined(c.T)
    assert ("unmarked" in c.name) == (c.status[bad][0] == 0)


ROAD = [c for c in lc.all_cases() if "road" in c.expect]


@pytest.mark.parametrize("c", ROAD, ids=lambda c: c.name)
def test_crossings_roundings_and_roads(c, models):
    e, q = c.expect, c.expect["q"]
    units, sums, kinds = models(c)
    # the prefixes do not depend on the device's order of summation
    assert sum(units) < 1 << 53
    # where the sum changes binade
    first = next(i for i, s in enumerate(sums) if s != 0)
    cross = [i for i in range(first + 1, len(sums)) if lc.binade(sums[i], q) != lc.binade(sums[i - 1], q)]
    assert cross == e["crossings"]
    at = e.get("at", [])
    assert set(at) <= set(cross)
    for j in e.get("lands", []):
        assert sums[j] == 1 << (sums[j].bit_length() - 1) and j in cross
    if c.group == "crossing":
        assert cross == at and sums[at[0]] != 1 << (sums[at[0]].bit_length() - 1)
    if e.get("rounds"):
        for part in (kinds[first + 1:at[0]], kinds[at[-1] + 1:]):
            assert all(part.count(k) > 0 for k in (lc.DOWN, lc.UP, lc.TIE)), (c.name, [part.count(k) for k in range(4)])
    if "unmarked" in e:
        assert float(lc.units_to_f32(sums[-1], q)) == e["unmarked"]
    # the roads, from the model's sums and the integer prefixes
    nchunks = (c.T.size + lc.CHUNK - 1) // lc.CHUNK
    for ch, road in e["road"].items():
        s_in = float(lc.units_to_f32(sums[ch * lc.CHUNK - 1], q)) if ch else 0.0
        s_out = float(lc.units_to_f32(sums[min(c.T.size, (ch + 1) * lc.CHUNK) - 1], q))
        P = math.ldexp(float(sum(units[:ch * lc.CHUNK])), q)
        assert lc.road_of(ch, s_in, s_out, P) == road, (c.name, ch)
        assert ch < nchunks
    for j in at:
        assert e["road"][j // lc.CHUNK] == (lc.ROAD_SERIAL if j < lc.CHUNK else lc.ROAD_STAGED)
    if c.group == "crossing":
        j = at[0]
        for ch in (j // lc.CHUNK - 1, j // lc.CHUNK + 1):
            if 0 < ch < nchunks:
                assert e["road"][ch] == lc.ROAD_ONE_STEP, (c.name, ch)
    if c.group == "order":
        i, j = e["swap"]
        if not at:
            assert {e["road"][i // lc.CHUNK], e["road"][j // lc.CHUNK]} == {lc.ROAD_ONE_STEP}
        else:
            assert i // lc.CHUNK == j // lc.CHUNK == at[0] // lc.CHUNK and ((i < at[0]) == (j < at[0]))


def test_the_placed_cases_are_where_the_issue_puts_them():
    names = {c.name for c in lc.all_cases()}
    for t in lc.SEAM_THREADS:
        for s in (0, 7):
            assert lc.get_case(f"cross_chunk1_t{t}_s{s}").expect["at"] == [lc.bin_of(1, t, s)]
    c = lc.get_case("cross_chunk255_t255_s7")
    assert c.expect["at"] == [lc.BATCH_BINS - 1] and c.T.size == 258 * lc.CHUNK + 40            # the last bin of the first record batch
    assert lc.get_case("cross_chunk256_t0_s0").expect["at"] == [lc.BATCH_BINS]
    assert lc.get_case("cross_chunk258_t4_s7").expect["at"] == [c.T.size - 1]
    assert lc.get_case("cross_partial_first").T.size == 2 * lc.CHUNK + 5
    assert lc.get_case("order_chunks_255_256").expect["swap"] == (lc.BATCH_BINS - 1, lc.BATCH_BINS)
    assert np.array_equal(lc.get_case("land_literal").T[:3], np.array([16777208, 4, 4], dtype=F32))
    assert np.array_equal(lc.sequential_sums(lc.get_case("land_literal").T[:3]), np.array([16777208, 16777212, 16777216], dtype=F32))
    e = lc.get_case("two_crossings_in_a_chunk").expect
    assert [j // lc.CHUNK for j in e["at"]] == [1, 1] and e["at"][0] // 8 != e["at"][1] // 8
    c = lc.get_case("lift_by_four_binades")
    run = lc.running_unmarked(c.T, c.status)
    j = c.expect["at"][0]
    assert math.frexp(float(run[j]))[1] - math.frexp(float(run[j - 1]))[1] >= 3
    c = lc.get_case("marked_chunk_between_crossings")
    assert [j // lc.CHUNK for j in c.expect["at"]] == [1, 3] and np.all(c.status[2 * lc.CHUNK:3 * lc.CHUNK] != 0)
    for k in (1, 2):
        c = lc.get_case(f"first_unmarked_at_{k * lc.CHUNK}")
        assert int(np.nonzero(c.status == 0)[0][0]) == k * lc.CHUNK and c.expect["crossings"] and c.expect["crossings"][0] // lc.CHUNK == k
    c = lc.get_case("first_unmarked_is_last_bin")
    assert list(np.nonzero(c.status == 0)[0]) == [c.T.size - 1]
    assert {f"nb_{n}" for n in (1, 8, 2047, 2048, 2049)} <= names
    assert all(lc.get_case(f"nb_{n}").T.size == n for n in (1, 8, 2047, 2048, 2049))


def test_start_cases():
    c = lc.get_case("all_plus_zero")
    assert not _unmarked(c).any() and not np.signbit(_unmarked(c)).any()
    c = lc.get_case("all_minus_zero")
    assert np.signbit(c.T).all()
    s, _ = lc.level_sums(c.T, c.status, c.Lmax)
    assert not s.any() and not np.signbit(s).any()
    tiny = float(np.finfo(F32).tiny)
    c = lc.get_case("stays_subnormal")
    s, _ = lc.level_sums(c.T, c.status, c.Lmax)
    assert 0 < s[c.Lmax] < tiny and (_unmarked(c) < tiny).all()
    c = lc.get_case("subnormal_to_normal_in_chunk_1")
    run = lc.running_unmarked(c.T, c.status)
    assert (c.T < tiny).all() and run[lc.CHUNK - 1] < tiny <= run[2 * lc.CHUNK - 1]
    units, sums, kinds = _model(c, -149)
    assert sums[2 * lc.CHUNK - 1] < 1 << 24 < sums[-1] and any(k != lc.EXACT for k in kinds[2 * lc.CHUNK:])   # rounding starts in chunk 2


def test_overflow_cases():
    for name, chunk in (("overflow_in_chunk_0", 0), ("overflow_in_chunk_1", 1)):
        c = lc.get_case(name)
        run = lc.running_unmarked(c.T, c.status)
        first = int(np.nonzero(np.isinf(run))[0][0])
        assert first // lc.CHUNK == chunk and first < c.T.size - lc.CHUNK and np.isfinite(c.T).all()
        units, sums, _ = _model(c, -149)
        assert sums[first - 1] != lc.INF and sums[first] == lc.INF
    c = lc.get_case("x_max_accepted")
    assert (c.T == lc.X_MAX).sum() == 2 and set(c.status[c.T == lc.X_MAX]) == {0, -2}
    assert np.isfinite(lc.level_sums(c.T, c.status, c.Lmax)[0]).all()


MARKED = [c for c in lc.all_cases() if "swap" in c.expect]


@pytest.mark.parametrize("c", MARKED, ids=lambda c: c.name)
def test_an_exchange_of_two_neighbours_changes_the_bits(c):
    """By the exact model, not the yardstick that chose the pair."""
    i, j = c.expect["swap"]
    l = int(c.status[i])
    assert i < j and c.status[j] == l == c.expect.get("swap_level", 0)
    idx = np.nonzero(c.status == l)[0]
    k = int(np.searchsorted(idx, i))
    assert idx[k] == i and idx[k + 1] == j                                  # neighbours inside the level
    x = c.T[idx]
    q = c.expect.get("q", -2)
    a = lc.exact_sums(lc.to_units(x, q), q)[0][-1]
    x[k], x[k + 1] = x[k + 1], x[k]
    b = lc.exact_sums(lc.to_units(x, q), q)[0][-1]
    assert a != b
    if c.group == "order":
        assert abs(a - b) == 2 * (2 if "staged" in c.name else 1)           # one unit of the sum at the end, in halves of the first unit


def test_marked_cases_reach_the_queue_and_list_edges():
    def count(name, level):
        c = lc.get_case(name)
        return int((c.status == level).sum()), int(np.count_nonzero(c.status))
    for n in (1, 63, 64, 65, 448, 449, 511, 512, 513, 1024, 1025):
        assert count(f"marked_alone_{n}", -7) == (n, n)
    c = lc.get_case("marked_mixed_level_8")
    assert sorted(int((c.status == l).sum()) for l in np.unique(c.status) if l) == [1, 63, 64, 65, 448, 449, 512, 513, 1025]
    for name in ("marked_alone_1025", "marked_mixed_level_8", "marked_lmax_99"):
        c = lc.get_case(name)
        pos = np.nonzero(c.status)[0]
        per_thread = np.bincount(pos // lc.PER_THREAD)
        assert pos[0] < lc.CHUNK <= pos[-1] and per_thread.max() >= 6 and len(set(per_thread[pos[0] // 8:])) >= 5   # both chunks, threads with few and many
    c = lc.get_case("marked_inside_one_step")
    entry = np.nonzero(c.status[np.nonzero(c.status)[0]] == -9)[0]
    assert entry.min() >= lc.STEP and entry.max() < 2 * lc.STEP and entry.size == lc.STEP - 1
    c = lc.get_case("marked_interleaved")
    lv = c.status[np.nonzero(c.status)[0]]
    assert np.array_equal(lv[0::2], np.full(300, 6)) and np.array_equal(lv[1::2], np.full(300, -6))
    for L in (1, 2, 99, lc.MAX_L):
        c = lc.get_case(f"marked_lmax_{L}")
        assert c.Lmax == L and set(np.unique(c.status)) == {-L, -1, 0, 1, L}
    c = lc.get_case("no_unmarked_bin")
    assert c.status.all() and lc.level_sums(c.T, c.status, c.Lmax)[1][c.Lmax] == 0


def test_premise_analytically():
    """Without building the array: 2^24 + 1 is a tie that stays at the even 2^24, so the sum is a fixed point over the ones; the last four
    bins take it to 16777224; and the restated candidate rule loses the sum's binade where 0.85 P reaches 2^25."""
    e = lc.PREMISE_EXPECT
    sums, kinds = lc.exact_sums([1 << 24, 1, 1], 0)
    assert sums == [1 << 24] * 3 and kinds[1:] == [lc.TIE, lc.TIE]
    sums, _ = lc.exact_sums([1 << 24] + [int(x) for x in lc.PREMISE_TAIL], 0)
    assert sums[-1] == 16777224 == int(e["unmarked"])
    nb = 1 + lc.PREMISE_ONES + len(lc.PREMISE_TAIL)
    assert (nb + lc.CHUNK - 1) // lc.CHUNK == e["chunks"]
    assert (1 << 24) + lc.PREMISE_ONES + 11 < 1 << 53

    def P(i):                       # the exact prefix in front of bin i >= 1 (within the ones)
        return float((1 << 24) + i - 1)
    lo, hi = 1, lc.PREMISE_ONES     # the first bin whose prefix times 0.85, in double, is 2^25 or more (monotone)
    while lo < hi:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if P(mid) * 0.85 >= 2.0 ** 25 else (mid + 1, hi)
    assert lo == 22698588 and -(-lo // lc.CHUNK) == e["misfit_from_chunk"]
    for ch, road in ((1, lc.ROAD_ONE_STEP), (e["misfit_from_chunk"] - 1, lc.ROAD_ONE_STEP), (e["misfit_from_chunk"], lc.ROAD_STAGED),
                     (e["chunks"] - 1, lc.ROAD_STAGED)):
        assert lc.road_of(ch, 2.0 ** 24, 2.0 ** 24, P(ch * lc.CHUNK)) == road
    # a level far beyond 2^22 bins: the 15 % argument does not hold here, and the walk must not need it
    assert lc.PREMISE_ONES > 1 << 22 and 2.0 ** 24 < 0.85 * P(lc.PREMISE_ONES) / 1.15
