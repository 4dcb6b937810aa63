"""Inputs for filterstatus' per-level float sums alone (rsi.cpp:967-976; kernels_fs.hip) at the edges of its arithmetic: binade crossings
at chosen bins, sums that land on a power of two, ties whose order matters, several crossings in a chunk, sums that start late, stay
subnormal or overflow, values the device declines, the marked levels' compaction and queue, and one array whose float sum falls out of the
two candidate binades.  tests/test_level_sum_cases.py proves every claim on the CPU, tests/test_level_sum_edges.py runs every case on the
GPU through rsi_hot_debug_level_sums.

numpy only, seeded.  A case is a Case: name, group, claim (what it was built for, in words), T (float32 bins), status (int32), Lmax and
expect, what the case claims about itself.  expect is a dict; its keys:
  q          every value is an integer multiple of 2^q and the total is below 2^53 such units: the exact prefixes are exact in double
             whatever order the device adds them in (every case with a road)
  at         [bin, ...]: bins in which the unmarked sum changes binade (a crossing), as placed
  crossings  every bin behind the first positive unmarked one in which the unmarked sum changes binade
  rounds     True: before the first crossing of `at` and behind the last, additions round down, up and on a tie
  road       {chunk: ROAD_*}: the road the last workgroup takes for that chunk
  swap       (i, j): exchanging T[i] and T[j], two neighbours of one level, changes the bits of that level's sum
  unmarked   the float the unmarked sum ends at
  declined   True: the device declines (counts[Lmax] == -1); nothing else is specified then

Two restatements live here: the yardstick (sequential_sums / level_sums: a float32 accumulation in index order, by numpy) and an exact
model (exact_sums: Python integers, every addition rounded to 24 bits, nearest-even, from IEEE 754 and not from the kernel's step
functions).  The kernel's constants that place a case are restated below; the CPU test states the derived numbers.
"""
from collections import namedtuple
import math

import numpy as np

Case = namedtuple("Case", "name group claim T status Lmax expect")

F32 = np.float32
THREADS, PER_THREAD = 256, 8
CHUNK = THREADS * PER_THREAD          # 2048 bins: one record, one workgroup of the two first passes
BATCH = 256                           # chunk records the last workgroup takes at a time
BATCH_BINS = BATCH * CHUNK            # 524 288
QUEUE, STEP, LOAD = 512, 64, 512      # a marked level's queue (floats), entries per step, entries per load batch
LIST_CAP = 1 << 20                    # marked bins the compact list holds
MAX_L = 10400                         # Lmax the device takes
X_MAX = F32(3.0e38)                   # accepted values: 0 <= x <= X_MAX
LMAX = 99
SEAM_THREADS = (0, 1, 15, 16, 31, 32, 63, 64, 127, 128, 191, 192, 254, 255)
ROAD_SERIAL, ROAD_ONE_STEP, ROAD_STAGED = "serial", "one step", "staged"


# ---- the yardstick ------------------------------------------------------------------------------------------------------------------------
def sequential_sums(x):
    """s_0 = +0.0, s_k = fl(s_(k-1) + x_k): the running float32 sums in index order (np.add.accumulate adds one element at a time)."""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.add.accumulate(np.concatenate((np.zeros(1, dtype=F32), np.asarray(x, dtype=F32))), dtype=F32)[1:]


def loop_sums(x):
    """The same, as the reference's loop reads."""
    s, out = F32(0.0), np.empty(len(x), dtype=F32)
    with np.errstate(over="ignore", invalid="ignore"):
        for k, v in enumerate(np.asarray(x, dtype=F32)):
            s = F32(s + v)
            out[k] = s
    return out


def level_sums(T, status, Lmax):
    """What rsi_hot_debug_level_sums returns: per level (index level + Lmax) the float sum in index order and the count."""
    sums = np.zeros(2 * Lmax + 1, dtype=F32)
    counts = np.zeros(2 * Lmax + 1, dtype=np.int32)
    for l in np.unique(status):
        x = T[status == l]
        sums[l + Lmax] = sequential_sums(x)[-1]
        counts[l + Lmax] = x.size
    return sums, counts


def running_unmarked(T, status):
    """The unmarked sum behind every bin (a marked bin leaves it as it is: adding +0.0 changes no float)."""
    return sequential_sums(np.where(status == 0, T, F32(0.0)))


def declined(T):
    return not bool(((T >= 0) & (T <= X_MAX)).all())


# ---- the exact model --------------------------------------------------------------------------------------------------------------------
INF = -1
EXACT, DOWN, UP, TIE = 0, 1, 2, 3


def to_units(x, q):
    """float32 values (>= 0, finite) as Python integers n with x = n 2^q."""
    m, e = np.frexp(np.asarray(x, dtype=np.float64))
    M = (m * 16777216.0).astype(np.int64).tolist()      # 24 bits hold a float32's mantissa
    E = (e.astype(np.int64) - 24 - q).tolist()
    out = []
    for a, s in zip(M, E):
        assert a >= 0
        if a == 0:
            out.append(0)
        elif s >= 0:
            out.append(a << s)
        else:
            assert a & ((1 << -s) - 1) == 0, "not a multiple of 2^q"
            out.append(a >> -s)
    return out


def exact_sums(units, q):
    """IEEE 754 binary32 addition of non-negative numbers given in units of 2^q (q >= -149), one after the other from +0: the exact sum
    t = s + x is kept when it has at most 24 significant bits (that covers every subnormal result: the smallest unit is 2^-149), else
    its bits below the 24th are dropped and the rest goes up by one when they are more than half of its last place, or exactly half and
    it is odd; a rounded result of 2^128 or more is +inf.  Returns the sums (INF for +inf) and how each addition rounded."""
    assert q >= -149
    top = 1 << (128 - q)
    s, sums, kinds = 0, [], []
    for x in units:
        kind = EXACT
        if s != INF:
            t = s + x
            n = t.bit_length()
            if n > 24:
                sh = n - 24
                r = t & ((1 << sh) - 1)
                half = 1 << (sh - 1)
                t -= r
                if r == 0:
                    pass
                elif r < half:
                    kind = DOWN
                elif r > half:
                    kind = UP
                    t += 1 << sh
                else:
                    kind = TIE
                    if (t >> sh) & 1:
                        t += 1 << sh
            s = INF if t >= top else t
        sums.append(s)
        kinds.append(kind)
    return sums, kinds


def units_to_f32(s, q):
    return F32(np.inf) if s == INF else F32(math.ldexp(float(s), q))


def binade(s, q):
    """floor(log2) of a sum given in units of 2^q; None for zero and +inf."""
    return None if s in (0, INF) else s.bit_length() - 1 + q


# ---- the road of a chunk: k_fs_chunk_fns' candidate rule and the last workgroup's walk, restated ---------------------------------------
def is_normal(s):
    return math.isfinite(s) and s >= 2.0 ** -126


def road_of(chunk, s_in, s_out, P):
    """chunk: its index; s_in / s_out: the float sum that reaches / leaves it (as Python floats); P: the exact sum of the unmarked bins
    in front of it (double).  Chunk 0 is added serially.  A later chunk is taken in one step when the sum is a normal number at entry,
    its binade is that of 0.85 P (in double) or the one above, and it is still in that binade at the exit (values are >= 0: it never
    left); everything else is staged bin by bin."""
    if chunk == 0:
        return ROAD_SERIAL
    if not is_normal(s_in) or not P > 0.0:
        return ROAD_STAGED
    d = math.frexp(s_in)[1] - math.frexp(P * 0.85)[1]
    if d not in (0, 1):
        return ROAD_STAGED
    return ROAD_ONE_STEP if is_normal(s_out) and math.frexp(s_out)[1] == math.frexp(s_in)[1] else ROAD_STAGED


def roads_yardstick(T, status, chunks):
    """The roads of `chunks` from the yardstick's sums and double prefixes (exact for a case that states q)."""
    run = running_unmarked(T, status)
    x = np.where(status == 0, T, F32(0.0)).astype(np.float64)
    out = {}
    for c in chunks:
        s_in = float(run[c * CHUNK - 1]) if c else 0.0
        out[c] = road_of(c, s_in, float(run[min(T.size, (c + 1) * CHUNK) - 1]), float(x[:c * CHUNK].sum()))
    return out


# ---- building ------------------------------------------------------------------------------------------------------------------------
def bin_of(chunk, thread, slot):
    return chunk * CHUNK + thread * PER_THREAD + slot


def _floats(v, q):
    """Integers v (units of 2^q) as float32, exactly."""
    t64 = np.asarray(v, dtype=np.float64) * 2.0 ** q
    t = t64.astype(F32)
    assert np.array_equal(t.astype(np.float64), t64), "a value does not fit a float32"
    return t


def _sprinkle(rng, nb, keep, frac=0.01, levels=(-3, -1, 1, 2)):
    """About frac of the bins marked, none of `keep`."""
    st = np.zeros(nb, dtype=np.int32)
    k = int(nb * frac)
    if k:
        idx = rng.choice(nb, size=k, replace=False)
        st[idx] = rng.choice(np.asarray(levels, dtype=np.int32), size=k)
    st[np.asarray(sorted(keep), dtype=np.int64)] = 0
    return st


def _run_units(v, st, q):
    """The yardstick's unmarked sum behind every bin, in units of 2^q (exact integers in double)."""
    return running_unmarked(_floats(v, q), st).astype(np.float64) / 2.0 ** q


def _cross_at(v, st, q, j, top, r):
    """Give bin j the value that takes the unmarked sum from below `top` (units of 2^q, a power of two) to top + r or what that rounds to."""
    before = _run_units(v[:j], st[:j], q)[-1]
    assert before < top and st[j] == 0
    v[j] = int(top - before) + r
    return v


def _crossing_array(rng, nb, j, q, r=7, gap=3, hi=40, s0_odd=True):
    """v (units of 2^q: quarters of the sum's unit) and status: bin 0 holds the start of the sum, 2^23 units or more, every other
    unmarked bin 1 .. hi quarters, and the sum passes 2^24 units (2^26 quarters) in bin j.  With r = 0 it lands on it."""
    assert 0 < j < nb
    v = rng.integers(1, hi + 1, nb).astype(np.int64)
    st = _sprinkle(rng, nb, {0, j})
    top = 1 << 26
    before = int(v[1:j][st[1:j] == 0].sum())
    s0 = (top - before) // 4 - 8192
    s0 -= (s0 & 1) != s0_odd
    assert s0 >= 1 << 23
    v[0] = 4 * s0
    g = int(top - _run_units(v[:j], st[:j], q)[-1]) // 4          # units still missing in front of bin j
    d = g - gap
    d -= d % 2                                                    # an even shift of the start keeps every rounding as it was
    v[0] += 4 * d
    g -= d
    assert int(_run_units(v[:j], st[:j], q)[-1]) == top - 4 * g and v[0] >= 1 << 25
    v[j] = 4 * g + r
    return v, st


_cases = None


def _build():
    C = []

    def add(name, group, claim, v, st, q, Lmax=LMAX, chunks=(), **expect):
        T = _floats(v, q)
        e = dict(expect)
        e["q"] = q
        e["road"] = roads_yardstick(T, st, sorted({c for c in chunks if 0 <= c < (T.size + CHUNK - 1) // CHUNK}))
        run = running_unmarked(T, st)
        first = int(np.nonzero(run > 0)[0][0])
        ex = np.frexp(run[first:].astype(np.float64))[1]
        e["crossings"] = [int(i) + first + 1 for i in np.nonzero(np.diff(ex))[0]]
        C.append(Case(name, group, claim, T, np.asarray(st, dtype=np.int32), Lmax, e))

    rng = np.random.default_rng(0x1E7E15)
    QS = (-2, -40, 30)

    # ---- crossing: the sum passes a power of two in a chosen bin ---------------------------------------------------------------------------
    k = 0
    for thread in SEAM_THREADS:
        for slot in (0, 7):
            j = bin_of(1, thread, slot)
            q = QS[k % 3]
            k += 1
            v, st = _crossing_array(rng, 2 * CHUNK + 300, j, q)
            add(f"cross_chunk1_t{thread}_s{slot}", "crossing", f"crossing in chunk 1, thread {thread}, slot {slot}", v, st, q, chunks=(0, 1, 2),
                at=[j], rounds=True)
    for thread, slot in ((0, 7), (1, 0), (16, 7), (63, 0), (64, 7), (128, 0), (255, 7)):
        j = bin_of(0, thread, slot)
        v, st = _crossing_array(rng, CHUNK + 700, j, -2)
        add(f"cross_chunk0_t{thread}_s{slot}", "crossing", f"crossing in chunk 0 (added serially), thread {thread}, slot {slot}", v, st, -2,
            chunks=(0, 1), at=[j], rounds=thread > 1)
    nb = 2 * CHUNK + 5
    for name, j, claim in (("cross_partial_first", bin_of(2, 0, 0), "crossing in the first bin of the last, partial chunk (5 bins)"),
                           ("cross_last_bin", nb - 1, "crossing in the last bin of the array"),
                           ("cross_chunk_last_bin", 2 * CHUNK - 1, "crossing in the last bin of chunk 1"),
                           ("cross_chunk_first_bin", 2 * CHUNK, "crossing in the first bin of chunk 2")):
        v, st = _crossing_array(rng, nb, j, -2)
        add(name, "crossing", claim, v, st, -2, chunks=(1, 2), at=[j], rounds=j < nb - 5)
    nb = 258 * CHUNK + 40
    for chunk, thread, slot in ((255, 0, 0), (255, 255, 7), (256, 0, 0), (256, 64, 7), (257, 31, 0), (257, 255, 7), (258, 4, 7)):
        j = bin_of(chunk, thread, slot)
        q = QS[k % 3]
        k += 1
        v, st = _crossing_array(rng, nb, j, q, hi=24)
        last = " (the last bin of the array)" if j == nb - 1 else ""
        add(f"cross_chunk{chunk}_t{thread}_s{slot}", "crossing", f"258 chunks and 40 bins; crossing in chunk {chunk}, thread {thread}, slot {slot}{last}",
            v, st, q, chunks=(chunk - 1, chunk, chunk + 1), at=[j], rounds=j < nb - 40)

    # ---- landing: the sum reaches a power of two exactly ----------------------------------------------------------------------------------
    v = np.concatenate(([(1 << 24) - 8, 4, 4], rng.integers(1, 9, 3 * CHUNK - 3))).astype(np.int64)
    add("land_literal", "landing", "2^24 - 8, 4, 4: 16777208, 16777212, 16777216, in chunk 0; ordinary bins behind", v, np.zeros(v.size, dtype=np.int32), 0,
        chunks=(0, 1, 2), at=[2], lands=[2])
    nb = 3 * CHUNK + 9
    for name, j, zero_to, claim in (
            ("land_mid_thread", bin_of(1, 100, 3), None, "lands on 2^k in slot 3 of thread 100 of chunk 1; the thread's other bins follow"),
            ("land_thread_end", bin_of(1, 100, 7), None, "lands on 2^k in the last slot of thread 100 of chunk 1: that thread's result is 2^24 units exactly"),
            ("land_thread_end_then_zeros", bin_of(1, 31, 7), bin_of(1, 40, 0), "lands on 2^k in the last slot of thread 31; eight threads of zeros behind"),
            ("land_chunk_end", 2 * CHUNK - 1, None, "lands on 2^k in the last bin of chunk 1: the chunk's one step gives 2^24 units exactly"),
            ("land_then_zeros_to_chunk_end", bin_of(1, 7, 2), 2 * CHUNK, "lands on 2^k early in chunk 1, zeros up to its end: the one step gives 2^24 units")):
        v, st = _crossing_array(rng, nb, j, -2, r=0, gap=4)
        if zero_to is not None:
            v[j + 1:zero_to] = 0
        add(name, "landing", claim, v, st, -2, chunks=(1, 2), at=[j], lands=[j])

    # ---- order: ties that make the composition non-commutative ------------------------------------------------------------------------
    def order_array(nb, first, second, s0, cross=None, after=False):
        """Units of half the sum's unit.  The sum starts odd (s0 units in bin 0), every other bin holds 0, 2 or 4 units (exact, parity kept),
        `first` half a unit and `second` one unit: at an odd sum (half, one) gives + 2 and (one, half) + 1.  cross: a bin that takes the sum
        to 2^24 + 2 units, odd in the new unit; after: the pair and the bins behind `cross` in the new unit."""
        v = 4 * rng.integers(0, 3, nb).astype(np.int64)
        st = _sprinkle(rng, nb, {0, first, second} | ({cross} if cross is not None else set()))
        v[0] = 2 * s0
        scale = 1
        if cross is not None and after:
            v[cross + 1:] *= 2
            scale = 2
        v[first], v[second] = scale, 2 * scale
        if cross is not None:
            v = _cross_at(v, st, q=0, j=cross, top=1 << 25, r=4)
        return v, st

    k = 0
    for a, b in ((0, 1), (15, 16), (31, 32), (63, 64), (127, 128), (191, 192), (254, 255)):
        s0 = (10_000_001, (1 << 23) + 1)[k % 2]
        k += 1
        i, j = bin_of(1, a, 7), bin_of(1, b, 0)
        v, st = order_array(3 * CHUNK, i, j, s0)
        add(f"order_threads_{a}_{b}", "order", f"half a unit in the last slot of thread {a} of chunk 1, one unit in the first of thread {b}; chunk 1 is one step",
            v, st, -1, chunks=(1,), swap=(i, j))
    i, j = bin_of(1, 77, 3), bin_of(1, 77, 4)
    v, st = order_array(3 * CHUNK, i, j, 10_000_001)
    add("order_inside_thread", "order", "the pair in slots 3 and 4 of one thread", v, st, -1, chunks=(1,), swap=(i, j))
    for c, nchunks in ((1, 3), (15, 34), (31, 34), (63, 66), (255, 258), (256, 258)):
        i, j = (c + 1) * CHUNK - 1, (c + 1) * CHUNK
        v, st = order_array(nchunks * CHUNK + 3, i, j, (10_000_001, (1 << 23) + 1)[c % 2 if c > 1 else 0])
        what = "the seam of two record batches" if c == 255 else "two one-step chunks"
        add(f"order_chunks_{c}_{c + 1}", "order", f"half a unit in the last bin of chunk {c}, one unit in the first of chunk {c + 1}: {what}", v, st, -1,
            chunks=(c, c + 1), swap=(i, j))
    for a, b, tc, after in ((31, 32, 200, False), (63, 64, 130, False), (0, 1, 255, False), (63, 64, 40, True), (223, 224, 5, True), (254, 255, 253, True)):
        i, j, cross = bin_of(1, a, 7), bin_of(1, b, 0), bin_of(1, tc, 4)
        v, st = order_array(3 * CHUNK, i, j, (1 << 24) - 12001, cross=cross, after=after)
        add(f"order_staged_{a}_{b}_{'behind' if after else 'before'}_{tc}", "order",
            f"chunk 1 is staged (crossing in thread {tc}); the pair at the seam of threads {a} and {b}, {'behind' if after else 'in front of'} the crossing",
            v, st, -1, chunks=(1,), at=[cross], swap=(i, j))

    # ---- several -------------------------------------------------------------------------------------------------------------------------
    def big_behind(v, lo, hi, top_quarters):
        v[lo:hi] = rng.integers(1, top_quarters + 1, hi - lo)
        return v

    j1, j2 = bin_of(1, 50, 2), bin_of(1, 200, 5)
    v, st = _crossing_array(rng, 3 * CHUNK, j1, -2)
    v = big_behind(v, j1 + 1, v.size, 90000)
    st[j2] = 0
    v = _cross_at(v, st, -2, j2, 1 << 27, 24)
    add("two_crossings_in_a_chunk", "several", "the sum passes 2^k in thread 50 and 2^(k+1) in thread 200 of chunk 1", v, st, -2, chunks=(1, 2), at=[j1, j2])
    j = bin_of(1, 100, 3)
    v, st = _crossing_array(rng, 3 * CHUNK, 3 * CHUNK - 1, -2)
    v[j] = 4 << 27
    v = big_behind(v, j + 1, v.size, 1024)
    add("lift_by_four_binades", "several", "one value of 2^27 units lifts the sum from below 2^24 units to above 2^27 in the middle of chunk 1", v, st, -2,
        chunks=(1, 2), at=[j])
    j1, j2 = bin_of(1, 128, 0), bin_of(3, 9, 7)
    v, st = _crossing_array(rng, 4 * CHUNK + 100, j1, -2)
    v = big_behind(v, j1 + 1, v.size, 48000)
    st[2 * CHUNK:3 * CHUNK] = rng.choice(np.array([-2, 1], dtype=np.int32), CHUNK)
    st[j2] = 0
    v = _cross_at(v, st, -2, j2, 1 << 27, 24)
    add("marked_chunk_between_crossings", "several", "chunks 1 and 3 each hold a crossing, chunk 2 holds no unmarked bin", v, st, -2, chunks=(1, 2, 3, 4),
        at=[j1, j2])
    for kk in (1, 2):
        nb = (kk + 1) * CHUNK + 40
        v = rng.integers(1, 41, nb).astype(np.int64)
        st = _sprinkle(rng, nb, ())
        st[:kk * CHUNK] = rng.choice(np.array([-1, 1, 3], dtype=np.int32), kk * CHUNK)
        st[kk * CHUNK] = 0
        v[kk * CHUNK] = 4 * ((1 << 24) - 3001)
        add(f"first_unmarked_at_{kk * CHUNK}", "several", f"the first unmarked bin is bin {kk * CHUNK}; the sum passes 2^24 units in that chunk", v, st, -2,
            chunks=tuple(range(kk + 2)))
    nb = 2 * CHUNK + 77
    v = rng.integers(1, 41, nb).astype(np.int64)
    st = rng.choice(np.array([-2, -1, 1], dtype=np.int32), nb)
    st[-1] = 0
    add("first_unmarked_is_last_bin", "several", "the only unmarked bin is the last bin of the array", v, st, -2, chunks=(0, 1, 2), unmarked=float(_floats(v[-1:], -2)[0]))

    # ---- start ------------------------------------------------------------------------------------------------------------------------------
    def raw(name, group, claim, T, st, Lmax=LMAX, **expect):
        C.append(Case(name, group, claim, np.asarray(T, dtype=F32), np.asarray(st, dtype=np.int32), Lmax, dict(expect)))

    nb = 3 * CHUNK
    st = _sprinkle(rng, nb, ())
    raw("all_plus_zero", "start", "every unmarked bin is +0.0", np.where(st == 0, F32(0.0), F32(3.5)), st, unmarked=0.0)
    raw("all_minus_zero", "start", "every bin is -0.0: every sum is +0.0 (the sums start at +0.0)", np.full(nb, -0.0, dtype=F32), st, unmarked=0.0, plus_zero=True)
    tiny = float(np.finfo(F32).smallest_subnormal)
    sub = (rng.integers(0, 4, nb) * tiny).astype(F32)
    raw("stays_subnormal", "start", "every unmarked bin is 0 .. 3 units of 2^-149: the sum stays subnormal through three chunks", sub, st, q=-149, subnormal_end=True)
    sub = (rng.integers(2000, 4001, nb) * tiny).astype(F32)
    raw("subnormal_to_normal_in_chunk_1", "start", "subnormal bins whose sum becomes a normal number in chunk 1 and passes 2^-125 in chunk 2", sub, st, q=-149,
        normal_from_chunk=1)
    for nb in (1, 8, 2047, 2048, 2049):
        v = rng.integers(1, 41, nb).astype(np.int64)
        v[0] = 4 * ((1 << 24) - 2 * nb - 1)
        s = _sprinkle(rng, nb, {0}, frac=0.05)
        raw(f"nb_{nb}", "start", f"{nb} bins", _floats(v, -2), s, q=-2)

    # ---- overflow and declines ----------------------------------------------------------------------------------------------------------
    ordinary = _floats(rng.integers(1, 41, 3 * CHUNK), -2)
    st = _sprinkle(rng, 3 * CHUNK, {0, 1, 2, CHUNK + 900, CHUNK + 901})
    T = ordinary.copy()
    T[:3] = (X_MAX, X_MAX, 1.0)
    raw("overflow_in_chunk_0", "overflow", "3.0e38, 3.0e38, 1, ...: +inf from bin 1 on", T, st, unmarked=float("inf"))
    T = ordinary.copy()
    T[0] = X_MAX
    T[CHUNK + 900] = X_MAX
    raw("overflow_in_chunk_1", "overflow", "3.0e38 in bin 0 and again in chunk 1: +inf there, ordinary bins behind", T, st, unmarked=float("inf"))
    T = ordinary.copy()
    T[CHUNK + 900] = X_MAX
    st2 = st.copy()
    st2[5] = -2
    T[5] = X_MAX
    raw("x_max_accepted", "overflow", "a bin of exactly float32(3.0e38), unmarked and marked, is accepted", T, st2, accepted=True)
    bad = (("above_x_max", np.nextafter(X_MAX, F32(np.inf))), ("nan", F32(np.nan)), ("plus_inf", F32(np.inf)), ("negative", F32(-1.0)))
    for name, x in bad:
        for where, level in (("unmarked", 0), ("marked", -2)):
            T = ordinary.copy()
            s = st.copy()
            T[CHUNK + 901] = x
            s[CHUNK + 901] = level
            raw(f"decline_{name}_{where}", "overflow", f"{name} in a{'n un' if level == 0 else ' '}marked bin: the device declines", T, s, declined=True)

    # ---- marked: the ordered compaction and the per-wave queue --------------------------------------------------------------------------------
    def level_values(n):
        """A level's values in units of a quarter: the first starts the sum odd just above 2^23 units, the others are 1 .. 40 quarters."""
        x = rng.integers(1, 41, n).astype(np.int64)
        x[0] = 4 * ((1 << 23) + 1 + 2 * int(rng.integers(0, 1000)))
        return x

    def find_swap(T, st, level):
        """Two neighbours of `level` (not its first bin) whose exchange changes the level's sum."""
        idx = np.nonzero(st == level)[0]
        base = sequential_sums(T[idx])[-1]
        for k in range(1, idx.size - 1):
            x = T[idx].copy()
            x[k], x[k + 1] = x[k + 1], x[k]
            if sequential_sums(x)[-1].view(np.uint32) != base.view(np.uint32):
                return int(idx[k]), int(idx[k + 1])
        return None

    def marked_case(name, claim, nb, entries, Lmax=LMAX, unmarked=True, swap_level=None):
        """entries: the compact list's levels in order.  The marked bins lie in a window around bin 2048 (or over the whole array when it
        is small), so they cross thread seams and the seam of chunks 0 and 1 with 0 .. 8 of them per thread."""
        entries = np.asarray(entries, dtype=np.int32)
        M = entries.size
        if unmarked:
            lo = max(0, CHUNK - M) if nb >= CHUNK + M + 16 else 0
            width = min(nb - lo, 2 * M + 16)
            pos = lo + np.sort(rng.choice(width, size=M, replace=False))
        else:
            assert M == nb
            pos = np.arange(nb)
        st = np.zeros(nb, dtype=np.int32)
        st[pos] = entries
        v = rng.integers(1, 41, nb).astype(np.int64)
        for l in np.unique(st):
            idx = np.nonzero(st == l)[0]
            v[idx] = level_values(idx.size)
        T = _floats(v, -2)
        e = {}
        if swap_level is not None:
            e["swap"] = find_swap(T, st, swap_level)
            assert e["swap"] is not None, name
            e["swap_level"] = swap_level
        e["marked"] = M
        e["q"] = -2
        C.append(Case(name, "marked", claim, T, st, Lmax, e))

    for n in (1, 63, 64, 65, 448, 449, 511, 512, 513, 1024, 1025):
        marked_case(f"marked_alone_{n}", f"one marked level of {n} bins: {n} entries in the list", 3 * CHUNK, np.full(n, -7), swap_level=-7 if n >= 63 else None)
    counts = {-40: 1, 3: 63, -3: 64, 5: 65, -5: 448, 8: 449, -8: 512, 13: 513, -13: 1025}
    entries = rng.permutation(np.concatenate([np.full(n, l) for l, n in counts.items()]))
    for l in (8, -8, -13):
        marked_case(f"marked_mixed_level_{l}", f"levels of 1, 63, 64, 65, 448, 449, 512, 513 and 1025 bins in random order; the exchange is in level {l}",
                    5 * CHUNK, entries, swap_level=l)
    entries = np.concatenate((np.full(64, 4), np.full(64, -9), np.full(200, 4)))
    entries[64 + 3] = 4                      # one entry of the other level inside the step, so that -9 is not the whole step either
    marked_case("marked_inside_one_step", "level -9 lies in entries 64 .. 127 of the list, one 64-entry step", 2 * CHUNK, entries, swap_level=-9)
    entries = np.tile(np.array([6, -6], dtype=np.int32), 300)
    marked_case("marked_interleaved", "levels 6 and -6 take the list's entries in turn, lane by lane", 2 * CHUNK, entries, swap_level=-6)
    marked_case("marked_interleaved_other", "levels 6 and -6 take the list's entries in turn; the exchange is in level 6", 2 * CHUNK, entries, swap_level=6)
    for L in (1, 2, 99, MAX_L):
        levels = sorted({-L, -1, 1, L})
        entries = rng.permutation(np.concatenate([np.full(70 + 3 * i, l) for i, l in enumerate(levels)]))
        marked_case(f"marked_lmax_{L}", f"Lmax = {L}: levels {levels}", 2 * CHUNK + 1, entries, Lmax=L, swap_level=-L)
        marked_case(f"marked_lmax_{L}_top", f"Lmax = {L}: levels {levels}; the exchange is in level {L}", 2 * CHUNK + 1, entries, Lmax=L, swap_level=L)
    entries = rng.choice(np.array([-2, -1, 1, 2], dtype=np.int32), 5000)
    marked_case("no_unmarked_bin", "every bin is marked: the unmarked level holds 0 bins and +0.0", 5000, entries, unmarked=False, swap_level=2)
    return C


PREMISE_ONES = 23_000_000
PREMISE_TAIL = (2.0, 3.0, 5.0, 1.0)
PREMISE_EXPECT = dict(q=0, unmarked=16777224.0, misfit_from_chunk=11084, chunks=11231)


def premise_case():
    """The one large case, built on demand: 2^24, 23 000 000 ones, then 2, 3, 5, 1, all unmarked.  The float sum stays at 2^24 over the
    ones while the exact prefix grows: from some chunk on neither candidate binade of 0.85 P holds the sum."""
    T = np.ones(1 + PREMISE_ONES + len(PREMISE_TAIL), dtype=F32)
    T[0] = F32(2.0 ** 24)
    T[-len(PREMISE_TAIL):] = PREMISE_TAIL
    return Case("premise", "premise", "the float sum stays at 2^24 while 0.85 P passes 2^25: neither candidate binade fits from chunk 11 084 on", T,
                np.zeros(T.size, dtype=np.int32), LMAX, dict(PREMISE_EXPECT))


def all_cases():
    """Every case but premise."""
    global _cases
    if _cases is None:
        _cases = _build()
        assert len({c.name for c in _cases}) == len(_cases)
    return _cases


def get_case(name):
    return next(c for c in all_cases() if c.name == name)
