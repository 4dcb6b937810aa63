"""GPU: the depth-track writer (kernels_track.hip, track.hip) through rsi_hot_debug_track, byte for byte against the numpy
restatement (tests/track_restatement.py).  The shapes are the smallest at which each pass can go wrong: one tile and its
edges, run boundaries at tile edges, runs across slice boundaries, every digit count of values and coordinates."""
import ctypes as C

import numpy as np
import pytest

import track_restatement as tr

pytestmark = pytest.mark.gpu

I32_MAX, I32_MIN = 2**31 - 1, -2**31
BAD_ARG = -2


@pytest.fixture(scope="module")
def hot():
    from rsicnv_amd import api
    h = api.RsiHot(0)
    yield h
    h.close()


def check(hot, v, name="chrT", pos0=0, slice_bases=0):
    v = np.asarray(v, dtype=np.int32)
    got, st = hot.debug_track(v, name, pos0=pos0, slice_bases=slice_bases)
    exp = tr.text(v, name, pos0)
    assert got == exp, (got[:200], exp[:200])
    assert st["n"] == v.size and st["lines"] == exp.count(b"\n") and st["bytes"] == len(exp)
    return got, st


def alternating(n):
    return (np.arange(n) & 1).astype(np.int32) * 7


# ---- tiny arrays ----

@pytest.mark.parametrize("v", [[4], [4, 4], [4, 5]], ids=["n1", "n2_equal", "n2_different"])
def test_one_and_two_bases(hot, v):
    got, st = check(hot, v)
    assert st["lines"] == len(set(v))


@pytest.mark.parametrize("n", [255, 256, 257])
def test_one_run_around_a_tile(hot, n):
    _, st = check(hot, np.full(n, 31))
    assert st["lines"] == 1


@pytest.mark.parametrize("n", [255, 256, 257])
def test_every_base_a_line_around_a_tile(hot, n):
    _, st = check(hot, alternating(n))
    assert st["lines"] == n


# ---- run boundaries at tile edges ----

@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("d", [-1, 0, 1])
def test_boundary_at_a_tile_edge(hot, k, d):
    v = np.full(1000, 3, dtype=np.int32)
    v[256 * k + d:] = 8
    _, st = check(hot, v)
    assert st["lines"] == 2


def test_boundaries_at_every_edge_of_three_tiles(hot):
    v = np.zeros(1000, dtype=np.int32)
    for j, b in enumerate(sorted(256 * k + d for k in (1, 2, 3) for d in (-1, 0, 1))):
        v[b:] = j + 1
    _, st = check(hot, v)
    assert st["lines"] == 10


@pytest.mark.parametrize("n", [256, 257, 700])
def test_single_changed_value_at_either_end(hot, n):
    v = np.full(n, 12, dtype=np.int32)
    v[n - 1] = 13
    assert check(hot, v)[1]["lines"] == 2
    v = np.full(n, 12, dtype=np.int32)
    v[0] = 13
    assert check(hot, v)[1]["lines"] == 2


# ---- slices: 1024 bases on n = 5000, boundaries at 1024, 2048, 3072, 4096 ----

def slice_cases():
    n = 5000
    long_run = (np.arange(n) % 5).astype(np.int32)
    long_run[1000:3100] = 77                              # starts before the first boundary, ends after the third
    ends_at = np.zeros(n, dtype=np.int32)
    for j, b in enumerate((1024, 2048, 3072, 4096)):      # runs that end exactly at a boundary
        ends_at[b:] = j + 1
    ends_at[1020:1024] = 50                               # ... a short one too
    different = np.arange(n, dtype=np.int32)              # every base its own line, across every boundary
    one_run = np.full(n, 6, dtype=np.int32)               # a run that spans every slice
    near = np.zeros(n, dtype=np.int32)
    near[1023] = 1; near[2048] = 2; near[3071:3073] = 3; near[4999] = 4   # single bases just before, at and across boundaries
    return {"long_run": long_run, "ends_at_boundary": ends_at, "all_different": different, "one_run": one_run, "near": near}


@pytest.mark.parametrize("case", list(slice_cases()))
def test_runs_across_slice_boundaries(hot, case):
    v = slice_cases()[case]
    sliced, st = check(hot, v, slice_bases=1024)
    assert st["slices"] == 5
    whole, st0 = check(hot, v, slice_bases=0)
    assert st0["slices"] == 1 and sliced == whole
    if case == "long_run":
        assert b"chrT\t1000\t3100\t77\n" in sliced       # ONE line
    if case == "one_run":
        assert sliced == b"chrT\t0\t5000\t6\n"


@pytest.mark.parametrize("slice_bases", [1, 255, 1000, 4999, 5000, 5001])
def test_slice_lengths_that_are_no_multiple_of_the_tile(hot, slice_bases):
    v = slice_cases()["long_run"]
    assert check(hot, v, slice_bases=slice_bases)[0] == tr.text(v, "chrT")


# ---- digits ----

def test_value_digits(hot):
    v = [0, 9]
    for k in range(1, 10):
        v += [10**k, 10**(k + 1) - 1 if k < 9 else I32_MAX]
    v += [-1, -9, -10, -99, -100, -999999999, -1000000000, I32_MIN, I32_MAX, I32_MIN]
    assert 999999999 in v and 1000000000 in v
    got, _ = check(hot, v)
    assert b"\t-2147483648\n" in got and b"\t2147483647\n" in got


def test_coordinate_digits_from_zero(hot):
    n = 100002
    v = np.zeros(n, dtype=np.int32)
    for k in range(1, 6):                                 # boundaries at 9|10, 99|100, ..., 99999|100000 and one base either side
        p = 10**k
        v[p - 2:p + 2] = [1, 2, 3, 4]
    got, _ = check(hot, v)
    assert b"chrT\t99999\t100000\t2\nchrT\t100000\t100001\t3\n" in got


@pytest.mark.parametrize("pos0", [2147483000, 9999999990, 999999999999999990, -40])
def test_coordinate_digits_with_an_offset(hot, pos0):
    v = (np.arange(64) // 3).astype(np.int32)             # 10-, 11- and 19-digit coordinates (and negative ones) without a large array
    check(hot, v, pos0=pos0)
    check(hot, v, pos0=pos0, slice_bases=16)


# ---- names ----

@pytest.mark.parametrize("name", [b"c", b"N" * 255, b"chr 1|x"], ids=["1_byte", "255_bytes", "blank_inside"])
def test_names(hot, name):
    v = alternating(600)
    check(hot, v, name=name)
    check(hot, v, name=name, slice_bases=256)


@pytest.mark.parametrize("name", [b"", b"chr\t1", b"chr1\n", b"N" * 256], ids=["empty", "tab", "newline", "256_bytes"])
def test_bad_names_are_rejected(hot, name):
    from rsicnv_amd import api
    with pytest.raises(api.RsiError) as ei:
        hot.debug_track([1, 2, 3], name)
    assert ei.value.code == BAD_ARG


def test_empty_array_writes_nothing(hot):
    got, st = hot.debug_track(np.zeros(0, dtype=np.int32), "chrT")
    assert got == b"" and st["lines"] == 0 and st["bytes"] == 0


# ---- seeded random arrays ----

def random_runs(n, mean, seed):
    rng = np.random.default_rng(seed)
    lens = rng.geometric(1.0 / mean, size=int(n / mean * 1.5) + 64)
    vals = rng.integers(0, 3, size=lens.size)
    v = np.repeat(vals, lens)[:n].astype(np.int32)
    assert v.size == n
    return v


@pytest.fixture(scope="module")
def random_cases():
    return {mean: (v, tr.text(v, "chr7")) for mean in (3, 3000) for v in [random_runs(300_000, mean, 0x7AC + mean)]}


@pytest.mark.parametrize("slice_bases", [0, 65536])
@pytest.mark.parametrize("mean", [3, 3000])
def test_random_runs(hot, random_cases, mean, slice_bases):
    v, exp = random_cases[mean]
    got, st = hot.debug_track(v, "chr7", slice_bases=slice_bases)
    assert got == exp
    assert st["lines"] == exp.count(b"\n")
    assert st["bytes"] == len(exp)
    assert st["slices"] == (1 if slice_bases == 0 else -(-v.size // slice_bases))


# ---- the return value ----

def test_return_value_without_room(hot):
    v = np.ascontiguousarray(slice_cases()["long_run"])
    exp = tr.text(v, "chrT")
    lib = hot.lib
    assert lib.rsi_hot_debug_track(hot.ctx, v.ctypes.data, v.size, b"chrT", 0, 0, None, 0, None) == len(exp)
    assert lib.rsi_hot_debug_track(hot.ctx, v.ctypes.data, v.size, b"chrT", 0, 1024, None, 1 << 30, None) == len(exp)
    guard = 64
    buf = np.full(len(exp) + guard, 0xA5, dtype=np.uint8)
    assert lib.rsi_hot_debug_track(hot.ctx, v.ctypes.data, v.size, b"chrT", 0, 0, buf.ctypes.data, len(exp) - 1, None) == len(exp)
    assert np.all(buf == 0xA5)                            # one byte too small: nothing written, in front of the guard or in it
    assert lib.rsi_hot_debug_track(hot.ctx, v.ctypes.data, v.size, b"chrT", 0, 0, buf.ctypes.data, len(exp), None) == len(exp)
    assert buf[:len(exp)].tobytes() == exp and np.all(buf[len(exp):] == 0xA5)
