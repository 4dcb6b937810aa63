"""GPU: the per-bin track writer through its test hook (rsi_hot_debug_bin_track), byte for byte against the restatement
(tests/bin_track_restatement.py), with the statistics' lines and bytes.  The shapes are the smallest at which each pass can go
wrong: the edges of the count tile (256 bins) and of the line tile (256 pieces), a break one base either side of a bin edge at
a tile boundary and at the last bin, a bin in m pieces, every slice length around a tile, the widest values and coordinates."""
import ctypes as C

import numpy as np
import pytest

import bin_track_restatement as bt
from test_bin_track_restatement import RATIO_TABLE

pytestmark = pytest.mark.gpu

BAD_ARG = -2
INT32_MAX = 2**31 - 1


@pytest.fixture(scope="module")
def hot():
    from rsicnv_amd import api
    h = api.RsiHot(0)
    yield h
    h.close()


def pairs_from_breaks(breaks, widths):
    """Regions that cut the compacted array at the positions `breaks` (increasing), region k removing widths[k] bases."""
    pairs, cum = [], 0
    for c, w in zip(breaks, widths):
        pairs.append((c + cum, c + cum + w - 1))
        cum += w
    return pairs


def values_for(nb, seed=1):
    return np.random.default_rng(seed).integers(0, 120, size=nb).astype(np.int32)


def check(hot, values, m, n, pairs, median2=60, which=0, name="chr1", slice_bins=0, by="mask", slices=None):
    values = np.asarray(values, dtype=np.int32)
    exp = bt.text(values, m, n, pairs, median2, which, name, by=by)
    got, st = hot.debug_bin_track(values, m, n, pairs, median2, which, name, slice_bins)
    assert got == exp, (got[:300], exp[:300])
    assert st["n"] == values.size and st["lines"] == exp.count(b"\n") and st["bytes"] == len(exp)
    if slices is not None:
        assert st["slices"] == slices
    return exp


# ---- the count tile's edges, without regions ----

@pytest.mark.parametrize("nb", [1, 2, 255, 256, 257])
@pytest.mark.parametrize("which", [0, 1])
def test_bins_without_regions(hot, nb, which):
    exp = check(hot, values_for(nb), 3, nb * 3, [], which=which, slices=1)
    assert exp.count(b"\n") == nb


# ---- bin sizes ----

@pytest.mark.parametrize("m", [1, 2, 3, 101])
def test_bin_sizes(hot, m):
    nb = 300
    breaks = [0, 1, m, 2 * m + 1, 7 * m - 1, 256 * m, 256 * m + 1, 299 * m, 300 * m]
    breaks = sorted(set(breaks))
    pairs = pairs_from_breaks(breaks, [3 + k for k in range(len(breaks))])
    n = nb * m + sum(e - s + 1 for s, e in pairs)
    for which in (0, 1):
        check(hot, values_for(nb, m), m, n, pairs, which=which)


def test_m1_with_a_removed_base_between_every_two_kept(hot):
    nb = 300                                   # kept 0 2 4 ...: every bin borders a break, none is cut
    pairs = [(2 * i + 1, 2 * i + 1) for i in range(nb - 1)]
    exp = check(hot, values_for(nb), 1, 2 * nb - 1, pairs)
    assert exp.count(b"\n") == nb


# ---- a break d compacted positions from a bin boundary ----

@pytest.mark.parametrize("d", [-1, 0, 1])
@pytest.mark.parametrize("edge", ["tiles_0_1", "last_bin_start", "last_bin_end"])
def test_break_beside_a_bin_boundary(hot, edge, d):
    nb, m = 300, 5
    c = {"tiles_0_1": 256 * m, "last_bin_start": (nb - 1) * m, "last_bin_end": nb * m}[edge] + d
    pairs = pairs_from_breaks([c], [5])
    n = nb * m + 5 + 2                         # a tail of two bases: the break behind the last bin's end lies in it
    exp = check(hot, values_for(nb), m, n, pairs)
    cut = d != 0 and not (edge == "last_bin_end" and d == 1)
    assert exp.count(b"\n") == nb + (1 if cut else 0)


# ---- many pieces ----

@pytest.mark.parametrize("m", [7, 101])
def test_one_bin_in_m_pieces(hot, m):
    pairs = [(2 * i + 1, 2 * i + 1) for i in range(m - 1)]      # bin 0: m single bases
    n = 2 * m - 1 + 2 * m                                         # two plain bins behind it
    exp = check(hot, [5, 6, 7], m, n, pairs)
    assert exp.count(b"\n") == m + 2
    check(hot, [5], m, 2 * m - 1, pairs, which=1)                 # ... and with nothing else


@pytest.mark.parametrize("npieces", [255, 256, 257, 513])
def test_pieces_at_the_line_tile_edges(hot, npieces):
    nb, m = 200, 4
    inner = [b * m + j for b in range(nb) for j in (1, 2, 3)]     # every position strictly inside a bin
    breaks = sorted(inner[:npieces - nb])
    pairs = pairs_from_breaks(breaks, [2] * len(breaks))
    exp = check(hot, values_for(nb), m, nb * m + 2 * len(breaks), pairs, slices=1)
    assert exp.count(b"\n") == npieces


# ---- the chromosome's ends and the tail ----

@pytest.mark.parametrize("tail", [0, 1, 6])
@pytest.mark.parametrize("ends", ["from_0", "to_end", "both"])
def test_regions_at_the_ends_and_tails(hot, ends, tail):
    nb, m = 40, 7
    kept = nb * m + tail
    head = 11 if ends in ("from_0", "both") else 0
    back = 13 if ends in ("to_end", "both") else 0
    n = head + kept + back
    pairs = ([(0, head - 1)] if head else []) + ([(n - back, n - 1)] if back else [])
    exp = check(hot, values_for(nb), m, n, pairs)
    assert exp.count(b"\n") == nb
    assert exp.splitlines()[0].split(b"\t")[1] == b"%d" % head
    assert int(exp.splitlines()[-1].split(b"\t")[2]) == head + nb * m


# ---- region counts ----

@pytest.mark.parametrize("nreg", [0, 1, 2, 127, 128, 129])
def test_region_counts(hot, nreg):
    m = 11
    pairs = [(50 + 37 * k, 50 + 37 * k + 4) for k in range(nreg)]
    n = 50 + 37 * 130 + 200
    nb = (n - 5 * nreg) // m
    check(hot, values_for(nb, nreg), m, n, pairs)


def test_4096_regions(hot):
    n, m = 600_000, 101
    pairs = [(100 + 130 * k, 109 + 130 * k) for k in range(4096)]
    nb = (n - 40960) // m
    for which in (0, 1):
        check(hot, values_for(nb), m, n, pairs, which=which)
    from rsicnv_amd import api
    with pytest.raises(api.RsiError) as ei:
        hot.debug_bin_track([1], m, n + 130, pairs + [(100 + 130 * 4096, 109 + 130 * 4096)], 60, 0, "c")
    assert ei.value.code == BAD_ARG


# ---- slices ----

@pytest.fixture(scope="module")
def sliced_case():
    rng = np.random.default_rng(0x511CE)
    nb, m = 1500, 5
    breaks = np.sort(rng.choice(nb * m, size=nb // 3, replace=False))
    pairs = pairs_from_breaks([int(c) for c in breaks], [int(w) for w in rng.integers(1, 9, size=breaks.size)])
    n = nb * m + sum(e - s + 1 for s, e in pairs) + 3
    values = rng.integers(0, 90, size=nb).astype(np.int32)
    return values, m, n, pairs, {w: bt.text(values, m, n, pairs, 61, w, "chrS") for w in (0, 1)}


@pytest.mark.parametrize("slice_bins", [0, 1, 2, 255, 256, 257, 1000])
def test_slice_lengths_give_the_same_text(hot, sliced_case, slice_bins):
    values, m, n, pairs, exp = sliced_case
    for which in (0, 1):
        got, st = hot.debug_bin_track(values, m, n, pairs, 61, which, "chrS", slice_bins)
        assert got == exp[which]
        assert st["slices"] == (1 if slice_bins == 0 else -(-values.size // slice_bins))
        assert st["lines"] == exp[which].count(b"\n") and st["bytes"] == len(exp[which])


# ---- digits ----

def test_value_digits_of_median(hot):
    values = [0, 9] + [10**k for k in range(1, 10)] + [10**k - 1 for k in range(2, 10)] + [INT32_MAX]
    exp = check(hot, values, 2, 2 * len(values), [])
    assert exp.splitlines()[-1] == b"chr1\t%d\t%d\t2147483647" % (2 * len(values) - 2, 2 * len(values))


def test_ratio_rounding_table(hot):
    for v, m2, text in RATIO_TABLE:
        got, _ = hot.debug_bin_track([v, v], 3, 7, [], m2, 1, "c")
        assert got == b"c\t0\t3\t" + text + b"\nc\t3\t6\t" + text + b"\n", (v, m2)
    check(hot, [v for v, _, _ in RATIO_TABLE] + list(range(0, 200)), 3, 3 * (len(RATIO_TABLE) + 200) + 1, [], median2=61, which=1)


def test_ten_digit_coordinates(hot):
    pairs = [(0, 1_999_999_999)]
    for which in (0, 1):
        exp = check(hot, [3, 1000, 7], 100, 2_000_000_300, pairs, which=which, by="intervals")
        assert exp.startswith(b"chr1\t2000000000\t2000000100\t")
    check(hot, [3, 1000], 100, 2_000_000_300, pairs + [(2_000_000_050, 2_000_000_059)], by="intervals")


# ---- names, refusals, the empty track, a short buffer ----

def test_names(hot):
    check(hot, [1, 2, 3], 2, 7, [(2, 2)], name="c")
    check(hot, [1, 2, 3], 2, 7, [(2, 2)], name="N" * 255, which=1)
    check(hot, [1, 2, 3], 2, 7, [(2, 2)], name="chr 1 with blanks")


@pytest.mark.parametrize("kw", [
    dict(name=""), dict(name="N" * 256), dict(name="a\tb"), dict(name="a\n"),
    dict(which=2), dict(which=-1),
    dict(which=1, median2=0),
    dict(pairs=[(2, 3), (4, 5)]),              # touching
    dict(pairs=[(5, 6), (1, 2)]),              # unsorted
    dict(pairs=[(3, 2)]),                      # empty
    dict(pairs=[(8, 10)]),                     # beyond n - 1
    dict(pairs=[(-1, 2)]),
    dict(values=[1, 2, 3, 4]),                 # nb m above the kept bases
    dict(values=[1, 2, 3], pairs=[(4, 5)]),
    dict(m=0),
])
def test_bad_arguments(hot, kw):
    from rsicnv_amd import api
    a = dict(values=[1, 2, 3], m=3, n=10, pairs=[], median2=60, which=0, name="c")
    a.update(kw)
    with pytest.raises(api.RsiError) as ei:
        hot.debug_bin_track(a["values"], a["m"], a["n"], a["pairs"], a["median2"], a["which"], a["name"])
    assert ei.value.code == BAD_ARG
    check(hot, [1, 2, 3], 3, 10, [])            # the context goes on


def test_median_ignores_the_chromosome_median(hot):
    check(hot, [1, 2, 3], 3, 10, [], median2=0, which=0)


def test_no_bins_is_ok_and_empty(hot):
    for which in (0, 1):
        got, st = hot.debug_bin_track([], 3, 2, [], 60, which, "c")
        assert got == b"" and st["n"] == 0 and st["lines"] == 0 and st["bytes"] == 0 and st["slices"] == 0
    got, st = hot.debug_bin_track([], 3, 10, [(0, 9)], 60, 0, "c")       # nothing kept
    assert got == b""


def test_short_buffer_returns_the_length_and_writes_nothing(hot):
    from rsicnv_amd import api
    values = np.array([4, 5, 6], dtype=np.int32)
    exp = bt.text(values, 3, 10, [], 0, 0, "c")
    st = api.RsiTrackStats()
    out = np.full(len(exp) + 8, 0x55, dtype=np.uint8)
    call = lambda buf, cap: hot.lib.rsi_hot_debug_bin_track(hot.ctx, values.ctypes.data, 3, 3, 10, None, 0, 0, 0, b"c", 0, buf, cap, C.byref(st))
    assert call(out.ctypes.data, len(exp) - 1) == len(exp) and (out == 0x55).all()
    assert call(None, 0) == len(exp)
    assert call(out.ctypes.data, len(exp)) == len(exp) and out[:len(exp)].tobytes() == exp and (out[len(exp):] == 0x55).all()


# ---- random cases ----

@pytest.mark.parametrize("seed", range(20))
def test_random_cases(hot, seed):
    rng = np.random.default_rng(0xB1A0 + seed)
    m = int(rng.choice([1, 2, 3, 5, 11, 101]))
    nb = int(rng.integers(1, 5001))
    nbreaks = int(rng.integers(0, min(nb * m, 4096) + 1)) if seed % 4 else int(rng.integers(0, 20))
    breaks = np.sort(rng.choice(nb * m + 1, size=nbreaks, replace=False))
    widths = rng.integers(1, 40, size=nbreaks)
    pairs = pairs_from_breaks([int(c) for c in breaks], [int(w) for w in widths])
    tail = int(rng.integers(0, m))
    n = nb * m + int(widths.sum()) + (0 if nbreaks and breaks[-1] == nb * m else tail)
    values = rng.integers(0, [3, 200, 70000, INT32_MAX][seed % 4], size=nb, dtype=np.int64).astype(np.int32)
    which = seed % 2
    median2 = int(rng.integers(1, 300))
    slice_bins = int(rng.choice([0, 0, 300, 1024]))
    exp = check(hot, values, m, n, pairs, median2=median2, which=which, name="chr%d" % seed, slice_bins=slice_bins)
    bt.check_valid(exp, n, pairs)
