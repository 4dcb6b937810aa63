"""GPU: `rsicnv depth` on the device.  The hooks against the numpy restatement of depth_cases: the summary and the
65536-bin distribution at every length and value class, a negative depth refused; window lines at every W that takes another
path (below, at and above a workgroup's span, at and around n) and across a forced slice seam; region records and lines for
empty, clipped, outside, overlapping, duplicate and unsorted regions, 3000 of them, and lists that shrink and grow on one
context; means on rounding ties and of 2^31 - 1; coordinates of 1 to 10 digits; BGZF equal to text; launch counts."""
import gzip

import numpy as np
import pytest

import depth_cases as dc

pytestmark = pytest.mark.gpu

VALUES = dc.value_cases()
BGZF_EOF = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])


@pytest.fixture(scope="module")
def hot(hotlib):
    from rsicnv_amd import api
    h = api.RsiHot(0)
    yield h
    h.close()


def check_summary(hot, d, span):
    rec, bins = hot.debug_depth_summary(d, span=span)
    want = dc.summary(d)
    assert {k: int(rec[k]) for k in want} == want
    assert np.array_equal(bins, dc.dist(d) if len(d) else np.zeros(dc.BINS, dtype=np.int64))
    return rec


@pytest.mark.parametrize("name", list(VALUES))
def test_summary_values(hot, name):
    d = VALUES[name]
    check_summary(hot, d, dc.SPAN)
    assert hot.depth_stats()["workgroups"] == -(-d.size // dc.SPAN) and hot.depth_stats()["launches"] == 1
    check_summary(hot, d, 0)            # the default span: one workgroup
    check_summary(hot, d[1:], 333)      # three workgroups in four start off a 16-byte boundary
    p, n = hot.loaded_depth()
    assert n == d.size - 1 and p


def test_summary_lengths(hot):
    rng = np.random.default_rng(11)
    for n in dc.LENGTHS:
        d = rng.poisson(30, n).astype(np.int32)
        if n > 2:
            d[-1] = 70000               # the last value counts, and above the cap
        check_summary(hot, d, dc.SPAN)
        assert hot.depth_stats()["launches"] == (1 if n else 0)


def test_same_bytes_twice(hot):
    d = VALUES["around_65535"]
    a = hot.debug_depth_summary(d, span=64)
    b = hot.debug_depth_summary(d, span=64)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_negative_depth_is_refused(hot):
    from rsicnv_amd import api
    for at in (0, 700, dc.SPAN, 3 * dc.SPAN + 16):
        d = VALUES["poisson_30"].copy()
        d[at] = -1
        with pytest.raises(api.RsiError) as e:
            hot.debug_depth_summary(d, span=dc.SPAN)
        assert api.STATUS_NAMES[e.value.code] == "RSI_ERR_BAD_ARG" and "negative depth" in str(e.value)
        assert int(hot.last_depth_summary["negative"]) == 1 and int(hot.last_depth_summary["sum"]) == 0
    d = np.full(300, -(1 << 31), dtype=np.int32)    # nothing but negative depths: nothing is indexed
    with pytest.raises(api.RsiError):
        hot.debug_depth_summary(d, span=64)
    assert int(hot.last_depth_summary["negative"]) == 300
    check_summary(hot, VALUES["poisson_30"], dc.SPAN)   # and the next call counts from zero


# ---------------------------------------------------------------------------------------------------------------------
# windows
# ---------------------------------------------------------------------------------------------------------------------

def window_lines(hot, d, W, **kw):
    text, st = hot.debug_region_track(d, "chr7", W=W, **kw)
    return text.decode(), st


@pytest.mark.parametrize("name", ["poisson_30", "int32_max_beside_0", "all_zero", "runs"])
def test_windows(hot, name):
    d = VALUES[name]
    n = d.size
    for W in (1, 2, 3, 64, 101, 500, dc.WSPAN - 1, dc.WSPAN, dc.WSPAN + 1, 2 * dc.WSPAN + 37, n - 1, n, n + 1):
        got, st = window_lines(hot, d, W, span=dc.WSPAN)
        assert got == dc.window_text("chr7", d, W), (name, W)
        assert st["lines"] == len(dc.windows(n, W)) and st["slices"] == 1
    for W in (1, 7, 500, 4096, 5000):                      # the default span, which W = 5000 exceeds
        d2 = np.tile(d, 4)[:3 * 4096 + 5]
        assert window_lines(hot, d2, W)[0] == dc.window_text("chr7", d2, W), (name, W)


def test_window_lengths(hot):
    rng = np.random.default_rng(12)
    for n in dc.LENGTHS:
        d = rng.poisson(30, n).astype(np.int32)
        for W in (1, 3, 64, 500):
            got, st = window_lines(hot, d, W, span=dc.WSPAN)
            assert got == dc.window_text("chr7", d, W), (n, W)
            assert st["slices"] == (1 if n else 0)


def test_window_slice_seams(hot):
    d = VALUES["poisson_30"]
    for W, slice_lines in ((3, 100), (101, 7), (500, 1), (64, 13)):
        got, st = window_lines(hot, d, W, span=dc.WSPAN, slice_lines=slice_lines)
        nwin = len(dc.windows(d.size, W))
        assert got == dc.window_text("chr7", d, W), (W, slice_lines)
        assert st["slices"] == -(-nwin // slice_lines) and st["lines"] == nwin


# ---------------------------------------------------------------------------------------------------------------------
# regions
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("values", ["poisson_30", "int32_max_beside_0"])
def test_regions(hot, values):
    d = VALUES[values]
    for name, regions in dc.region_cases(d.size).items():
        for tile in (dc.TILE, 0):
            got = hot.debug_depth_regions(d, [r[0] for r in regions], [r[1] for r in regions], tile=tile)
            assert [dc.record_of(r) for r in got] == [dc.region_record(d, s, e) for s, e in regions], (name, tile)
        text, st = hot.debug_region_track(d, "1", start=[r[0] for r in regions], end=[r[1] for r in regions], tile=dc.TILE)
        assert text.decode() == dc.region_text("1", d, regions), name
        assert st["lines"] == len(regions)


def test_region_lists_shrink_and_grow_on_one_context(hot):
    d = VALUES["poisson_30"]
    big = dc.region_cases(d.size)["batch_3000"]
    want = [dc.region_record(d, s, e) for s, e in big]
    for regions, expect in ((big, want), (big[5:7], want[5:7]), (big, want), ([], [])):
        got = hot.debug_depth_regions(d, [r[0] for r in regions], [r[1] for r in regions], tile=dc.TILE)
        assert [dc.record_of(r) for r in got] == expect
    text, st = hot.debug_region_track(d, "1", start=[r[0] for r in big], end=[r[1] for r in big], tile=dc.TILE, slice_lines=700)
    assert text.decode() == dc.region_text("1", d, big) and st["slices"] == 5


def test_regions_of_an_empty_array(hot):
    got = hot.debug_depth_regions(np.zeros(0, dtype=np.int32), [0, -5], [10, 5])
    assert [dc.record_of(r) for r in got] == [(0, 0, 0, 0)] * 2
    text, _ = hot.debug_region_track(np.zeros(0, dtype=np.int32), "1", start=[0, -5], end=[10, 5])
    assert text.decode() == "1\t0\t10\t0.00\n1\t-5\t5\t0.00\n"


# ---------------------------------------------------------------------------------------------------------------------
# text
# ---------------------------------------------------------------------------------------------------------------------

def test_means_on_rounding_ties(hot):
    for d, W, mean in dc.TIES:
        assert dc.fixed2(int(d.astype(np.int64).sum()), W) == mean
        assert window_lines(hot, d, W)[0] == f"chr7\t0\t{W}\t{mean}\n"
        text, _ = hot.debug_region_track(d, "chr7", start=[0], end=[W])
        assert text.decode() == f"chr7\t0\t{W}\t{mean}\n"


def test_coordinates_of_1_to_10_digits(hot):
    d = VALUES["poisson_30"][:300]
    for digits in range(1, 11):
        pos0 = 10 ** digits - 150                      # the lines' coordinates pass from `digits` to digits + 1 digits
        got, _ = window_lines(hot, d, 50, pos0=pos0)
        assert got == dc.window_text("chr7", d, 50, pos0=pos0)
        regions = [(0, 9), (100, 200), (149, 151), (299, 300)]
        text, _ = hot.debug_region_track(d, "chr7", start=[r[0] for r in regions], end=[r[1] for r in regions], pos0=pos0)
        assert text.decode() == dc.region_text("chr7", d, regions, pos0=pos0)
    assert window_lines(hot, d[:5], 2, pos0=0)[0] == dc.window_text("chr7", d[:5], 2)


def test_bgzf_equals_text(hot):
    d = VALUES["poisson_30"]
    for kw in (dict(W=3, span=dc.WSPAN), dict(W=3, span=dc.WSPAN, slice_lines=400),
               dict(start=[0, 5, -3], end=[100, 3000, 4], tile=dc.TILE)):
        plain, _ = hot.debug_region_track(d, "chrX", **kw)
        packed, st = hot.debug_region_track(d, "chrX", format="bgzf", **kw)
        assert packed[:4] == b"\x1f\x8b\x08\x04" and gzip.decompress(packed + BGZF_EOF) == plain
        assert hot.deflate_stats()["text_bytes"] == len(plain) and hot.deflate_stats()["members"] >= st["slices"]


def test_launch_counts_do_not_depend_on_the_list(hot):
    d = VALUES["poisson_30"]
    counts = []
    for W in (1, 500, d.size):
        window_lines(hot, d, W, span=dc.WSPAN)
        counts.append(hot.depth_stats()["launches"])
    assert counts == [6, 6, 6]
    big = dc.region_cases(d.size)["batch_3000"]
    counts = []
    for regions in (big[:1], big):
        hot.debug_depth_regions(d, [r[0] for r in regions], [r[1] for r in regions], tile=dc.TILE)
        a = hot.depth_stats()["launches"]
        hot.debug_region_track(d, "1", start=[r[0] for r in regions], end=[r[1] for r in regions], tile=dc.TILE)
        counts.append((a, hot.depth_stats()["launches"]))
    assert counts == [(2, 6), (2, 6)]
    hot.debug_depth_regions(d, [], [])
    assert hot.depth_stats()["launches"] == 0


def test_bad_arguments(hot):
    from rsicnv_amd import api
    d = VALUES["poisson_30"][:100]
    for kw in (dict(W=5, span=4097), dict(W=-1), dict(start=[(1 << 62) + 1], end=[5])):
        with pytest.raises(api.RsiError) as e:
            hot.debug_region_track(d, "1", **kw)
        assert api.STATUS_NAMES[e.value.code] == "RSI_ERR_BAD_ARG"
    with pytest.raises(api.RsiError):
        hot.debug_region_track(d, "a\tb", W=5)
