"""GPU: the tabix index of a BGZF track, built from the device's per-slice records (rsi_hot_set_track_index).
Through the test hooks: for every case and slice length the index, resolved to text offsets through the file's own members, is
the one tabix_util.expected_index derives from the inflated text alone -- which knows nothing of slices."""
import gzip

import numpy as np
import pytest

import tabix_util as tx

BAD_ARG, UNSUPPORTED = -2, -5
SLICES = [1, 255, 1024, 0]


@pytest.fixture(scope="module")
def hot():
    from rsicnv_amd import api
    h = api.RsiHot(0)
    yield h
    h.set_track_index(None)
    h.close()


def indexed(hot, write):
    """write() with a fresh index set: (BGZF bytes, the parsed index, its counts)."""
    from rsicnv_amd import api
    ix = api.TrackIndex()
    hot.set_track_index(ix)
    try:
        data, st = write()
    finally:
        hot.set_track_index(None)
    index = tx.parse_raw(ix.tbi_bytes())
    counts = ix.counts()
    ix.close()
    return data, index, counts


def check_index(data, index, counts, names):
    """The index of `data` against the rules; returns the inflated text and expected_index of it."""
    table = tx.member_table(data)
    text = b"".join(m[3] for m in table)
    assert text == gzip.decompress(data)
    exp = tx.expected_index(text, table)
    assert index["kind"] == "tbi" and index["names"] == names == list(exp) and index["trailing"] == 0
    assert index["header"] == dict(format=0x10000, col_seq=1, col_beg=2, col_end=3, meta=ord("#"), skip=0)
    got = tx.resolved(index, table)
    starts = {p for ref in exp.values() for p in ref["bin_of"]}
    for name, ref in zip(index["names"], index["refs"]):
        assert ref["pseudo"] is None and ref["order"] == sorted(ref["order"])
        g, e = got[name], exp[name]
        assert g["linear"] == e["linear"], (name, g["linear"][:8], e["linear"][:8])
        assert g["chunks"] == e["chunks"], (name, sorted(g["chunks"])[:8], sorted(e["chunks"])[:8])
        assert all(p in starts for p in g["linear"]) and g["linear"] == sorted(g["linear"])
        for b, cs in g["chunks"].items():
            for beg, end in cs:                # every chunk begins at a line, and holds lines of its bin only
                assert beg in starts and beg < end
                assert all(e["bin_of"][p] == b for p in e["bin_of"] if beg <= p < end)
    assert counts["nref"] == len(names)
    assert counts["chunks"] == sum(len(cs) for ref in index["refs"] for cs in ref["bins"].values())
    assert counts["windows"] == sum(len(ref["linear"]) for ref in index["refs"])
    return text, exp


def window_edges():
    """A line ending at 16 384, one starting there, and -- further on -- one spanning 16 383 .. 16 385 of the next window."""
    v = np.zeros(40_000, dtype=np.int32)
    v[16_000:16_384] = 5                      # ends at the boundary
    v[16_384:16_500] = 6                      # starts there
    v[32_767:32_769] = 7                      # [2 * 16384 - 1, 2 * 16384 + 1): spans a boundary
    v[20_000:20_010] = np.arange(10) + 1
    return v


def boundary_span():
    v = np.zeros(40_000, dtype=np.int32)
    v[16_383:16_385] = 9                      # 16 383 .. 16 385 itself
    v[100:200] = np.arange(100) % 7
    return v


def zero_run():
    v = (np.arange(200_000) // 997 % 5 + 1).astype(np.int32)   # few lines: at slice length 1 the slices are the cost
    v[49_990:50_000] = np.arange(10) + 1
    v[50_000:150_000] = 0                     # one line over windows 3 .. 9
    return v


def straddling():
    """Placed by pos0 around 2^17 or 2^20: lines that straddle position 600 of the array, and single bases around them."""
    v = np.zeros(1_200, dtype=np.int32)
    v[550:650] = 3
    v[650:700] = 4
    v[300:320] = np.arange(20) + 1
    v[900:910] = np.arange(10) + 1
    return v


def alternating():
    return (np.arange(6_000) % 2 + 1).astype(np.int32)


CASES = {"window_edges": (window_edges, 0), "boundary_span": (boundary_span, 0), "zero_run": (zero_run, 0), "level_17": (straddling, 131_072 - 600), "level_20": (straddling, 1_048_576 - 600),
         "member_boundary": (alternating, 0), "member_and_window": (alternating, 16_384 - 5_000), "near_limit": (lambda: (np.arange(4_000) // 3 % 4).astype(np.int32), 2**29 - 5_000)}

_RESULTS = {}


@pytest.mark.gpu
@pytest.mark.parametrize("slice_bases", SLICES)
@pytest.mark.parametrize("case", list(CASES))
def test_index_is_the_text_s_own(hot, case, slice_bases):
    make, pos0 = CASES[case]
    v = make()
    data, index, counts = indexed(hot, lambda: hot.debug_track(v, "chrT", pos0=pos0, slice_bases=slice_bases, format="bgzf"))
    text, exp = check_index(data, index, counts, ["chrT"])
    # the same for every slice length: text and index (as text offsets)
    got = (text, tx.resolved(index, tx.member_table(data)))
    assert _RESULTS.setdefault(case, got) == got
    lines = tx.parse_lines(text)
    ref = exp["chrT"]
    if case == "window_edges":
        assert ("chrT", 16_000, 16_384) in [l[:3] for l in lines] and ("chrT", 16_384, 16_500) in [l[:3] for l in lines]
        assert tx.reg2bin(16_000, 16_384) == 4681 and tx.reg2bin(16_384, 16_500) == 4682 and tx.reg2bin(32_767, 32_769) == 585
        assert set(ref["chunks"]) == {4681, 4682, 4683, 585}
    if case == "boundary_span":
        assert ("chrT", 16_383, 16_385) in [l[:3] for l in lines] and 585 in ref["chunks"]
    if case == "zero_run":
        p = [l[3] for l in lines if l[1:3] == (50_000, 150_000)]
        assert len(p) == 1 and ref["linear"][4:10] == p * 6 and ref["linear"][3] < p[0] < ref["linear"][10]
    if case == "level_17":
        assert tx.reg2bin(131_072 - 50, 131_072 + 50) == 73 and set(ref["chunks"]) == {4681 + 7, 73, 4681 + 8}
    if case == "level_20":
        assert tx.reg2bin(1_048_576 - 50, 1_048_576 + 50) == 9 and set(ref["chunks"]) == {4681 + 63, 9, 4681 + 64}
    if case == "member_boundary":
        table = tx.member_table(data)
        if slice_bases == 0:
            assert len(table) == 2 and table[1][2] == 65280 and 65280 not in ref["bin_of"]   # the boundary falls inside a line
            cut = max(p for p in ref["bin_of"] if p < 65280)
            after = min(p for p in ref["bin_of"] if p > 65280)
            assert tx.to_voff(cut, table) >> 16 == 0 and tx.to_voff(after, table) >> 16 == table[1][0]
    if case == "member_and_window":
        # more than 65 280 bytes of text in front of position 16 384: the chunk of window 1 and linear[1] begin in a later member,
        # and it is the device's own offsets that say so
        table = tx.member_table(data)
        at = next(l[3] for l in lines if l[1] == 16_384)
        assert at > 65_280 and set(ref["chunks"]) == {4681, 4682} and ref["chunks"][4682][0][0] == at and ref["linear"] == [0, at]
        dev = index["refs"][0]
        (beg, end), = dev["bins"][4682]
        member = next(m for m in table if m[2] <= at < m[2] + len(m[3]))
        assert beg == dev["linear"][1] == (member[0] << 16 | (at - member[2])) and dev["bins"][4681] == [(0, beg)]
        assert end >> 16 == table[-1][0] + table[-1][1] and end & 0xFFFF == 0
        if slice_bases == 0:
            assert len(table) == 2 and member is table[1] and beg >> 16 > 0
    if case == "near_limit":
        assert max(ref["chunks"]) == 4681 + 32_767 and len(ref["linear"]) == 32_768


@pytest.mark.gpu
def test_a_line_beyond_the_limit_is_refused(hot):
    from rsicnv_amd import api
    v = (np.arange(6_000) // 3 % 4).astype(np.int32)
    ix = api.TrackIndex()
    hot.set_track_index(ix)
    try:
        with pytest.raises(api.RsiError) as e:
            hot.debug_track(v, "chrT", pos0=2**29 - 5_000, format="bgzf")
        assert e.value.code == UNSUPPORTED and "536870912" in str(e.value)
        assert ix.counts() == dict(nref=0, chunks=0, windows=0)
    finally:
        hot.set_track_index(None)
    data, _ = hot.debug_track(v, "chrT", pos0=2**29 - 5_000, format="bgzf")      # without an index the limit is not the writer's
    assert gzip.decompress(data).count(b"\n") == 2_000


def bin_case():
    m, n = 101, 300_000
    pairs = [(40_000, 59_999), (150_000, 219_999)]       # 20 000 and 70 000 bases removed
    nb = (n - 90_000) // m
    values = np.random.default_rng(11).integers(0, 120, size=nb).astype(np.int32)
    return values, m, n, pairs


@pytest.mark.gpu
@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("slice_bins", SLICES)
def test_bin_track(hot, slice_bins, which):
    values, m, n, pairs = bin_case()
    data, index, counts = indexed(hot, lambda: hot.debug_bin_track(values, m, n, pairs, 61, which, "chrB", slice_bins, format="bgzf"))
    text, exp = check_index(data, index, counts, ["chrB"])
    got = (text, tx.resolved(index, tx.member_table(data)))
    assert _RESULTS.setdefault(("bins", which), got) == got
    # the windows inside the removed regions have no line: they take the next line's offset
    ref, lines = exp["chrB"], tx.parse_lines(text)
    behind = min(l[3] for l in lines if l[1] >= 220_000)
    inside = [w for w in range(len(ref["linear"])) if 150_000 <= w << 14 and (w + 1) << 14 <= 220_000]
    assert len(inside) >= 3 and all(ref["linear"][w] == behind for w in inside)
    assert not any(l[1] < 219_999 and l[2] > 150_000 for l in lines)


@pytest.mark.gpu
def test_text_format_with_an_index_is_refused_and_bytes_do_not_change(hot):
    from rsicnv_amd import api
    v = window_edges()
    values, m, n, pairs = bin_case()
    plain, _ = hot.debug_track(v, "chrT", format="bgzf")
    plain_bins, _ = hot.debug_bin_track(values, m, n, pairs, 61, 1, "chrB", format="bgzf")
    ix = api.TrackIndex()
    hot.set_track_index(ix)
    try:
        for call in (lambda: hot.debug_track(v, "chrT", format="text"), lambda: hot.debug_bin_track(values, m, n, pairs, 61, 1, "chrB", format="text")):
            with pytest.raises(api.RsiError) as e:
                call()
            assert e.value.code == BAD_ARG and "index" in str(e.value)
        assert hot.debug_track(v, "chrT", format="bgzf")[0] == plain
        assert hot.debug_bin_track(values, m, n, pairs, 61, 1, "chrB", format="bgzf")[0] == plain_bins
        assert ix.counts()["nref"] == 2
    finally:
        hot.set_track_index(None)
    assert hot.debug_track(v, "chrT", format="text")[0] == gzip.decompress(plain)
    assert hot.debug_track(v, "chrT", format="bgzf")[0] == plain


def test_the_symbols_are_declared_and_exported(hotlib):
    from rsicnv_amd import api
    for sym in ("rsi_track_index_create", "rsi_track_index_free", "rsi_hot_set_track_index", "rsi_track_index_append",
                "rsi_track_index_write_tbi", "rsi_track_index_counts", "rsi_track_index_debug_tbi"):
        assert sym in api.EXPORTS and hasattr(hotlib, sym)
