"""GPU: tracks as BGZF (kernels_deflate.hip, deflate_core.h, track.hip) through the C ABI, judged by zlib: the two kernels alone
(rsi_hot_debug_deflate), the writers' test hooks with the format set to BGZF against their own text, files with their end-of-file
block, determinism, and the size condition.  The format contract is checked member by member in tests/bgzf_walk.py."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

import bgzf_walk as bw
import track_restatement as tr
from bgzf_util import EOF_BLOCK

pytestmark = pytest.mark.gpu

I32_MIN = -2**31
BAD_ARG = -2


@pytest.fixture(scope="module")
def hot():
    from rsicnv_amd import api
    h = api.RsiHot(0)
    yield h
    h.close()


def deflate(hot, text):
    """text through the two kernels: the members, with every point of the contract and the figures checked."""
    data, st = hot.debug_deflate(text)
    ms = bw.check_file(data, text, eof=False)
    assert len(ms) == st["members"] == -(-len(text) // bw.MEMBER_TEXT)
    assert all(len(m["text"]) == bw.MEMBER_TEXT for m in ms[:-1])
    assert st["text_bytes"] == len(text) and st["file_bytes"] == len(data)
    assert st["stored_members"] == sum(1 for m in ms if m["btype"] == 0 and m["size"] == len(m["text"]) + 5 + 26)
    assert hot.deflate_stats() == st
    return data, st, ms


# ---- the kernels alone ----

def test_no_text_no_member(hot):
    data, st = hot.debug_deflate(b"")
    assert data == b"" and st["members"] == 0 and st["file_bytes"] == 0


@pytest.mark.parametrize("case", bw.length_cases(), ids=lambda c: c[0])
def test_lengths(hot, case):
    deflate(hot, case[1])


@pytest.mark.parametrize("case", bw.content_cases(), ids=lambda c: c[0])
def test_contents(hot, case):
    name, text = case
    data, st, ms = deflate(hot, text)
    if name in ("one_value", "two_values", "permutation"):
        assert st["stored_members"] == 0 and len(data) < len(text) // 40
    if name == "random_then_text":
        assert any(m["btype"] == 2 for m in ms)


def test_random_bytes_are_stored(hot):
    rand = os.urandom(bw.MEMBER_TEXT)
    data, st, ms = deflate(hot, rand)
    assert st["stored_members"] == 1 and ms[0]["btype"] == 0 and len(data) <= 65311


# ---- through the writers ----

def both(call):
    """call(format) -> (bytes, stats): the text and the BGZF bytes of the same call on the same context."""
    text, st_text = call("text")
    data, st = call("bgzf")
    return text, st_text, data, st


def check_writer(hot, call):
    text, st_text, data, st = both(call)
    ms = bw.check_file(data, text, eof=False)
    assert st["bytes"] == len(text) == st_text["bytes"] and st["lines"] == st_text["lines"] == text.count(b"\n")
    ds = hot.deflate_stats()
    assert ds["file_bytes"] == len(data) and ds["text_bytes"] == len(text) and ds["members"] == len(ms)
    assert call("text")[0] == text and hot.deflate_stats()["members"] == 0      # the setting did not stick
    return text, data, st


@pytest.mark.parametrize("slice_bases", [1, 255, 65536, 0])
def test_depth_track_slices(hot, slice_bases):
    # a slice costs a wait, and three calls run here: slices of one base over the first 5000 bases only (5000 one-line members,
    # each copied one slice late), the other lengths over all 200 000
    n = 5000 if slice_bases == 1 else 200_000
    v = bw.poisson_depth()[:n]
    text, data, st = check_writer(hot, lambda f: hot.debug_track(v, "chr1", slice_bases=slice_bases, format=f))
    assert text == tr.text(v, "chr1")
    assert st["slices"] == (-(-n // slice_bases) if slice_bases else 1)


def test_constant_array_one_line(hot):
    text, data, st = check_writer(hot, lambda f: hot.debug_track(np.full(70_000, 31, dtype=np.int32), "chr1", format=f))
    assert text == b"chr1\t0\t70000\t31\n" and st["lines"] == 1


def test_extreme_values_and_coordinates(hot):
    v = np.array([I32_MIN, I32_MIN, -1, -1, -1, 0, 2**31 - 1, -2147483647, 5, 5], dtype=np.int32)
    text, data, st = check_writer(hot, lambda f: hot.debug_track(v, "chrX", pos0=2**40 - 5, slice_bases=3, format=f))
    assert text == tr.text(v, "chrX", 2**40 - 5) and b"1099511627776" in text and b"-2147483648" in text


@pytest.mark.parametrize("which", [0, 1], ids=["median", "ratio"])
def test_bin_track(hot, which):
    nb, m, nreg = 5000, 7, 49
    kept = nb * m + 3
    breaks = [int(x) for x in np.linspace(1, kept - 2, nreg).astype(np.int64)]
    assert len(set(breaks)) == nreg
    pairs, cum = [], 0
    for k, c in enumerate(breaks):
        pairs.append((c + cum, c + cum + 2 + k % 5))
        cum += 3 + k % 5
    values = np.random.default_rng(9).integers(0, 120, nb).astype(np.int32)
    text, data, st = check_writer(hot, lambda f: hot.debug_bin_track(values, m, kept + cum, pairs, 60, which, "chr2", slice_bins=1500, format=f))
    assert st["slices"] == 4 and st["lines"] > nb


def test_set_track_format(hot):
    from rsicnv_amd import api
    v = bw.poisson_depth()[:5000]
    text = hot.debug_track(v, "c")[0]
    hot.set_track_format("bgzf")                     # holds until changed
    a = hot.debug_track(v, "c")[0]
    b = hot.debug_track(v, "c")[0]
    hot.set_track_format(0)
    assert a == b and gzip.decompress(a) == text == hot.debug_track(v, "c")[0]
    for bad in (2, -1):
        with pytest.raises(api.RsiError) as ei:
            hot.set_track_format(bad)
        assert ei.value.code == BAD_ARG
    assert hot.debug_track(v, "c")[0] == text


# ---- files ----

def test_two_chromosomes_appended_and_the_eof_block(hot, tmp_path):
    import torch
    from rsicnv_amd import api
    va, vb = bw.poisson_depth()[:150_000], (np.arange(90_001) // 9 % 50).astype(np.int32)
    da, db = torch.from_numpy(va).to("cuda:0"), torch.from_numpy(vb).to("cuda:0")
    torch.cuda.synchronize()
    p, plain = str(tmp_path / "two.bedgraph.gz"), str(tmp_path / "two.bedgraph")
    sa = hot.write_track_device(da.data_ptr(), va.size, "chrA", p, format="bgzf")
    fa = hot.deflate_stats()
    sb = hot.write_track_device(db.data_ptr(), vb.size, "chrB", p, append=True, format="bgzf")
    fb = hot.deflate_stats()
    text = tr.text(va, "chrA") + tr.text(vb, "chrB")
    assert os.path.getsize(p) == fa["file_bytes"] + fb["file_bytes"] and sa["bytes"] + sb["bytes"] == len(text)
    api.bgzf_write_eof(p)
    data = open(p, "rb").read()
    ms = bw.check_file(data, text)
    assert len(ms) == fa["members"] + fb["members"] and data.count(EOF_BLOCK) == 1
    # members are cut per call: chrA's last one is short, chrB starts its own
    assert len(ms[fa["members"] - 1]["text"]) == len(tr.text(va, "chrA")) % bw.MEMBER_TEXT
    # the plain-text call on the same context: the text as before
    hot.write_track_device(da.data_ptr(), va.size, "chrA", plain)
    hot.write_track_device(db.data_ptr(), vb.size, "chrB", plain, append=True)
    assert open(plain, "rb").read() == text
    # a file that cannot be written
    with pytest.raises(api.RsiError) as ei:
        api.bgzf_write_eof(str(tmp_path / "no_such_dir" / "t.gz"))
    assert ei.value.code == -6


def test_abi():
    from rsicnv_amd import api
    lib = api.load_library()
    for sym in ("rsi_hot_set_track_format", "rsi_hot_last_deflate_stats", "rsi_bgzf_write_eof", "rsi_hot_debug_deflate"):
        assert sym in api.EXPORTS and hasattr(lib, sym)
    assert C.sizeof(api.RsiDeflateStats) == 5 * 8 and C.sizeof(api.RsiTrackStats) == 7 * 8


# ---- determinism ----

def test_same_text_same_bytes_on_any_context(hot):
    from rsicnv_amd import api
    v = bw.poisson_depth()
    a = hot.debug_track(v, "chr1", format="bgzf")[0]
    b = hot.debug_track(v, "chr1", format="bgzf")[0]
    fresh = api.RsiHot(0)
    c = fresh.debug_track(v, "chr1", format="bgzf")[0]
    d = fresh.debug_deflate(bw.poisson_text())[0]
    fresh.close()
    assert a == b == c == d


# ---- the size condition ----

@pytest.mark.parametrize("name,values", [("poisson", bw.poisson_depth), ("ten_digit", bw.ten_digit_values)])
def test_size_condition(hot, name, values):
    """Smaller than zlib level 1 with Z_HUFFMAN_ONLY on the same 65280-byte members plus 26 bytes each: a coder without matches
    or without codes of the text's own does not get there."""
    v = values()
    text = tr.text(v, "chr1")
    data, st = hot.debug_track(v, "chr1", format="bgzf")
    assert gzip.decompress(data) == text
    cap = bw.size_cap(text)
    print(f"{name}: text {len(text)} file {len(data)} cap {cap} level1 {bw.zlib_bytes(text, 1)} level6 {bw.zlib_bytes(text, 6)}")
    assert len(data) < cap
