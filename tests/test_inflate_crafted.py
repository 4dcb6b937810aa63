"""The inflate decoder (rsicnv_amd/csrc/inflate_core.h) on legal deflate streams that zlib's compressor never writes, and on
the malformed ones next to them (tests/deflate_craft.py).  The reference is zlib's inflate.

CPU: every valid case is what its family claims (recomputed from the tables it was written from), zlib inflates it to the
tokens' text, and the decoder built as plain C++ under ASan + UBSan (tests/sanitize_inflate) returns the same bytes; every
refused case gets the listed verdict from that build, and zlib refuses it too but for three named cases.

GPU: k_inflate_bgzf on the same files.  Only these runs reach what 64 lanes add to the decoder: the lane-shared match copy
(every_len_at_dist_*, match_*, length_258_*, dist_32768_*), the lane-shared stored copy (stored_at_every_bit_offset,
match_from_stored_bytes, isize_*), the CRC of 64 slices with its shift and fold (isize_*: slices of 0 and 1 bytes, sizes that
are no multiple of 64) and the ordering of lane 0's literals against the other lanes' reads (match_after_literal_dist_1_2)."""
import gzip
import os
import re
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

import bgzf_util as bz
import deflate_craft as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "tests", "sanitize_inflate", "inflate_harness")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
CASES = dc.crafted_cases()
SPECS = dc.crafted_specs()
REFUSED = dc.refused_cases()
FIRST = bz.member(b"fine\n")
READER_N = 20_000
ISIZE_SIZES = list(range(201)) + [4095, 4096, 4097, 65535, 65536]


def _members(data):
    """[(deflate payload, crc, isize)] of a BGZF file (BSIZE walked; the header is deflate_craft's fixed 18 bytes)."""
    out, p = [], 0
    while p < len(data):
        bsize = struct.unpack_from("<H", data, p + 16)[0] + 1
        assert bsize <= 65536
        out.append((data[p + 18:p + bsize - 8],) + struct.unpack_from("<II", data, p + bsize - 8))
        p += bsize
    return out


def _block(cid, member=0, block=0):
    return SPECS[cid][member][block]


def _matches(tokens):
    return [t for t in tokens if isinstance(t, tuple) and isinstance(t[0], int)]


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the cases are what they claim
# ---------------------------------------------------------------------------------------------------------------------

def test_every_family_of_the_issue_has_its_case():
    ids = [c[0] for c in CASES]
    assert len(set(ids)) == len(ids) == len(SPECS)
    assert len({r[0] for r in REFUSED}) == len(REFUSED) == 20
    for data in [c[1] for c in CASES]:
        assert data.endswith(dc.EOF_BLOCK)


@pytest.mark.parametrize("cid", ["codes_1_to_15", "hclen19_7bit_clcodes"])
def test_codes_of_1_to_15_bits_with_both_15_bit_codes_in_use(cid):
    b = _block(cid)
    lit_used, dist_used = dc.used_symbols(b["tokens"])
    for lengths, used in ((b["lit_len"], lit_used), (b["dist_len"], dist_used)):
        assert sorted(l for l in lengths if l) == list(range(1, 16)) + [15] and max(lengths) == 15
        assert dc.kraft(lengths) == 32768
        assert {s for s, l in enumerate(lengths) if l} == used
        assert len([s for s in used if lengths[s] == 15]) == 2
    if cid == "hclen19_7bit_clcodes":
        spelled = {it if isinstance(it, int) else int(it[0][1:]) for it in b["spelling"]}
        seven = [s for s in range(19) if b["cl_len"][s] == 7]
        assert b["hclen"] == 19 and max(b["cl_len"]) == 7 and len(seven) == 2 and set(seven) <= spelled
        assert dc.kraft(b["cl_len"]) == 32768 and {16, 17, 18} & spelled


def test_hlit_hdist_and_hclen_at_their_ends():
    b = _block("hlit286_hdist30_all_codes")
    lit_used, dist_used = dc.used_symbols(b["tokens"])
    assert len(b["lit_len"]) == 286 and len(b["dist_len"]) == 30 and all(b["lit_len"]) and all(b["dist_len"])
    assert dc.kraft(b["lit_len"]) == 32768 and dc.kraft(b["dist_len"]) == 32768
    assert lit_used == set(range(286)) and dist_used == set(range(30))
    dists = {t[1] for t in _matches(b["tokens"])}
    assert {16385, 24576, 24577, 32768} <= dists              # symbols 28 and 29, extra bits all 0 and all 1
    assert dc.dist_symbol(24576)[1:] == (13, 8191) and dc.dist_symbol(32768)[1:] == (13, 8191)
    b = _block("hlit257_hdist1")
    assert len(b["lit_len"]) == 257 and b["dist_len"] == [1] and not _matches(b["tokens"])
    b = _block("no_distance_code")
    assert len(b["lit_len"]) == 257 and b["dist_len"] == [0] and not _matches(b["tokens"])
    b = _block("hclen5_smallest")
    assert b["hclen"] == 5 and [s for s in range(19) if b["cl_len"][s]] == [0, 8, 16]
    lone = [b for b in SPECS["lone_end_of_block_code"][0] if b["type"] == "dynamic"]
    assert len(lone) == 3 and all(b["lit_len"] == [0] * 256 + [1] and b["tokens"] == [] for b in lone)


@pytest.mark.parametrize("cid,kind", [("zero_run_18_across_seam", "r18"), ("zero_run_17_across_seam", "r17"), ("copy_run_16_across_seam", "r16")])
def test_a_run_crosses_the_seam(cid, kind):
    b = _block(cid)
    hlit = len(b["lit_len"])
    crossing = [(k, i, n) for k, i, n in dc.spelling_runs(b["spelling"]) if i < hlit < i + n]
    assert [k for k, _, _ in crossing] == [kind]
    if kind == "r16":
        assert b["lit_len"][crossing[0][1] - 1] > 0


def test_the_other_spellings():
    b = _block("copy_run_16_from_last_literal_length")
    hlit = len(b["lit_len"])
    assert [(k, n) for k, i, n in dc.spelling_runs(b["spelling"]) if i == hlit] == [("r16", 6)] and b["lit_len"][-1] > 0
    b = _block("runs_of_3_6_10_11_138")
    assert {(k, n) for k, _, n in dc.spelling_runs(b["spelling"])} >= {("r16", 3), ("r16", 6), ("r17", 3), ("r17", 10), ("r18", 11), ("r18", 138)}
    b = _block("one_distance_code_of_1_bit")
    assert sorted(l for l in b["dist_len"] if l) == [1] and dc.used_symbols(b["tokens"])[1] == {b["dist_len"].index(1)}
    assert len(_matches(b["tokens"])) >= 50
    assert not any(_block("no_distance_code")["dist_len"])
    toks = _matches(_block("length_258_as_285_and_as_284_31")["tokens"])
    assert sum(1 for t in toks if t[0] == 258 and len(t) == 2) >= 9 and sum(1 for t in toks if t[0] == 258 and t[2:] == (284,)) >= 9
    assert dc.len_symbol(258) == (285, 0, 0) and dc.len_symbol(258, 284) == (284, 5, 31)


def test_copy_geometry_cases():
    for cid, dists in (("every_len_at_dist_1_to_130", list(range(1, 131))), ("every_len_at_dist_255_256_257", [255, 256, 257])):
        assert len(SPECS[cid]) == len(dists)
        for d, blocks in zip(dists, SPECS[cid]):
            m = dc.match_positions(blocks)
            assert {x[2] for x in m} == {d} and sorted(x[1] for x in m) == list(range(3, 259)) and m[0][0] == d
    toks = _block("match_after_literal_dist_1_2")["tokens"]
    for i, t in enumerate(toks):
        if isinstance(t, tuple):
            assert all(isinstance(x, int) for x in toks[i - t[1]:i]) and t[1] in (1, 2)
    assert {t[0] for t in _matches(toks)} >= set(range(3, 70)) | {127, 128, 129, 257, 258}
    m = dc.match_positions(SPECS["match_from_previous_match_tail"][0])
    assert len(m) > 100 and all(b[2] <= a[1] for a, b in zip(m, m[1:]))
    blocks = SPECS["match_from_stored_bytes"][0]
    op, stored = 0, []
    for b in blocks:
        k = b["n"] if b["type"] == "stored" else sum(1 if isinstance(t, int) else t[0] for t in b["tokens"])
        if b["type"] == "stored":
            stored.append((op, op + k))
        op += k
    inside = [x for x in dc.match_positions(blocks) if any(lo <= x[0] - x[2] and x[0] - x[2] + min(x[1], x[2]) <= hi for lo, hi in stored)]
    assert len(inside) >= 5 and len(stored) == 2
    m = dc.match_positions(SPECS["dist_32768_at_op_32768_and_end_on_65536"][0])
    assert m[0] == (32768, 258, 32768) and m[-1][0] + m[-1][1] == 65536 and m[-1][2] == 32768


def test_bit_reader_cases():
    members = SPECS["stored_at_every_bit_offset"]
    assert len(members) == 16
    for group in (members[:8], members[8:]):
        assert sorted(blocks[1]["header_end_bit"] % 8 for blocks in group) == list(range(8))
    sizes = [len(m[0]) for m in _members(dict((c[0], c[1]) for c in CASES)["stored_at_every_bit_offset"])]
    assert max(sizes[:8]) < 20 and min(sizes[8:16]) > 300       # few and many bytes behind the stored header
    blocks = SPECS["empty_stored_first_middle_final"][0]
    empty = [i for i, b in enumerate(blocks) if b["type"] == "stored" and b["n"] == 0]
    assert 0 in empty and len(blocks) - 1 in empty and any(0 < i < len(blocks) - 1 and blocks[i - 1]["type"] == "fixed" for i in empty)
    assert sorted(-blocks[-1]["end_bit"] % 8 for blocks in SPECS["final_block_padding_0_to_7"]) == list(range(8))
    blocks = SPECS["3000_one_literal_blocks"][0]
    assert len(blocks) == 3000 and all(len(b["tokens"]) == 1 for b in blocks)
    data = dict((c[0], c[1]) for c in CASES)["isize_0_to_200_4095_4096_4097_65535_65536"]
    assert [m[2] for m in _members(data)] == ISIZE_SIZES + [0]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_zlib_inflates_the_case_to_the_tokens_text(case):
    cid, data, text = case
    got = []
    for cdata, crc, isize in _members(data):
        d = zlib.decompressobj(-15)
        t = d.decompress(cdata)
        assert d.eof and not d.unused_data and len(t) == isize and zlib.crc32(t) == crc, cid
        got.append(t)
    assert b"".join(got) == text == gzip.decompress(data)


def _zlib_refuses(cdata):
    d = zlib.decompressobj(-15)
    try:
        d.decompress(cdata)
    except zlib.error:
        return True
    return not d.eof


@pytest.mark.parametrize("case", REFUSED, ids=lambda c: c[0])
def test_zlib_refuses_what_the_decoder_refuses(case):
    """But for a match past ISIZE and a wrong footer ISIZE (raw deflate knows no ISIZE) and a byte behind the final block
    (zlib stops at the stream's end; BGZF has the footer there, so the decoder refuses it by design)."""
    cid, member, reason = case
    cdata = _members(member)[0][0]
    if cid in dc.ZLIB_ACCEPTS:
        d = zlib.decompressobj(-15)
        d.decompress(cdata)
        assert d.eof and len(d.unused_data) == (cid == "trailing_byte")
    else:
        assert _zlib_refuses(cdata), cid


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the decoder as plain C++ under ASan + UBSan
# ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    tmp = tmp_path_factory.mktemp("probe")
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", str(tmp / "probe")], input=b"int main(){return 0;}",
                           capture_output=True)
    if probe.returncode != 0:
        pytest.skip("g++ cannot link the sanitizer runtimes here")
    r = subprocess.run(["make", "-f", "tests/sanitize_inflate/Makefile"], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return HARNESS


def _clean(r):
    return "Sanitizer" not in r.stderr and "runtime error" not in r.stderr


@pytest.mark.timeout(300)
@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_decoder_inflates_the_case_as_zlib_does(harness, tmp_path, case):
    cid, data, text = case
    src, out = tmp_path / "in.gz", tmp_path / "out.txt"
    src.write_bytes(data)
    r = subprocess.run([harness, "inflate", str(src), str(out)], capture_output=True, text=True, env=ENV, timeout=250)
    assert r.returncode == 0 and "inflate ok" in r.stdout and _clean(r), r.stdout[-1000:] + r.stderr[-3000:]
    assert out.read_bytes() == text


@pytest.mark.timeout(120)
@pytest.mark.parametrize("case", REFUSED, ids=lambda c: c[0])
def test_decoder_refuses_the_case_for_its_reason(harness, tmp_path, case):
    cid, member, reason = case
    src, out = tmp_path / "in.gz", tmp_path / "out.txt"
    src.write_bytes(FIRST + member + dc.EOF_BLOCK)
    r = subprocess.run([harness, "verdicts", str(src), str(out)], capture_output=True, text=True, env=ENV, timeout=100)
    assert r.returncode == 0 and _clean(r), r.stdout[-1000:] + r.stderr[-3000:]
    # the footer's ISIZE above 65536: the kernel's own check says "more data than ISIZE"; the host refuses it before any launch
    expected = "more data than ISIZE" if cid == "footer_isize_65537" else reason
    assert r.stdout.splitlines() == ["member 0: ok", "member 1: " + expected, "member 2: ok"], r.stdout
    assert out.read_bytes() == b"fine\n"


@pytest.mark.timeout(120)
def test_decoder_inflates_the_reader_case(harness, tmp_path):
    text = bz.depth_text(READER_N, 4)
    data, offsets = dc.reader_case(text)
    assert gzip.decompress(data) == text and len(set(offsets)) >= 6 and any(o % 2 for o in offsets)
    src, out = tmp_path / "in.gz", tmp_path / "out.txt"
    src.write_bytes(data)
    r = subprocess.run([harness, "inflate", str(src), str(out)], capture_output=True, text=True, env=ENV, timeout=100)
    assert r.returncode == 0 and "inflate ok" in r.stdout and _clean(r), r.stdout[-1000:] + r.stderr[-3000:]
    assert out.read_bytes() == text


# ---------------------------------------------------------------------------------------------------------------------
# GPU: k_inflate_bgzf
# ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def hot():
    from rsicnv_amd import api
    h = api.RsiHot(0)
    yield h
    h.close()


@pytest.mark.gpu
@pytest.mark.timeout(120)
@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_inflate_bgzf_equals_zlib_on_the_case(hot, case):
    cid, data, text = case
    got = hot.inflate_bgzf(data)
    assert got == text, (cid, len(got), len(text), next((i for i, (a, b) in enumerate(zip(got, text)) if a != b), None))
    st = hot.inflate_stats()
    assert st["format"] == "bgzf" and st["text_bytes"] == len(text) and st["compressed_bytes"] == len(data) and st["eof_block"] == 1
    assert st["blocks"] == len(_members(data))


@pytest.mark.gpu
@pytest.mark.timeout(120)
def test_refused_members_are_errors_and_the_context_stays_usable(hot):
    from rsicnv_amd import api
    good_text = bz.depth_text(3000, 9)
    good = bz.bgzf(good_text, block=7000)
    for cid, member, reason in REFUSED:
        with pytest.raises(api.RsiError) as e:
            hot.inflate_bgzf(FIRST + member + dc.EOF_BLOCK)
        msg = str(e.value)
        assert e.value.code == -2 and re.search(r"compressed offset %d\b" % len(FIRST), msg), (cid, msg)
        if cid == "footer_isize_65537":       # refused by the host's walk of the member headers
            assert "ISIZE above 65536" in msg, msg
        else:
            assert msg.endswith("is bad: " + reason), (cid, msg)
        assert hot.inflate_bgzf(good) == good_text, cid


@pytest.mark.gpu
@pytest.mark.timeout(120)
def test_chromosome_reader_on_crafted_members_equals_text(hot, tmp_path):
    """A depth text in members of 15-bit literal codes, a lone 1-bit distance code, an 18 run across the seam and a stored
    block at whatever bit the block before ends on."""
    stats = ("bytes", "lines", "stored", "beyond", "fallback")
    n = READER_N
    text = bz.depth_text(n, 4)
    data, offsets = dc.reader_case(text)
    assert gzip.decompress(data) == text and len(set(offsets)) >= 6 and any(o % 2 for o in offsets)
    plain, packed = tmp_path / "d.txt", tmp_path / "d.txt.gz"
    plain.write_bytes(text)
    packed.write_bytes(data)
    st0 = hot.load_depth_text(str(plain), n)
    d0 = hot.fetch("depth_in")
    assert st0["fallback"] == 0 and hot.inflate_stats()["format"] == "text"
    st = hot.load_depth_text(str(packed), n)
    assert np.array_equal(hot.fetch("depth_in"), d0)
    assert tuple(st[k] for k in stats) == tuple(st0[k] for k in stats), (st, st0)
    ist = hot.inflate_stats()
    assert ist["format"] == "bgzf" and ist["text_bytes"] == len(text) and ist["compressed_bytes"] == len(data), ist
