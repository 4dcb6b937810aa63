"""GPU: the reference unfolded on the device (kernels_ref.hip through RsiRef.load_host) against "".join of the FASTA's lines,
byte for byte: every line layout and terminator, sequences at every file offset modulo 16, lengths around the line and around
the kernel's tile, with and without the last terminator; the same files as BGZF with small members, read by .gzi, by walking
the members and by explicitly named indexes; and the checks that keep a .fai or .gzi that does not fit the file from handing
over a wrong sequence."""
import struct

import numpy as np
import pytest

from bgzf_util import bgzf
from test_ref_host import gzi_of, write_fai

pytestmark = pytest.mark.gpu

BAD_ARG = -2
TILE = 4096                      # kRefTileBases (kernels.h): bases per workgroup
ALPHABET = np.frombuffer(b"ACGTNacgtnRYKM", dtype=np.uint8)
LINEBASES = [1, 3, 15, 16, 17, 60, 61, 64]


@pytest.fixture(scope="module")
def api(hotlib):
    from rsicnv_amd import api
    return api


def bases(n, rng):
    return ALPHABET[rng.integers(0, ALPHABET.size, n)].tobytes().decode()


def lengths_for(lb):
    return sorted({1, 15, 16, 17, max(lb - 1, 1), lb, lb + 1, 2 * lb, TILE - 1, TILE + 1, 2 * TILE + 1})


def build(seqs, lb, term, last_term=True, residues=None):
    """[(name, sequence)] -> (file bytes, .fai rows, [sequence]).  residues: the file offset modulo 16 each sequence is to begin
    at -- its header's name is padded to get there."""
    text, fai = b"", []
    for k, (nm, seq) in enumerate(seqs):
        if residues is not None:
            while (len(text) + 1 + len(nm) + len(term)) % 16 != residues[k] % 16:
                nm += "x"
        text += f">{nm}{term}".encode()
        fai.append([nm, len(seq), len(text), lb, lb + len(term)])
        lines = [seq[i:i + lb] for i in range(0, len(seq), lb)]
        text += (term.join(lines) + (term if last_term or k + 1 < len(seqs) else "")).encode()
    return text, fai, [s for _, s in seqs]


def files_for(lb, term, seed):
    """Files of up to five sequences covering lengths_for(lb), offsets stepping through the residues modulo 16."""
    rng = np.random.default_rng(seed)
    lens = lengths_for(lb)
    out = []
    for f, i in enumerate(range(0, len(lens), 4)):
        part = lens[i:i + 4]
        if len(part) < 3:
            part = part + [lb + 2, 33][:3 - len(part)]
        seqs = [(f"s{f}_{j}", bases(n, rng)) for j, n in enumerate(part)]
        out.append(build(seqs, lb, term, last_term=(f % 2 == 0), residues=[(5 * f + 3 * j + lb) for j in range(len(seqs))]))
    return out


def put(tmp_path, name, data, fai, gzi=None):
    p = tmp_path / name
    p.write_bytes(data)
    write_fai(tmp_path / (name + ".fai"), fai)
    if gzi is not None:
        (tmp_path / (name + ".gzi")).write_bytes(gzi)
    return p


def small_members(seed):
    rng = np.random.default_rng(seed)
    return iter(int(x) for x in rng.integers(1, 3000, 1 << 20))


def load_all(api, path, want, chunks=None, **kw):
    """chunks: (bases per transfer of a text load, text bytes per inflate launch of a BGZF load) instead of the 32 Mi defaults."""
    r = api.RsiRef(str(path), **kw)
    try:
        if chunks:
            r.debug_set_chunks(*chunks)
        assert r.count == len(want)
        for i, seq in enumerate(want):
            got = r.load_host(i)
            assert len(got) == len(seq)
            if got != seq.encode():
                k = next(j for j in range(len(seq)) if got[j] != ord(seq[j]))
                raise AssertionError(f"{path.name} sequence {i} ({len(seq)} bases): first difference at base {k}: {got[k:k + 20]!r} != {seq[k:k + 20]!r}")
        assert r.load_host(0) == want[0].encode()          # once more: the same bytes
    finally:
        r.close()


@pytest.mark.parametrize("term", ["\n", "\r\n"], ids=["lf", "crlf"])
@pytest.mark.parametrize("lb", LINEBASES)
def test_text_and_bgzf_layouts(api, tmp_path, lb, term):
    seen = set()
    for f, (text, fai, want) in enumerate(files_for(lb, term, 100 + lb)):
        seen |= {row[2] % 16 for row in fai}
        load_all(api, put(tmp_path, f"t{f}.fa", text, fai), want)
        data = bgzf(text, sizes=small_members(lb + f))
        load_all(api, put(tmp_path, f"walk{f}.fa.gz", data, fai), want)                          # no .gzi: the members are walked
        load_all(api, put(tmp_path, f"gzi{f}.fa.gz", data, fai, gzi=gzi_of(data)[0]), want)      # FILE.gzi beside it
    assert len(seen) >= 8, seen


def test_every_offset_residue(api, tmp_path):
    rng = np.random.default_rng(16)
    seqs = [(f"r{k}", bases(int(rng.integers(1, 200)), rng)) for k in range(16)]
    text, fai, want = build(seqs, 60, "\n", residues=list(range(16)))
    assert sorted(row[2] % 16 for row in fai) == list(range(16))
    load_all(api, put(tmp_path, "res.fa", text, fai), want)
    data = bgzf(text, sizes=small_members(1))
    load_all(api, put(tmp_path, "res.fa.gz", data, fai, gzi=gzi_of(data)[0]), want)


def test_long_terminators_take_the_unstaged_kernel(api, tmp_path):
    """Lines of one or two bases ended by four bytes: a tile's text no longer fits the kernel's LDS stage."""
    rng = np.random.default_rng(4)
    for lb in (1, 2):
        seqs = [(f"u{j}", bases(n, rng)) for j, n in enumerate((1, lb + 1, TILE + 1, 2 * TILE + 1))]
        text, fai, want = build(seqs, lb, "\r\r\r\n", last_term=False, residues=[1, 6, 11, 0])
        load_all(api, put(tmp_path, f"long{lb}.fa", text, fai), want)


@pytest.mark.parametrize("lb", [60, 61])
def test_a_few_hundred_kilobases(api, tmp_path, lb):
    rng = np.random.default_rng(lb)
    seqs = [("a", bases(70_001, rng)), ("big", bases(300_007, rng)), ("z", bases(lb * 1000, rng))]
    for last_term in (True, False):                     # "z" ends a full line: with and without its terminator at the end of the file
        text, fai, want = build(seqs, lb, "\n", last_term=last_term, residues=[9, 2, 13])
        load_all(api, put(tmp_path, f"big{int(last_term)}.fa", text, fai), want)
        data = bgzf(text, sizes=small_members(lb))
        load_all(api, put(tmp_path, f"big{int(last_term)}.fa.gz", data, fai, gzi=gzi_of(data)[0]), want)
        load_all(api, put(tmp_path, f"bigw{int(last_term)}.fa.gz", data, fai), want)
        load_all(api, put(tmp_path, f"std{int(last_term)}.fa.gz", bgzf(text), fai), want)   # bgzip's own 65280-byte members


def crafted(tmp_path):
    """A BGZF file whose second sequence begins mid-member, spans five members with an empty one among them, and ends -- its last
    terminator included -- on a member's last byte."""
    rng = np.random.default_rng(77)
    seqs = [("first", bases(500, rng)), ("second", bases(60 * 50, rng)), ("third", bases(333, rng))]
    text, fai, want = build(seqs, 60, "\n")
    a = fai[1][2]
    b = a + 61 * 50
    sizes = [a + 5, 1000, 0, 1200, b - (a + 5) - 2200] + [400] * 20
    data = bgzf(text, sizes=iter(sizes))
    _, table = gzi_of(data)
    starts = [u for _, u in table]
    assert a not in starts and b in starts and starts.count(a + 1005) == 2
    return text, data, fai, want


def test_crafted_member_layout(api, tmp_path):
    text, data, fai, want = crafted(tmp_path)
    gzi = gzi_of(data)[0]
    load_all(api, put(tmp_path, "c.fa.gz", data, fai, gzi=gzi), want)
    load_all(api, put(tmp_path, "cw.fa.gz", data, fai), want)
    # explicitly named index files, as -refindex gives them; "none" walks although FILE.gzi is there
    (tmp_path / "elsewhere.gzi").write_bytes(gzi)
    write_fai(tmp_path / "elsewhere.fai", fai)
    (tmp_path / "bare.bgz").write_bytes(data)
    load_all(api, tmp_path / "bare.bgz", want, fai=str(tmp_path / "elsewhere.fai"), gzi=str(tmp_path / "elsewhere.gzi"))
    load_all(api, tmp_path / "c.fa.gz", want, gzi="none")
    # the text and the BGZF form of one file give the same bytes
    rt = api.RsiRef(str(put(tmp_path, "c.fa", text, fai)))
    rz = api.RsiRef(str(tmp_path / "c.fa.gz"))
    assert [rt.load_host(i) for i in range(3)] == [rz.load_host(i) for i in range(3)]
    rt.close(); rz.close()


# ---- many chunks, many spans: what every chromosome takes (32 M bases per transfer, 32 MB of text per inflate launch), forced
# on sequences of a few kilobases by rsi_ref_debug_set_chunks ----

@pytest.mark.parametrize("term", ["\n", "\r\n"], ids=["lf", "crlf"])
@pytest.mark.parametrize("lb", [1, 3, 16, 17, 60, 61])
def test_small_chunks_and_spans(api, tmp_path, lb, term):
    rng = np.random.default_rng(900 + lb)
    seqs = [(f"m{j}", bases(n, rng)) for j, n in enumerate((7 * lb + 3, 50 * lb, TILE + 1 + lb, 2 * TILE + 1))]
    text, fai, want = build(seqs, lb, term, last_term=False, residues=[3, 14, 8, 5])
    p = put(tmp_path, "m.fa", text, fai)
    # chunks that begin at a base index that is no multiple of 16, at a line's last base (lb - 1 + k lb), mid-line; larger than a tile
    for chunk in sorted({1009, max(lb - 1, 1) + 16 * lb, TILE + 3, 1}) if lb == 3 else sorted({1009, max(lb - 1, 1) + 16 * lb, TILE + 3}):
        if chunk == 1:
            want1 = [w[:200] for w in want]                      # one base per launch: the first 200 bases are enough
            text1, fai1, _ = build([(nm, w) for (nm, _), w in zip(seqs, want1)], lb, term, residues=[3, 14, 8, 5])
            load_all(api, put(tmp_path, "m1.fa", text1, fai1), want1, chunks=(1, 0))
            continue
        load_all(api, p, want, chunks=(chunk, 0))
    for k, span in enumerate((1024, 2048, 4099)):
        sizes = iter(int(x) for x in np.random.default_rng(lb + k).integers(200, 900, 1 << 16))     # a few members per span
        data = bgzf(text, sizes=sizes)
        load_all(api, put(tmp_path, f"m{span}.fa.gz", data, fai, gzi=gzi_of(data)[0]), want, chunks=(0, span))
        load_all(api, put(tmp_path, f"mw{span}.fa.gz", data, fai), want, chunks=(0, span))
    load_all(api, put(tmp_path, "mstd.fa.gz", bgzf(text, block=3000), fai), want, chunks=(0, 1024))   # a member larger than the span


def test_carried_spans_begin_where_it_is_hard(api, tmp_path):
    """One member per span (members of 600 to 1000 bytes under a span of 1024), so the spans end where the members end: right behind a
    line's last base with its terminator cut (the base waits for the next span, which then begins at a line's last base), mid-line
    at a base index that is no multiple of 16, and exactly behind a terminator."""
    rng = np.random.default_rng(41)
    seqs = [("h", bases(500, rng)), ("s", bases(60 * 100, rng)), ("t", bases(777, rng))]
    for last_term in (True, False):
        text, fai, want = build(seqs, 60, "\n", last_term=last_term)
        a = fai[1][2]
        m0 = a + 61 * 3 + 60            # ends behind base 239 = 3 * 60 + 59, in front of its "\n"
        m1 = 701                        # ends mid-line: text offset a + 944 = a + 15 * 61 + 29, base 929
        m2 = 642                        # ends at a + 1586 = a + 26 * 61: behind a terminator, base 1560
        assert 600 <= m0 <= 1000 and (m0 - a) % 61 == 60 and (m0 - a + m1) % 61 == 29 and (15 * 60 + 29) % 16 != 0 and 239 % 16 != 0
        assert (m0 - a + m1 + m2) % 61 == 0
        sizes = [m0, m1, m2] + [int(x) for x in rng.integers(600, 1000, 40)]
        data = bgzf(text, sizes=iter(sizes))
        for gzi in (gzi_of(data)[0], None):
            tag = f"carry{int(last_term)}{int(gzi is None)}.fa.gz"
            load_all(api, put(tmp_path, tag, data, fai, gzi=gzi), want, chunks=(0, 1024))
    # the crafted file (a sequence that begins mid-member, an empty member inside, an end on a member's last byte) span by span
    text, data, fai, want = crafted(tmp_path)
    load_all(api, put(tmp_path, "cs.fa.gz", data, fai, gzi=gzi_of(data)[0]), want, chunks=(0, 1024))
    load_all(api, put(tmp_path, "csw.fa.gz", data, fai), want, chunks=(0, 1024))
    load_all(api, put(tmp_path, "cs.fa", text, fai), want, chunks=(59, 0))       # text chunks that begin at a line's last base


def test_misfits_are_still_found_across_chunks(api, tmp_path):
    rng = np.random.default_rng(6)
    seqs = [("one", bases(700, rng)), ("two", bases(60 * 40 + 7, rng)), ("three", bases(900, rng))]
    text, fai, want = build(seqs, 60, "\n")
    bad = [row[:] for row in fai]
    bad[1][3] -= 1; bad[1][4] -= 1
    data = bgzf(text, sizes=iter([300] * 100))
    for path, chunks in ((put(tmp_path, "x.fa", text, bad), (333, 0)), (put(tmp_path, "x.fa.gz", data, bad), (0, 1024))):
        r = api.RsiRef(str(path))
        r.debug_set_chunks(*chunks)
        with pytest.raises(api.RsiError) as e:
            r.load_host(1)
        assert e.value.code == BAD_ARG and "two" in str(e.value)
        assert r.load_host(0) == want[0].encode()
        r.close()
    r = api.RsiRef(str(put(tmp_path, "y.fa", text, fai)))
    for args in ((-1, 0), (0, 1023), (0, 1 << 26)):
        with pytest.raises(api.RsiError):
            r.debug_set_chunks(*args)
    r.close()


def test_loaded_bytes_classify_like_the_string(api, tmp_path):
    rng = np.random.default_rng(5)
    seq = bases(20_011, rng)
    text, fai, _ = build([("p", bases(100, rng)), ("q", seq)], 60, "\n")
    data = bgzf(text, sizes=small_members(9))
    r = api.RsiRef(str(put(tmp_path, "q.fa.gz", data, fai)))
    got = np.frombuffer(r.load_host(1), dtype=np.uint8)
    r.close()
    hot = api.RsiHot(0)
    gc1, n1 = hot.debug_classify(got)
    gc2, n2 = hot.debug_classify(np.frombuffer(seq.encode(), dtype=np.uint8))
    hot.close()
    assert np.array_equal(gc1, gc2) and np.array_equal(n1, n2) and gc1.any() and n1.any()


def fails_naming(api, path, i, name, **kw):
    r = api.RsiRef(str(path), **kw)
    try:
        with pytest.raises(api.RsiError) as e:
            r.load_host(i)
        assert e.value.code == BAD_ARG and name in str(e.value), str(e.value)
    finally:
        r.close()


def test_a_fai_that_does_not_fit_is_refused(api, tmp_path):
    rng = np.random.default_rng(6)
    seqs = [("one", bases(700, rng)), ("two", bases(60 * 40 + 7, rng)), ("three", bases(900, rng))]
    text, fai, want = build(seqs, 60, "\n")
    crlf, fai_crlf, _ = build(seqs, 60, "\r\n")
    data = bgzf(text, sizes=small_members(2))
    off_lb = [row[:] for row in fai]
    off_lb[1][3] += 1                                       # LINEBASES off by one: the line end becomes a base
    off_off = [row[:] for row in fai]
    off_off[1][2] -= 1                                      # OFFSET one into the header line: its line end becomes the first base
    for tag, bad in (("lb", off_lb), ("off", off_off)):
        fails_naming(api, put(tmp_path, f"{tag}.fa", text, bad), 1, "two")
        fails_naming(api, put(tmp_path, f"{tag}.fa.gz", data, bad), 1, "two")
        load_all(api, put(tmp_path, f"{tag}_ok.fa", text, fai), want)      # the other sequences of such a file still load
    short = [row[:] for row in fai]
    short[1][3] -= 1; short[1][4] -= 1                      # one base less per line: bases land on the terminator positions
    fails_naming(api, put(tmp_path, "short.fa", text, short), 1, "two")
    fails_naming(api, put(tmp_path, "lf_on_crlf.fa", crlf, fai), 1, "two")   # the "\n" file's .fai on the "\r\n" file
    load_all(api, put(tmp_path, "crlf_ok.fa", crlf, fai_crlf), want)


def test_a_gzi_or_member_that_does_not_fit_gives_an_error_never_bytes(api, tmp_path):
    text, data, fai, want = crafted(tmp_path)
    other = bgzf(text, sizes=small_members(123))            # another compression of the same text
    p = put(tmp_path, "mix.fa.gz", data, fai, gzi=gzi_of(other)[0])
    r = api.RsiRef(str(p))
    for i in range(3):
        with pytest.raises(api.RsiError):
            r.load_host(i)
    r.close()
    # a .gzi whose text offsets disagree with the members' ISIZE
    image, table = gzi_of(data)
    shifted = struct.pack("<Q", len(table) - 1) + b"".join(struct.pack("<QQ", c, u + (1 if k >= 1 else 0)) for k, (c, u) in enumerate(table[1:]))
    fails_naming(api, put(tmp_path, "shift.fa.gz", data, fai, gzi=shifted), 1, "second")
    # a member of the second sequence with a corrupted CRC32: with the index and without
    at = table[1][0]
    bsize = struct.unpack_from("<H", data, at + 16)[0] + 1
    broken = bytearray(data)
    broken[at + bsize - 8] ^= 0x40
    for name, gzi in (("crc.fa.gz", image), ("crcw.fa.gz", None)):
        r = api.RsiRef(str(put(tmp_path, name, bytes(broken), fai, gzi=gzi)))
        with pytest.raises(api.RsiError) as e:
            r.load_host(1)
        assert "CRC32" in str(e.value) and "second" in str(e.value)
        assert r.load_host(0) == want[0].encode()            # the first sequence lies in front of the broken member
        r.close()
