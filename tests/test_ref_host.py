"""CPU: the host decisions of the reference reader (rsicnv_amd/csrc/ref_host.h) through rsi_ref_open and the rsi_ref_debug_*
exports -- no GPU call anywhere: the .fai parse, read_fasta's name rule, flen and the text a base range needs, the bases a text
span holds whole, the .gzi parse, the members that cover a text range, and the refusal of plain gzip."""
import ctypes as C
import struct

import numpy as np
import pytest

import bgzf_walk
from bgzf_util import bgzf, gzip_members

BAD_ARG, UNSUPPORTED = -2, -5


@pytest.fixture(scope="module")
def api(hotlib):
    from rsicnv_amd import api
    return api


def fai_line(api, line):
    s = api.RsiRefSeq()
    rc = api.load_library().rsi_ref_debug_fai_line(line.encode(), C.byref(s))
    return rc, s, api.load_library().rsi_ref_last_error(None).decode()


def ranges(api, length, offset, lb, lw, k0, k1, a=0, b=0, at_eof=False):
    s = api.RsiRefSeq(length, offset, lb, lw, b"")
    out = np.zeros(5, dtype=np.int64)
    assert api.load_library().rsi_ref_debug_ranges(C.byref(s), k0, k1, a, b, int(at_eof), out.ctypes.data) == 0
    return [int(x) for x in out]


def write_ref(tmp_path, seqs, lb=60, term="\n", name="ref.fa", last_term=True):
    """[(name, sequence)] as a FASTA file and its .fai lines [(name, length, offset, lb, lw)]."""
    text, fai = "", []
    for k, (nm, seq) in enumerate(seqs):
        text += f">{nm}{term}"
        fai.append([nm, len(seq), len(text.encode()), lb, lb + len(term)])
        lines = [seq[i:i + lb] for i in range(0, len(seq), lb)]
        text += term.join(lines) + (term if last_term or k + 1 < len(seqs) else "")
    p = tmp_path / name
    p.write_bytes(text.encode())
    return p, fai


def write_fai(path, fai):
    path.write_text("".join("\t".join(str(x) for x in row) + "\n" for row in fai))


# ---- the .fai line ----

def test_fai_line_is_parsed(api):
    rc, s, _ = fai_line(api, "chr7\t159345973\t1234567890123\t60\t61")
    assert rc == 0 and (s.name, s.length, s.offset, s.linebases, s.linewidth) == (b"chr7", 159345973, 1234567890123, 60, 61)
    rc, s, _ = fai_line(api, "x 5 3 5 7 extra columns")            # blanks, a FASTQ index's further columns
    assert rc == 0 and (s.length, s.offset, s.linebases, s.linewidth) == (5, 3, 5, 7)
    rc, s, _ = fai_line(api, "x\t5\t3\t5\t5")                       # a file without terminators: linewidth == linebases
    assert rc == 0


@pytest.mark.parametrize("line, word", [
    ("chr1\t1000\t6\t60", "columns"),              # missing columns
    ("chr1\t1000", "columns"),
    ("", "columns"),
    ("chr1\t1000\t6\t0\t1", "LINEBASES"),          # linebases == 0
    ("chr1\t1000\t6\t60\t59", "LINEWIDTH"),        # linewidth < linebases
    ("chr1\t-1\t6\t60\t61", "LENGTH"),
    ("chr1\t2147479552\t6\t60\t61", "LENGTH"),     # 2^31 - 4096 and more: beyond the pipeline
    ("chr1\t1000\t-6\t60\t61", "OFFSET"),
    ("chr1\t1000\t6\t60\t200", "terminator"),
])
def test_fai_line_is_refused(api, line, word):
    rc, _, msg = fai_line(api, line)
    assert rc == BAD_ARG and word in msg, msg


def test_open_refuses_a_bad_fai_with_its_line_number(api, tmp_path):
    p, fai = write_ref(tmp_path, [("a", "ACGT" * 30), ("b", "TTGA" * 10)])
    fai[1][3] = 0
    write_fai(tmp_path / "ref.fa.fai", fai)
    with pytest.raises(api.RsiError) as e:
        api.RsiRef(str(p))
    assert e.value.code == BAD_ARG and "line 2" in str(e.value) and "LINEBASES" in str(e.value)


def test_open_refuses_a_length_that_does_not_fit_the_file(api, tmp_path):
    p, fai = write_ref(tmp_path, [("a", "ACGT" * 30), ("b", "TTGA" * 10)], last_term=False)
    write_fai(tmp_path / "ref.fa.fai", fai)
    api.RsiRef(str(p)).close()                       # as written it fits, the last terminator missing
    fai[1][1] += 1                                   # one base more than the file holds
    write_fai(tmp_path / "ref.fa.fai", fai)
    with pytest.raises(api.RsiError) as e:
        api.RsiRef(str(p))
    assert e.value.code == BAD_ARG and "b ends behind the end" in str(e.value)


def test_open_without_fai_and_explicit_paths(api, tmp_path):
    p, fai = write_ref(tmp_path, [("a", "ACGT" * 30)])
    with pytest.raises(api.RsiError) as e:
        api.RsiRef(str(p))
    assert e.value.code == BAD_ARG and "ref.fa.fai not found" in str(e.value)
    write_fai(tmp_path / "elsewhere.idx", fai)
    r = api.RsiRef(str(p), fai=str(tmp_path / "elsewhere.idx"))
    assert r.count == 1 and r.format == 0 and r.sequence(0) == dict(name="a", length=120, offset=3, linebases=60, linewidth=61)
    with pytest.raises(IndexError):
        r.sequence(1)
    r.close()


# ---- rsi_ref_find: read_fasta's rule ----

def test_find_follows_read_fasta(api, tmp_path):
    p, fai = write_ref(tmp_path, [("chr1", "A" * 10), ("1", "C" * 10), ("2", "G" * 10), ("chr2", "T" * 10), ("chrX", "N" * 10)])
    write_fai(tmp_path / "ref.fa.fai", fai)
    r = api.RsiRef(str(p))
    assert r.count == 5
    assert r.find("1") == 0          # "chr" + "1" comes first in the file: the first match wins
    assert r.find("chr1") == 0
    assert r.find("2") == 2          # the name itself comes first here
    assert r.find("chr2") == 3
    assert r.find("X") == 4          # rname -> chr + rname ...
    assert r.find("chrX") == 4
    p2, fai2 = write_ref(tmp_path, [("7", "A" * 10)], name="plain.fa")
    write_fai(tmp_path / "plain.fa.fai", fai2)
    r2 = api.RsiRef(str(p2))
    assert r2.find("7") == 0 and r2.find("chr7") == -1   # ... and not the other way round
    assert r.find("Y") == -1 and r.find("") == -1
    r.close(); r2.close()


# ---- flen, the text of a base range, the bases of a text span ----

def brute(length, offset, lb, lw):
    """pos[k] for every base, and per base whether it ends a full line."""
    return [offset + (k // lb) * lw + k % lb for k in range(length)]


@pytest.mark.parametrize("lb, tw", [(1, 1), (3, 2), (16, 1), (60, 1), (61, 2)])
def test_flen_and_text_ranges(api, lb, tw):
    lw, offset = lb + tw, 17
    for length in sorted({1, max(lb - 1, 1), lb, lb + 1, 3 * lb}):
        pos = brute(length, offset, lb, lw)
        out = ranges(api, length, offset, lb, lw, 0, length)
        assert out[0] == length + (length // lb) * tw                       # read_fasta's flen
        assert (out[1], out[2]) == (offset, offset + out[0])                # the whole sequence: its lines with every full line's terminator
        for k0 in range(length):
            for k1 in range(k0 + 1, length + 1):
                a, b = ranges(api, length, offset, lb, lw, k0, k1)[1:3]
                assert a == pos[k0]
                assert b == pos[k1 - 1] + 1 + (tw if k1 % lb == 0 else 0)


@pytest.mark.parametrize("lb, tw", [(1, 1), (3, 2), (16, 1), (5, 0)])
def test_contained_bases_invert_text_ranges(api, lb, tw):
    lw, offset, length = lb + tw, 9, 3 * lb + max(lb - 1, 1)
    pos = brute(length, offset, lb, lw)
    end = [pos[k] + 1 + (tw if (k + 1) % lb == 0 else 0) for k in range(length)]   # a base with its terminator
    for a in range(0, offset + length + 3 * tw + 6):
        for b in range(a, offset + length + 4 * tw + 8):
            k0, k1 = ranges(api, length, offset, lb, lw, 0, 1, a, b)[3:5]
            want0 = next((k for k in range(length) if pos[k] >= a), length)
            want1 = max([k + 1 for k in range(length) if end[k] <= b], default=0)
            assert (k0, k1) == (want0, max(want1, want0)), (a, b)


def test_last_base_without_its_terminator_at_the_end_of_the_file(api):
    lb, lw, offset = 4, 6, 10
    for length in (8, 7):
        text_end = offset + (length // lb) * lw + length % lb - (2 if length % lb == 0 else 0)   # the file stops behind the last base
        k1 = ranges(api, length, offset, lb, lw, 0, 1, 0, text_end, at_eof=False)[4]
        k1_eof = ranges(api, length, offset, lb, lw, 0, 1, 0, text_end, at_eof=True)[4]
        assert k1_eof == length
        assert k1 == (length - 1 if length % lb == 0 else length)   # inside a file that base waits for its terminator
    # an earlier line's cut terminator is never excused
    assert ranges(api, 12, offset, lb, lw, 0, 1, 0, offset + 4, at_eof=True)[4] == 3


# ---- .gzi ----

def gzi_of(data):
    """bgzip's .gzi for BGZF bytes: an entry for every member but the first, end-of-file block included."""
    ms = bgzf_walk.members(data)
    c = u = 0
    table = []
    for m in ms:
        table.append((c, u))
        c += m["size"]; u += len(m["text"])
    image = struct.pack("<Q", len(table) - 1) + b"".join(struct.pack("<QQ", a, b) for a, b in table[1:])
    return image, table


def parse_gzi(api, image):
    lib = api.load_library()
    n = lib.rsi_ref_debug_gzi(image, len(image), None, 0)
    if n < 0:
        return n, lib.rsi_ref_last_error(None).decode()
    t = np.zeros(2 * n, dtype=np.int64)
    assert lib.rsi_ref_debug_gzi(image, len(image), t.ctypes.data, n) == n
    return n, [(int(t[2 * i]), int(t[2 * i + 1])) for i in range(n)]


def test_gzi_round_trip(api):
    rng = np.random.default_rng(3)
    text = rng.integers(65, 70, 40_000, dtype=np.uint8).tobytes()
    data = bgzf(text, sizes=iter([1, 700, 0, 5000, 0, 0, 65280] + [3000] * 40))   # empty members repeat a text offset
    image, table = gzi_of(data)
    n, got = parse_gzi(api, image)
    assert n == len(table) and got == table
    n, got = parse_gzi(api, struct.pack("<Q", 0))         # a one-member file
    assert (n, got) == (1, [(0, 0)])


def test_gzi_refusals(api):
    text = bytes(10_000)
    image, table = gzi_of(bgzf(text, block=1000))
    for cut in (image[:-1], image[:-16], image[:7], b"", image + b"\0"):       # truncated, or longer than announced
        n, msg = parse_gzi(api, cut)
        assert n == BAD_ARG, (len(cut), msg)
    pairs = table[1:]
    for bad in ([pairs[1], pairs[0]] + pairs[2:],                             # not increasing
                [pairs[0], pairs[0]] + pairs[2:],                             # a compressed offset twice
                [(pairs[0][0], 5000), (pairs[1][0], 4000)] + pairs[2:]):      # text offsets going back
        img = struct.pack("<Q", len(bad)) + b"".join(struct.pack("<QQ", a, b) for a, b in bad)
        n, msg = parse_gzi(api, img)
        assert n == BAD_ARG and "increase" in msg, msg


# ---- the members that cover a text range ----

def cover(api, table, a, b):
    t = np.array(table, dtype=np.int64).reshape(-1)
    out = np.zeros(3, dtype=np.int64)
    assert api.load_library().rsi_ref_debug_cover(t.ctypes.data, len(table), a, b, out.ctypes.data) == 0
    return tuple(int(x) for x in out)


def test_member_cover(api):
    # text offsets: members of 100, 100, 0 (empty), 100, 50 bytes and the end-of-file block
    table = [(0, 0), (40, 100), (90, 200), (118, 200), (170, 300), (200, 350)]
    assert cover(api, table, 100, 150) == (1, 2, 0)        # starts on a member's first byte
    assert cover(api, table, 130, 200) == (1, 2, 30)       # ends on a member's last byte: the next one is not read
    assert cover(api, table, 10, 20) == (0, 1, 10)         # inside one member
    assert cover(api, table, 150, 250) == (1, 4, 50)       # across the empty member in the middle
    assert cover(api, table, 200, 201) == (3, 4, 0)        # begins behind the empty member: it is passed over
    assert cover(api, table, 0, 350) == (0, 5, 0)          # everything, the end-of-file block left out
    assert cover(api, table, 320, 360) == (4, 6, 20)       # runs into the last member: to the end of the file
    # brute force over every range
    starts = [u for _, u in table]
    for a in range(0, 350):
        for b in range(a + 1, 352, 7):
            first, stop, skew = cover(api, table, a, b)
            assert starts[first] <= a and skew == a - starts[first]
            assert first + 1 == len(table) or starts[first + 1] > a
            assert stop == len(table) or starts[stop] >= b
            assert stop == first + 1 or starts[stop - 1] < b


# ---- formats ----

def test_format_from_the_first_bytes(api, tmp_path):
    p, fai = write_ref(tmp_path, [("a", "ACGT" * 300)])
    raw = p.read_bytes()
    for name, data, fmt in (("plain.gz", raw, 0), ("bgzf.fa", bgzf(raw, block=500), 1)):   # the name says nothing
        q = tmp_path / name
        q.write_bytes(data)
        write_fai(tmp_path / (name + ".fai"), fai)
        r = api.RsiRef(str(q))
        assert r.format == fmt and r.count == 1
        r.close()


def test_plain_gzip_is_refused(api, tmp_path):
    p, fai = write_ref(tmp_path, [("a", "ACGT" * 300)])
    q = tmp_path / "ref.fa.gz"
    q.write_bytes(gzip_members(p.read_bytes(), parts=2))
    write_fai(tmp_path / "ref.fa.gz.fai", fai)
    with pytest.raises(api.RsiError) as e:
        api.RsiRef(str(q))
    assert e.value.code == UNSUPPORTED and "bgzip" in str(e.value)


def test_named_gzi_must_exist(api, tmp_path):
    p, fai = write_ref(tmp_path, [("a", "ACGT" * 300)])
    q = tmp_path / "ref.fa.gz"
    q.write_bytes(bgzf(p.read_bytes(), block=400))
    write_fai(tmp_path / "ref.fa.gz.fai", fai)
    with pytest.raises(api.RsiError) as e:
        api.RsiRef(str(q), gzi=str(tmp_path / "missing.gzi"))
    assert e.value.code == BAD_ARG and "missing.gzi" in str(e.value)
    api.RsiRef(str(q), gzi="none").close()
    api.RsiRef(str(q)).close()                      # no .gzi beside it: the members will be walked
