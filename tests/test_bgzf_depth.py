"""Compressed depth files: BGZF inflated on the device (kernels_inflate.hip), ordinary gzip inflated on the host.  The rule:
for a text file T and any compressed form C of T, the depth arrays, the counts (lines, stored, beyond, fallback, and bytes,
which count text bytes) and the command line's rows and log blocks are identical -- the log gains one line naming the format."""
import os
import shutil
import struct
import subprocess
import gzip

import numpy as np
import pytest

import bgzf_util as bz
from test_genome_text import EXE, cli_case, fai_of, genome_case, read_all, render, restate, slice_text

STATS = ("bytes", "lines", "stored", "beyond", "fallback")


@pytest.fixture(scope="module")
def hot():
    from rsicnv_amd import api
    h = api.RsiHot(0)
    yield h
    h.close()


def compressed_forms(text):
    """{form: bytes}: BGZF with 100-4000-byte members (lines straddle members and chunks), BGZF with 65280-byte members,
    gzip in one member and in several."""
    rng = np.random.default_rng(len(text))
    sizes = iter(lambda: int(rng.integers(100, 4001)), None)
    return {"bgzf_small": bz.bgzf(text, sizes=sizes), "bgzf_65280": bz.bgzf(text), "gzip": bz.gzip_members(text),
            "gzip_multi": bz.gzip_members(text, parts=7)}


# ---------------------------------------------------------------------------------------------------------------------
# the kernel against zlib
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("case", bz.inflate_cases(), ids=lambda c: c[0])
def test_inflate_bgzf_equals_zlib(hot, case):
    name, data, text = case
    got = hot.inflate_bgzf(data)
    assert got == text == gzip.decompress(data), name
    st = hot.inflate_stats()
    assert st["format"] == "bgzf" and st["text_bytes"] == len(text) and st["compressed_bytes"] == len(data) and st["eof_block"] == 1


def _bit_member(bits, isize, crc=0):
    """A member around a hand-made deflate stream: bits = [(value, nbits, msb_first)]."""
    acc, n, out = 0, 0, bytearray()
    for v, k, msb in bits:
        seq = [(v >> (k - 1 - i)) & 1 for i in range(k)] if msb else [(v >> i) & 1 for i in range(k)]
        for b in seq:
            acc |= b << n
            n += 1
            if n == 8:
                out.append(acc)
                acc, n = 0, 0
    if n:
        out.append(acc)
    return _wrap(bytes(out), crc, isize)


def _wrap(cdata, crc, isize):
    bsize = 18 + len(cdata) + 8
    return b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", bsize - 1) + cdata + struct.pack("<II", crc, isize)


def bad_members():
    text = bz.depth_text(3000, 5)
    good = bz.member(text)
    cdata = good[18:-8]
    crc, isize = struct.unpack("<II", good[-8:])
    return {
        "bad_crc": _wrap(cdata, crc ^ 0x10, isize),
        "bad_isize": _wrap(cdata, crc, isize - 1),
        # a dynamic block whose code-length code has no codes at all
        "bad_code_lengths": _bit_member([(1, 1, False), (2, 2, False), (0, 5, False), (0, 5, False), (0, 4, False)] + [(0, 3, False)] * 4, 3),
        # a fixed block that starts with a match (length 3, distance 1) before any byte exists
        "distance_too_far": _bit_member([(1, 1, False), (1, 2, False), (1, 7, True), (0, 5, True), (0, 7, True)], 3),
        "truncated": _wrap(cdata[:len(cdata) // 2], crc, isize),
    }


@pytest.mark.gpu
@pytest.mark.timeout(120)
def test_bad_members_are_errors_and_the_context_stays_usable(hot):
    from rsicnv_amd import api
    good_text = bz.depth_text(20_000, 9)
    good = bz.bgzf(good_text)
    reasons = {"bad_crc": "CRC32", "bad_isize": "ISIZE", "bad_code_lengths": "code lengths", "distance_too_far": "distance",
               "truncated": "ends inside"}
    first = bz.member(b"fine\n")
    for name, m in bad_members().items():
        data = first + m + bz.EOF_BLOCK
        with pytest.raises(api.RsiError) as e:
            hot.inflate_bgzf(data)
        assert e.value.code == -2 and f"compressed offset {len(first)} " in str(e.value) and reasons[name] in str(e.value), (name, str(e.value))
        assert hot.inflate_bgzf(good) == good_text, name


@pytest.mark.gpu
@pytest.mark.timeout(120)
def test_bad_member_messages_name_the_member_and_the_file(hot, tmp_path):
    """Three members of a few hundred bytes, the CRC32 of the second one flipped: the whole message of the depth reader (the
    member's offset in the file, the file) and of inflate_bgzf (the member's offset in the caller's bytes)."""
    from rsicnv_amd import api
    text = bz.depth_text(400, 7)
    cut =[0, len(text) // 3, 2 * len(text) // 3, len(text)]
    members = [bytearray(bz.member(text[a:b])) for a, b in zip(cut, cut[1:])]
    assert all(200 < len(m) < 1000 for m in members)
    members[1][-8] ^= 0x10
    data = b"".join(bytes(m) for m in members) + bz.EOF_BLOCK
    path = tmp_path / "bad_second.depth.gz"
    path.write_bytes(data)
    with pytest.raises(api.RsiError) as e:
        hot.load_depth_text(str(path), 1000)
    assert str(e.value) == f"RSI_ERR_BAD_ARG: BGZF: the member at compressed offset {len(members[0])} of {path} is bad: CRC32 mismatch"
    with pytest.raises(api.RsiError) as e:
        hot.inflate_bgzf(data)
    assert str(e.value) == f"RSI_ERR_BAD_ARG: BGZF: the member at compressed offset {len(members[0])} is bad: CRC32 mismatch"


# ---------------------------------------------------------------------------------------------------------------------
# the readers: every form of a file gives what its text gives
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.timeout(1500)
def test_genome_reader_compressed_equals_text(hotlib, tmp_path):
    """The genome file of test_genome_text (quirky lines, unknown and filtered names, chrC unsorted -> its fallback) as text,
    BGZF and gzip, with chunks of 128 KiB, 1 MiB and the default."""
    from rsicnv_amd import api
    cases, lines, order, fai_seqs = genome_case(hotlib, unsorted_chrom="chrC")
    text = render(lines, 21).encode()
    names, lens = fai_of(fai_seqs)
    plain = tmp_path / "genome.depth"
    plain.write_bytes(text)
    files = {"text": plain}
    for form, data in compressed_forms(text).items():
        files[form] = tmp_path / f"genome_{form}.depth.gz"
        files[form].write_bytes(data)
    ref = None
    for chunk in (128 << 10, 1 << 20, 0):
        for form, path in files.items():
            with api.GenomeText(str(path), names, lens, chunk_bytes=chunk) as g:
                got = read_all(g)
                ist = g.inflate_stats()
            assert ist["format"] == {"text": "text", "gzip": "gzip", "gzip_multi": "gzip"}.get(form, "bgzf")
            assert ist["text_bytes"] == len(text), form
            if ref is None:
                ref = got
                assert [x[3]["fallback"] for x in got if x[1] is not None] == [int(x[0] == "chrC") for x in got if x[1] is not None]
                for name, d, n, st in got:
                    if d is not None:
                        assert np.array_equal(d, restate(lines, name, n)), name
            assert [x[0] for x in got] == [x[0] for x in ref], (form, chunk)
            for (name, d, n, st), (_, d0, _, st0) in zip(got, ref):
                assert (d is None) == (d0 is None), (form, chunk, name)
                if d is not None:
                    assert np.array_equal(d, d0), (form, chunk, name)
                assert tuple(st[k] for k in STATS) == tuple(st0[k] for k in STATS), (form, chunk, name)


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_single_chromosome_reader_compressed_equals_text(hotlib, hot, tmp_path):
    cases, lines, order, fai_seqs = genome_case(hotlib, unsorted_chrom="chrC")
    for name in ("chrA", "chrC"):   # sorted; unsorted (the whole file through the host parser)
        text = slice_text(lines, name).encode()
        n = cases[name][0].size
        p = tmp_path / f"{name}.txt"
        p.write_bytes(text)
        st0 = hot.load_depth_text(str(p), n)
        d0 = hot.fetch("depth_in")
        assert st0["fallback"] == int(name == "chrC") and hot.inflate_stats()["format"] == "text"
        for form, data in compressed_forms(text).items():
            q = tmp_path / f"{name}_{form}.gz"
            q.write_bytes(data)
            st = hot.load_depth_text(str(q), n)
            assert np.array_equal(hot.fetch("depth_in"), d0), (name, form)
            assert tuple(st[k] for k in STATS) == tuple(st0[k] for k in STATS), (name, form, st, st0)
            ist = hot.inflate_stats()
            assert ist["text_bytes"] == len(text) and ist["compressed_bytes"] == len(data), (name, form, ist)


@pytest.mark.gpu
@pytest.mark.timeout(120)
def test_tiny_contigs_through_bgzf(tmp_path):
    """360 contigs in 128 KiB chunks of small members: many name changes per chunk, names read back from the device."""
    from rsicnv_amd import api
    rng = np.random.default_rng(12)
    lines, names, lens = ["# tiny"], [], []
    for i in range(360):
        n = int(rng.integers(200, 2001))
        names.append(f"ctg{i:04d}"); lens.append(n)
        lines += [(names[-1], f"{p}\t{p % 77}", p, p % 77) for p in range(1, n + 1)]
    text = render(lines, 4).encode()
    path = tmp_path / "tiny.depth.gz"
    path.write_bytes(bz.bgzf(text, block=1500))
    with api.GenomeText(str(path), names, lens, chunk_bytes=128 << 10, max_resident=3) as g:
        seen = [(name, g.depth(st["slot"])) for name, ptr, n, st in g]
    assert [x[0] for x in seen] == names
    for name, d in seen:
        assert np.array_equal(d, restate(lines, name, d.size)), name


# ---------------------------------------------------------------------------------------------------------------------
# command line: the same relative name in two directories, text in one and compressed in the other
# ---------------------------------------------------------------------------------------------------------------------

def _run(cwd, args):
    return subprocess.run([EXE, "rsi"] + args, cwd=cwd, capture_output=True, text=True, timeout=600)


def _log(path):
    return [l for l in open(path).read().splitlines() if not l.startswith(("timing:", "#depth file:"))]


@pytest.mark.gpu
@pytest.mark.timeout(1200)
@pytest.mark.parametrize("form", ["bgzf_small", "gzip_multi"])
def test_cli_compressed_equals_text(hotlib, tmp_path, form):
    base = tmp_path / "plain"
    base.mkdir()
    fa, genome, slices = cli_case(hotlib, str(base))
    other = tmp_path / "packed"
    other.mkdir()
    for f in ("ref.fa", "ref.fa.fai"):
        shutil.copy(base / f, other / f)
    files = [("genome.depth", None)] + [(os.path.basename(sl), name) for name, sl in slices[:1]]
    for rel, _ in files:
        (other / rel).write_bytes(compressed_forms((base / rel).read_bytes())[form])
    for rel, chrom in files:
        args = ["-f", "ref.fa", "-d", rel, "-o", "out.txt", "-np"] + (["-c", chrom] if chrom else [])
        r1, r2 = _run(base, args), _run(other, args)
        assert r1.returncode == 0 and r2.returncode == 0, r2.stderr[-3000:]
        assert (base / "out.txt").read_bytes() == (other / "out.txt").read_bytes(), rel
        assert _log(base / "out.txt.log") == _log(other / "out.txt.log"), rel
        packed_log = open(other / "out.txt.log").read()
        assert packed_log.count("#depth file: " + ("BGZF" if form.startswith("bgzf") else "gzip")) == 1, packed_log[-2000:]
        assert "#depth file:" not in open(base / "out.txt.log").read()
        assert [l for l in open(other / "out.txt") if not l.startswith("#")], rel


@pytest.mark.gpu
@pytest.mark.timeout(600)
@pytest.mark.parametrize("form", ["bgzf", "gzip"])
def test_cli_corrupt_compressed_file_exits_1_without_output(hotlib, tmp_path, form):
    fa, genome, slices = cli_case(hotlib, str(tmp_path))
    text = open(genome, "rb").read()
    data = bytearray(bz.bgzf(text) if form == "bgzf" else bz.gzip_members(text, parts=3))
    data[len(data) // 2] ^= 0x5A                    # inside a member's deflate data
    bad = tmp_path / "bad.depth.gz"
    bad.write_bytes(bytes(data))
    sl_bad = tmp_path / "bad_slice.gz"
    sdata = bytearray(bz.bgzf(open(slices[0][1], "rb").read()) if form == "bgzf" else bz.gzip_members(open(slices[0][1], "rb").read()))
    sdata[len(sdata) // 2] ^= 0x5A
    sl_bad.write_bytes(bytes(sdata))
    for path, chrom in ((bad, None), (sl_bad, slices[0][0])):
        out = tmp_path / "out.txt"
        r = _run(str(tmp_path), ["-f", fa, "-d", str(path), "-o", str(out), "-np"] + (["-c", chrom] if chrom else []))
        assert r.returncode == 1, (path, r.returncode, r.stderr[-2000:])
        assert ("BGZF" if form == "bgzf" else "gzip") in r.stderr and "offset" in r.stderr, r.stderr[-2000:]
        assert not out.exists()


@pytest.mark.gpu
@pytest.mark.timeout(900)
@pytest.mark.parametrize("form", ["gzip", "gzip_multi", "bgzf"])
def test_cli_truncated_file_exits_1_without_output(hotlib, tmp_path, form):
    """A file cut short (an interrupted `samtools depth | gzip`): zlib reports the early end as Z_BUF_ERROR after a short
    read, BGZF as a member past the end of the file.  Both -d forms exit 1 and leave no output."""
    fa, genome, slices = cli_case(hotlib, str(tmp_path))
    pack = {"gzip": lambda t: bz.gzip_members(t), "gzip_multi": lambda t: bz.gzip_members(t, parts=5), "bgzf": lambda t: bz.bgzf(t)}[form]
    for src, chrom in ((genome, None), (slices[0][1], slices[0][0])):
        data = pack(open(src, "rb").read())
        cut = tmp_path / ("cut_" + os.path.basename(src) + ".gz")
        cut.write_bytes(data[:int(len(data) * 0.6)])
        out = tmp_path / "out.txt"
        r = _run(str(tmp_path), ["-f", fa, "-d", str(cut), "-o", str(out), "-np"] + (["-c", chrom] if chrom else []))
        assert r.returncode == 1, (form, chrom, r.returncode, r.stderr[-2000:])
        assert "offset" in r.stderr and ("end of" in r.stderr or "past the end" in r.stderr), r.stderr[-2000:]
        assert not out.exists()


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_bgzf_without_eof_block_is_read_and_noted(hotlib, tmp_path):
    base, other = tmp_path / "plain", tmp_path / "packed"
    base.mkdir(); other.mkdir()
    fa, genome, slices = cli_case(hotlib, str(base))
    for f in ("ref.fa", "ref.fa.fai"):
        shutil.copy(base / f, other / f)
    (other / "genome.depth").write_bytes(bz.bgzf((base / "genome.depth").read_bytes(), eof=False))
    args = ["-f", "ref.fa", "-d", "genome.depth", "-o", "out.txt", "-np"]
    r1, r2 = _run(base, args), _run(other, args)
    assert r1.returncode == 0 and r2.returncode == 0, r2.stderr[-3000:]
    assert (base / "out.txt").read_bytes() == (other / "out.txt").read_bytes()
    assert "no BGZF EOF block" in open(other / "out.txt.log").read()
    from rsicnv_amd import api
    names, lens = ["chrP", "chrQ", "chrR"], [400_007, 350_019, 300_001]
    with api.GenomeText(str(other / "genome.depth"), names, lens) as g:
        list(g)
        assert g.inflate_stats()["eof_block"] == 0


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_single_chromosome_reader_over_many_chunks(hot, tmp_path):
    """More than one 64 MiB chunk of text through rsi_hot_load_depth_text: BGZF's device-to-device carry, the cut at the
    inflate's last line end and the text offsets; gzip's chunk loop."""
    n = 7_000_003
    rng = np.random.default_rng(31)
    d = rng.integers(0, 400, n)
    text = ("\n".join(f"{p}\t{x}" for p, x in zip(range(1, n + 3), np.concatenate([d, [5, 6]]))) + "\n").encode()
    assert len(text) > (64 << 20) + (1 << 20)
    p = tmp_path / "big.txt"
    p.write_bytes(text)
    st0 = hot.load_depth_text(str(p), n)
    d0 = hot.fetch("depth_in")
    assert st0["fallback"] == 0 and np.array_equal(d0[:n - 1], d[:n - 1])
    sizes = iter(lambda: int(rng.integers(100, 4001)), None)
    for form, data in (("bgzf", bz.bgzf(text, level=1)), ("bgzf_small", bz.bgzf(text, level=1, sizes=sizes)), ("gzip", bz.gzip_members(text, level=1))):
        q = tmp_path / f"big_{form}.gz"
        q.write_bytes(data)
        st = hot.load_depth_text(str(q), n)
        assert np.array_equal(hot.fetch("depth_in"), d0), form
        assert tuple(st[k] for k in STATS) == tuple(st0[k] for k in STATS), (form, st, st0)
        q.unlink()
    # The order broken exactly at each format's first chunk cut: the first line of chunk 2 repeats the last position of
    # chunk 1, which only the host's check across chunks sees.  The cut is the last line end in the first 64 MiB of text;
    # for BGZF, in the whole members (bz.bgzf's 65280 text bytes each) that fit in 64 MiB.
    chunk = 64 << 20
    for form, limit, pack in (("text", chunk, None), ("gzip", chunk, bz.gzip_members), ("bgzf", chunk // 65280 * 65280, bz.bgzf)):
        cut = text.rindex(b"\n", 0, limit) + 1
        end = text.index(b"\n", cut)
        pos, x = (int(v) for v in text[cut:end].split(b"\t"))
        line = f"{pos - 1}\t{x}".encode()
        assert len(line) == end - cut
        q = tmp_path / f"cut_{form}"
        bad = text[:cut] + line + text[end:]
        q.write_bytes(pack(bad, level=1) if pack else bad)
        st = hot.load_depth_text(str(q), n)
        exp = d0.copy()
        exp[pos - 2], exp[pos - 1] = x, 0   # what the sequential loop stores: the repeat overwrites, pos stays unset
        assert st["fallback"] == 1, (form, st)
        assert np.array_equal(hot.fetch("depth_in"), exp), form
        q.unlink()


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_bgzf_chunk_with_more_name_changes_than_the_list_is_cut_shorter(tmp_path):
    """Thousands of two-line contigs in 128 KiB chunks: more name changes than the boundary list holds (chunk / 64), so the
    chunk is cut shorter on the device, as the text path cuts it on the host.  Both give the same depth."""
    from rsicnv_amd import api
    lines, names, lens = [], [], []
    for i in range(9000):
        names.append(f"k{i:05d}"); lens.append(4)
        lines += [(names[-1], f"{p}\t{(i + p) % 50}", p, (i + p) % 50) for p in (1, 2)]
    text = render(lines, 9).encode()
    plain, packed = tmp_path / "k.depth", tmp_path / "k.depth.gz"
    plain.write_bytes(text)
    packed.write_bytes(bz.bgzf(text, block=3000))
    runs = {}
    for path in (plain, packed):
        with api.GenomeText(str(path), names, lens, chunk_bytes=128 << 10, max_resident=4) as g:
            runs[path.name] = [(name, g.depth(st["slot"]), tuple(st[k] for k in STATS)) for name, ptr, n, st in g]
    a, b = runs[plain.name], runs[packed.name]
    assert [x[0] for x in a] == [x[0] for x in b] == names
    for (name, d, s), (_, d2, s2) in zip(a, b):
        assert np.array_equal(d, d2) and s == s2, name
        assert np.array_equal(d, restate(lines, name, 4)), name
