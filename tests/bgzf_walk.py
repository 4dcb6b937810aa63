"""The BGZF format contract of the track writers, judged by zlib: a walk over a file's members that checks every point of it, the
inputs of the deflate tests (shared by the CPU harness and the GPU kernel), and the size cap of the size condition."""
import gzip
import os
import struct
import zlib

import numpy as np

import track_restatement as tr
from bgzf_util import EOF_BLOCK, depth_text

MEMBER_TEXT = 65280
HEAD = b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00"


def members(data):
    """data: a sequence of BGZF members and nothing else.  Every member: the fixed 16 header bytes (gzip, CM = 8, FLG = FEXTRA
    only, XLEN = 6, a BC subfield of length 2), BSIZE = its true size -- the raw deflate payload ends exactly where the footer
    begins --, ISIZE <= 65280, CRC32 and ISIZE those of its text.  Returns [dict(text, size, btype)] (btype: of the first deflate
    block)."""
    out, p = [], 0
    while p < len(data):
        assert data[p:p + 16] == HEAD, (p, data[p:p + 16].hex())
        bsize = struct.unpack_from("<H", data, p + 16)[0] + 1
        assert 18 + 8 < bsize and p + bsize <= len(data), (p, bsize, len(data))
        payload = data[p + 18:p + bsize - 8]
        d = zlib.decompressobj(-15)
        text = d.decompress(payload) + d.flush()
        assert d.eof and d.unused_data == b"" and d.unconsumed_tail == b"", (p, len(d.unused_data))   # the whole payload and nothing beyond
        short = zlib.decompressobj(-15)                      # ... and not a byte less: the stream's end is the payload's last byte
        short.decompress(payload[:-1])
        assert not short.eof, p
        crc, isize = struct.unpack_from("<II", data, p + bsize - 8)
        assert isize == len(text) <= MEMBER_TEXT and crc == (zlib.crc32(text) & 0xFFFFFFFF), (p, isize, len(text))
        out.append(dict(text=text, size=bsize, btype=(payload[0] >> 1) & 3))
        p += bsize
    return out


def check_file(data, text, eof=True):
    """A whole track file: members of `text`, none empty, then (eof) exactly one end-of-file block; gzip reads it as `text`."""
    body = data
    if eof:
        assert data[-28:] == EOF_BLOCK
        body = data[:-28]
    ms = members(body)
    assert all(len(m["text"]) > 0 for m in ms)
    assert b"".join(m["text"] for m in ms) == text
    assert gzip.decompress(data) == text if data else text == b""
    return ms


def zlib_bytes(text, level, strategy=zlib.Z_DEFAULT_STRATEGY):
    """What zlib makes of the same 65280-byte members, 26 bytes of frame each."""
    total = 0
    for p in range(0, len(text), MEMBER_TEXT):
        c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
        total += len(c.compress(text[p:p + MEMBER_TEXT]) + c.flush()) + 26
    return total


def size_cap(text):
    """The size condition: a file must be smaller than level 1 with Z_HUFFMAN_ONLY."""
    return zlib_bytes(text, 1, zlib.Z_HUFFMAN_ONLY)


def poisson_depth(n=200_000, seed=30):
    return np.random.default_rng(seed).poisson(30, n).astype(np.int32)


def ten_digit_values(n=60_000, seed=31):
    """Values uniform in 10^8 .. 10^8 + 2^30: long, digit-heavy lines, every base its own."""
    return np.random.default_rng(seed).integers(10**8, 10**8 + 2**30, n).astype(np.int32)


_CACHE = {}


def poisson_text():
    if "poisson" not in _CACHE:
        _CACHE["poisson"] = tr.text(poisson_depth(), "chr1")
    return _CACHE["poisson"]


def ten_digit_text():
    if "ten" not in _CACHE:
        _CACHE["ten"] = tr.text(ten_digit_values(), "chr1")
    return _CACHE["ten"]


def far_marker(distance, filler):
    """A 64-byte random marker and its repeat `distance` bytes on, `filler` bytes between and behind."""
    rng = np.random.default_rng(distance)
    marker = rng.integers(0, 256, 64, dtype=np.uint8).tobytes()
    return marker + filler(distance - 64, rng) + marker + filler(500, rng)


def _random(n, rng):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def _letters(n, rng):
    return (rng.integers(0, 4, n, dtype=np.uint8) + 97).tobytes()     # compresses (2 bits a byte), long repeats are rare


def length_cases():
    """(name, text): the lengths at which a path changes -- below the shortest match, the longest match and its chain at distance
    1, one member or two, three members."""
    cases = [(f"rep{n}", b"a" * n) for n in (1, 2, 3, 258, 259, 260, 517)]
    text = poisson_text()
    cases += [(f"len{n}", text[:n]) for n in (65279, 65280, 65281, 2 * 65280 + 1)]
    return cases


def content_cases():
    perm = np.random.default_rng(5).permutation(256).astype(np.uint8).tobytes()
    return [
        ("one_value", b"7" * 70_000),
        ("two_values", b"01" * 20_000),
        ("permutation", perm * 300),
        ("random_then_text", os.urandom(40_000) + poisson_text()[:200_000]),
        ("marker_32768_random", far_marker(32768, _random)),
        ("marker_32769_random", far_marker(32769, _random)),
        ("marker_32768_letters", far_marker(32768, _letters)),
        ("marker_32769_letters", far_marker(32769, _letters)),
        ("depth_text", depth_text(20_000, 4)),
        ("poisson_track", poisson_text()),
    ]
