"""BGZF and gzip writers for the tests: BGZF members written here with Python's zlib at any level or strategy, with deflate
blocks split by full flushes, and the inputs that reach every part of the inflate kernel."""
import struct
import zlib

import numpy as np

EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def member(raw, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flushes=()):
    """One BGZF member holding raw (len <= 65536); flushes: offsets at which the deflate stream is ended with a full flush
    (a new deflate block)."""
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    parts, prev = [], 0
    for f in flushes:
        parts.append(c.compress(raw[prev:f]))
        parts.append(c.flush(zlib.Z_FULL_FLUSH))
        prev = f
    parts.append(c.compress(raw[prev:]))
    parts.append(c.flush())
    cdata = b"".join(parts)
    bsize = 18 + len(cdata) + 8
    assert bsize <= 65536, bsize
    head = b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", bsize - 1)
    return head + cdata + struct.pack("<II", zlib.crc32(raw) & 0xFFFFFFFF, len(raw))


def bgzf(data, block=65280, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, eof=True, sizes=None):
    """data as BGZF: members of `block` bytes (or of the sizes drawn from `sizes`, an iterator), plus the EOF member."""
    out, p = [], 0
    while p < len(data):
        k = next(sizes) if sizes is not None else block
        out.append(member(data[p:p + k], level, strategy))
        p += k
    if eof:
        out.append(EOF_BLOCK)
    return b"".join(out)


def gzip_members(data, parts=1, level=6):
    """Ordinary gzip (not BGZF): `parts` members one after the other."""
    out, step = [], max(1, -(-len(data) // parts))
    for p in range(0, max(len(data), 1), step):
        c = zlib.compressobj(level, zlib.DEFLATED, 31)
        out.append(c.compress(data[p:p + step]) + c.flush())
    return b"".join(out)


def depth_text(n, seed=1, name=None):
    rng = np.random.default_rng(seed)
    d = rng.integers(0, 120, n)
    pre = f"{name}\t" if name else ""
    return "".join(f"{pre}{i + 1}\t{int(x)}\n" for i, x in enumerate(d)).encode()


def inflate_cases():
    """(name, BGZF bytes, text): levels, strategies, stored blocks, several deflate blocks per member, ISIZE 0 / 1 / 65536,
    distance-1 runs, 258-byte matches, distances near 32768, depth text."""
    rng = np.random.default_rng(7)
    text = depth_text(30_000, 3)
    rand = rng.integers(0, 256, 200_000, dtype=np.uint8).tobytes()
    cases = []
    for lv in (0, 1, 6, 9):
        cases.append((f"level{lv}", bgzf(text, level=lv), text))
    for nm, stg in (("fixed", zlib.Z_FIXED), ("huffman_only", zlib.Z_HUFFMAN_ONLY), ("rle", zlib.Z_RLE), ("filtered", zlib.Z_FILTERED)):
        cases.append((nm, bgzf(text, strategy=stg), text))
    cases.append(("random_stored", bgzf(rand, block=65000), rand))
    cases.append(("random_level1", bgzf(rand[:60_000], block=30_000, level=1), rand[:60_000]))
    multi = text[:60_000]
    cases.append(("full_flush", member(multi, 6, flushes=(1, 100, 5000, 5001, 40_000)) + EOF_BLOCK, multi))
    cases.append(("full_flush_fixed", member(multi, 6, zlib.Z_FIXED, flushes=(20_000,)) + EOF_BLOCK, multi))
    cases.append(("isize0", member(b"") + member(b"x") + EOF_BLOCK, b"x"))
    big = (b"12345\t67\n" * 8000)[:65536]
    cases.append(("isize65536", member(big) + EOF_BLOCK, big))
    runs = b"a" * 30_000 + b"b" + b"c" * 20_000
    cases.append(("dist1_runs", member(runs) + EOF_BLOCK, runs))
    far = rand[:300] + bytes(32_400) + rand[:300] + rand[300:1000]    # a 300-byte repeat 32700 bytes back: 258-byte matches
    cases.append(("far_distance", member(far, 9) + EOF_BLOCK, far))
    ladder = b"".join(bytes([i % 251]) * (i % 300 + 1) for i in range(400))[:65000]
    cases.append(("ladder", member(ladder, 9) + EOF_BLOCK, ladder))
    return cases
