"""Record streams for the device record finder, shared by the CPU test of bam_walk_core.h and the GPU test of
`set_bam_read("device")`: each case is (refs, records, tid) -- the records' bytes joined are the inflated stream behind the
header -- built so that record starts, seams of the 16 384-byte segments and look-alike bytes meet in the ways the finder has
to survive.  serial_walk() is the chain every result is compared with."""
import struct

import numpy as np

import bam_util as bu

SEG = 16384
BEYOND, BAD, OPEN = 1, 2, 4
REFS = [("chrA", 120_011), ("chrS", 200_003)]


def serial_walk(data, start, tid):
    """The record chain from `start`: (starts of the whole records of tid, whole records seen, where it stopped, why)."""
    p, recs, seen = start, [], 0
    while p < len(data):
        if p + 4 > len(data): return recs, seen, p, OPEN
        bs = struct.unpack_from("<I", data, p)[0]
        if bs < 32: return recs, seen, p, BAD
        if p + 4 + bs > len(data): return recs, seen, p, OPEN
        rtid = struct.unpack_from("<i", data, p + 4)[0]
        seen += 1
        if rtid == tid: recs.append(p)
        elif rtid > tid or rtid < 0: return recs, seen, p, BEYOND
        p += 4 + bs
    return recs, seen, p, 0


def read_of_size(size, tid, pos, qual_byte=30, name=b"p"):
    """A plain read whose record takes exactly `size` bytes (>= 48)."""
    for l in range(max(0, (size - 48) * 2 // 3 - 4), size):
        for pad in range(0, 8):
            nm = name + b"x" * pad
            r = bu.encode_read(tid, pos, 30, 0, [("M", l)] if l else [], l, bytes([qual_byte]) * l, name=nm)
            if len(r) == size:
                return r
    raise ValueError(f"no read of {size} bytes")


def plain_reads(count, tid, pos0=10, seed=5, read_len=100):
    rng = np.random.default_rng(seed)
    out, pos = [], pos0
    for i in range(count):
        L = int(rng.integers(read_len // 2, read_len + 1))
        out.append(bu.encode_read(tid, pos, int(rng.integers(0, 61)), 0, [("M", L)], L, rng.integers(2, 41, L).astype(np.uint8).tobytes(),
                                  name=f"q{i}".encode()))
        pos += int(rng.integers(0, 9))
    return out


def fill_to(records, target, tid, pos):
    """Append reads until the stream is exactly `target` bytes long."""
    cur = sum(map(len, records))
    while target - cur > 400:
        records.append(read_of_size(150, tid, pos)); cur += 150
    if target - cur >= 96:
        records.append(read_of_size((target - cur) // 2, tid, pos)); cur += len(records[-1])
    records.append(read_of_size(target - cur, tid, pos))
    assert sum(map(len, records)) == target


def straddle_case(split):
    """A record whose length field lies `split` bytes before a seam and 4 - split behind it (split 0: it ends on the seam)."""
    recs = plain_reads(20, 0)
    fill_to(recs, SEG - split, 0, 300)
    recs += plain_reads(60, 0, pos0=400, seed=6)
    fill_to(recs, 2 * SEG - split, 0, 2000)           # and once more at the next seam
    recs += plain_reads(30, 0, pos0=2100, seed=7)
    return REFS, recs, 0


def long_record_case(size=40_000):
    recs = plain_reads(20, 0)
    fill_to(recs, SEG - 100, 0, 300)
    recs.append(read_of_size(size, 0, 500))            # covers the segments 1 and 2 whole
    recs += plain_reads(40, 0, pos0=600, seed=8)
    return REFS, recs, 0


def decoy_case():
    """Reads that carry look-alike records: three consecutive small records, fields consistent, as the quality bytes of one read and
    as the name of another, each placed right behind a seam while the read that carries them began before it -- the lowest
    plausible offset of that segment is the decoy, the true entry lies behind it."""
    fakes = b"".join(bu.encode_read(0, 700 + i, 20, 0, [("M", 10)], 10, bytes([25]) * 10, name=b"f") for i in range(3))
    recs = plain_reads(20, 0)
    # quality decoy: the carrier begins 400 bytes before the first seam; its quality starts with filler up to the seam
    L = 600
    head = 36 + 2 + 4 + (L + 1) // 2                     # bytes of the carrier in front of its quality (name "c")
    fill_to(recs, SEG - 400, 0, 300)
    lead = 400 - head                                    # quality bytes in front of the seam
    assert lead >= 0
    qual = bytes([30]) * lead + fakes + bytes([30]) * (L - lead - len(fakes))
    recs.append(bu.encode_read(0, 310, 30, 0, [("M", L)], L, qual, name=b"c"))
    recs += plain_reads(60, 0, pos0=320, seed=9)
    # name decoy: the carrier's name (behind 36 bytes of fixed fields) starts exactly on the second seam
    fill_to(recs, 2 * SEG - 36, 0, 900)
    assert len(fakes) < 250
    recs.append(bu.encode_read(0, 910, 30, 0, [("M", 50)], 50, bytes([30]) * 50, name=fakes))
    recs += plain_reads(100, 0, pos0=920, seed=10)
    return REFS, recs, 0


def beyond_case():
    recs = plain_reads(100, 0)
    fill_to(recs, SEG + 5000, 0, 3000)                    # the next chromosome begins in mid-segment
    recs += plain_reads(200, 1, seed=11)
    return REFS, recs, 0


def unplaced_case():
    recs = plain_reads(180, 0) + plain_reads(60, 1, seed=12)
    recs += [bu.encode_read(-1, -1, 0, bu.FLAG_UNMAP, [], 40, bytes([20]) * 40, name=f"u{i}".encode()) for i in range(200)]
    return REFS, recs, 1


def bad_chain_case():
    recs = plain_reads(200, 0)
    recs.append(struct.pack("<i", 31) + bytes(31))        # block_size 31 where a record must start
    recs += plain_reads(20, 0, pos0=3000, seed=13)
    return REFS, recs, 0


def bad_body_case():
    """block_size 31 spelled inside record bodies only: never on the chain."""
    recs = plain_reads(100, 0)
    for i in range(60):
        recs.append(bu.encode_read(0, 1500 + i, 30, 0, [("M", 80)], 80, (struct.pack("<i", 31) * 20), name=b"b"))
    recs += plain_reads(250, 0, pos0=1600, seed=14)
    return REFS, recs, 0


def cut_case():
    recs = plain_reads(300, 0)
    recs.append(plain_reads(1, 0, pos0=5000, seed=15)[0][:57])   # the stream ends inside a record
    return REFS, recs, 0


def cases():
    """name -> (refs, records, tid).  `bad_chain` is the one whose chain is broken (flags BAD, a load error)."""
    out = {f"straddle{k}": straddle_case(k) for k in (1, 2, 3)}
    out["ends_on_seam"] = straddle_case(0)
    out["long_record"] = long_record_case()
    out["decoys"] = decoy_case()
    out["beyond"] = beyond_case()
    out["unplaced"] = unplaced_case()
    out["bad_chain"] = bad_chain_case()
    out["bad_body"] = bad_body_case()
    out["cut"] = cut_case()
    out["empty"] = (REFS, [], 0)
    return out
