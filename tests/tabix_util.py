"""The tabix (.tbi) and CSI (.csi) index formats and BGZF virtual offsets, restated for the tests from the published layouts:
binning, parsers and writers, a member walk that resolves a virtual offset to a text offset, a region query as a tabix reader
does it, and the index that the rules of DESIGN.md 6i give for a BGZF file of bedGraph lines.  Nothing but zlib, struct and
bgzf_walk.members."""
import gzip
import struct
import zlib

import bgzf_walk as bw
from bgzf_util import EOF_BLOCK, bgzf

TBI_PSEUDO_BIN = 37450


def pseudo_bin(depth):
    return ((1 << 3 * (depth + 1)) - 1) // 7 + 1


def reg2bin(beg, end, min_shift=14, depth=5):
    """The bin of the 0-based half-open [beg, end): the smallest one that holds it whole."""
    end -= 1
    s, t = min_shift, ((1 << depth * 3) - 1) // 7
    for l in range(depth, 0, -1):
        if beg >> s == end >> s:
            return t + (beg >> s)
        s += 3
        t -= 1 << (l - 1) * 3
    return 0


def reg2bins(beg, end, min_shift=14, depth=5):
    """Every bin that can hold a line overlapping [beg, end)."""
    end -= 1
    out, t, s = [], 0, min_shift + depth * 3
    for l in range(depth + 1):
        out += list(range(t + (beg >> s), t + (end >> s) + 1))
        s -= 3
        t += 1 << l * 3
    return out


# ---- the files ----
# An index here: dict(kind="tbi" | "csi", min_shift, depth, names=[...], refs=[dict(bins={bin: [(beg, end), ...]}, linear=[...],
# loffset={bin: voff})]); linear is what a .tbi holds, loffset what a .csi holds.

def _header(names):
    nm = b"".join(n.encode() + b"\0" for n in names)
    return struct.pack("<7i", 0x10000, 1, 2, 3, ord("#"), 0, len(nm)) + nm


def _bins_bytes(ref, csi, pseudo):
    bins = dict(ref["bins"])
    out = [struct.pack("<i", len(bins) + (1 if pseudo is not None else 0))]
    for b in sorted(bins):
        out.append(struct.pack("<I", b))
        if csi:
            out.append(struct.pack("<Q", ref["loffset"][b]))
        out.append(struct.pack("<i", len(bins[b])))
        out += [struct.pack("<QQ", beg, end) for beg, end in bins[b]]
    if pseudo is not None:   # two "chunks": the reference's range in the file, and its mapped / unmapped counts
        lo = min(c[0] for cs in bins.values() for c in cs)
        hi = max(c[1] for cs in bins.values() for c in cs)
        out.append(struct.pack("<I", pseudo) + (struct.pack("<Q", 0) if csi else b"") + struct.pack("<iQQQQ", 2, lo, hi, 7, 0))
    return b"".join(out)


def tbi_bytes(index, pseudo=False, n_no_coor=None):
    """The .tbi stream of an index, before compression."""
    out = [b"TBI\1", struct.pack("<i", len(index["names"])), _header(index["names"])]
    for ref in index["refs"]:
        out.append(_bins_bytes(ref, False, TBI_PSEUDO_BIN if pseudo else None))
        out.append(struct.pack("<i", len(ref["linear"])) + b"".join(struct.pack("<Q", v) for v in ref["linear"]))
    if n_no_coor is not None:
        out.append(struct.pack("<Q", n_no_coor))
    return b"".join(out)


def csi_bytes(index, pseudo=False, n_no_coor=None):
    aux = _header(index["names"])
    out = [b"CSI\1", struct.pack("<3i", index["min_shift"], index["depth"], len(aux)), aux, struct.pack("<i", len(index["names"]))]
    for ref in index["refs"]:
        out.append(_bins_bytes(ref, True, pseudo_bin(index["depth"]) if pseudo else None))
    if n_no_coor is not None:
        out.append(struct.pack("<Q", n_no_coor))
    return b"".join(out)


def write_index(path, index, **kw):
    raw = csi_bytes(index, **kw) if index["kind"] == "csi" else tbi_bytes(index, **kw)
    with open(path, "wb") as f:
        f.write(bgzf(raw))


class _Reader:
    def __init__(self, raw):
        self.raw, self.p = raw, 0

    def take(self, fmt):
        size = struct.calcsize(fmt)
        if self.p + size > len(self.raw):
            raise ValueError("index: truncated")
        v = struct.unpack_from(fmt, self.raw, self.p)
        self.p += size
        return v

    def bytes(self, n):
        if n < 0 or self.p + n > len(self.raw):
            raise ValueError("index: truncated")
        self.p += n
        return self.raw[self.p - n:self.p]


def parse_raw(raw):
    """The stream of a .tbi or .csi, field by field; pseudo-bins are kept apart (ref["pseudo"])."""
    r = _Reader(raw)
    magic = r.bytes(4)
    if magic == b"TBI\1":
        kind, min_shift, depth = "tbi", 14, 5
        (n_ref,) = r.take("<i")
        fmt, col_seq, col_beg, col_end, meta, skip, l_nm = r.take("<7i")
        names = r.bytes(l_nm)
    elif magic == b"CSI\1":
        kind = "csi"
        min_shift, depth, l_aux = r.take("<3i")
        aux = _Reader(r.bytes(l_aux))
        fmt, col_seq, col_beg, col_end, meta, skip, l_nm = aux.take("<7i")
        names = aux.bytes(l_nm)
        (n_ref,) = r.take("<i")
    else:
        raise ValueError("index: neither TBI nor CSI")
    names = [n.decode() for n in names.split(b"\0")[:-1]]
    if len(names) != n_ref:
        raise ValueError("index: names and n_ref differ")
    pseudo = TBI_PSEUDO_BIN if kind == "tbi" else pseudo_bin(depth)
    refs = []
    for _ in range(n_ref):
        ref = dict(bins={}, loffset={}, linear=[], pseudo=None, order=[])
        (n_bin,) = r.take("<i")
        for _ in range(n_bin):
            (b,) = r.take("<I")
            if kind == "csi":
                (lo,) = r.take("<Q")
            (n_chunk,) = r.take("<i")
            chunks = [r.take("<QQ") for _ in range(n_chunk)]
            if b == pseudo:
                ref["pseudo"] = chunks
                continue
            ref["order"].append(b)
            ref["bins"][b] = chunks
            if kind == "csi":
                ref["loffset"][b] = lo
        if kind == "tbi":
            (n_intv,) = r.take("<i")
            ref["linear"] = [r.take("<Q")[0] for _ in range(n_intv)]
        refs.append(ref)
    rest = len(raw) - r.p
    if rest not in (0, 8):
        raise ValueError("index: bytes behind the last reference")
    return dict(kind=kind, min_shift=min_shift, depth=depth, names=names, refs=refs,
                header=dict(format=fmt, col_seq=col_seq, col_beg=col_beg, col_end=col_end, meta=meta, skip=skip), trailing=rest)


def parse_index(path):
    with open(path, "rb") as f:
        data = f.read()
    assert data[-28:] == EOF_BLOCK
    bw.members(data[:-28])                 # a well-formed BGZF file
    return parse_raw(gzip.decompress(data))


# ---- virtual offsets ----

def member_table(data):
    """The members of a BGZF file (an end-of-file block, if there, is left out): [(file offset, size, text offset, text)]."""
    body = data[:-28] if data[-28:] == EOF_BLOCK else data
    out, off, toff = [], 0, 0
    for m in bw.members(body):
        out.append((off, m["size"], toff, m["text"]))
        off += m["size"]
        toff += len(m["text"])
    return out


def table_ends(table):
    return (table[-1][0] + table[-1][1], table[-1][2] + len(table[-1][3])) if table else (0, 0)


def resolve(voff, table):
    """A virtual offset as an offset into the file's text; the file's end (where an end-of-file block would begin) is the text's end."""
    coff, uoff = voff >> 16, voff & 0xFFFF
    for off, size, toff, text in table:
        if off == coff:
            assert uoff < len(text) or (uoff == len(text) == 0), (voff, uoff, len(text))
            return toff + uoff
    fend, tend = table_ends(table)
    assert coff == fend and uoff == 0, f"virtual offset {voff:#x}: no member begins at {coff}"
    return tend


def to_voff(t, table):
    """The virtual offset of text offset t: in the member that holds the byte, or, for the text's end, the file's end."""
    for off, size, toff, text in table:
        if toff <= t < toff + len(text):
            return off << 16 | (t - toff)
    fend, tend = table_ends(table)
    assert t == tend, (t, tend)
    return fend << 16


# ---- what the index of a file must be ----

def parse_lines(text):
    """[(name, start, end, text offset, text offset behind it)] of bedGraph text."""
    out, p = [], 0
    for line in text.split(b"\n")[:-1]:
        f = line.split(b"\t")
        out.append((f[0].decode(), int(f[1]), int(f[2]), p, p + len(line) + 1))
        p += len(line) + 1
    assert p == len(text)
    return out


def expected_index(text, table=None, min_shift=14, depth=5):
    """Per chromosome, in file order: the chunks (a new one wherever a line's bin differs from the line's before; the last
    ends behind the chromosome's last line) per bin, and linear[w] = the first line whose end lies beyond w << min_shift --
    all as text offsets.  Returns {name: dict(chunks={bin: [(beg, end)]}, linear=[...], bin_of={text offset: bin})}."""
    out = {}
    for name, s, e, p, q in parse_lines(text):
        assert e > s >= 0
        b = reg2bin(s, e, min_shift, depth)
        if name not in out:
            out[name] = dict(chunks={}, linear=[], last=None, bin_of={})
        ref = out[name]
        ref["bin_of"][p] = b
        if ref["last"] is not None and ref["last"][0] == b:
            ref["last"][2] = q
        else:
            ref["last"] = [b, p, q]
            ref["chunks"].setdefault(b, []).append(ref["last"])
        while len(ref["linear"]) <= (e - 1) >> min_shift:
            ref["linear"].append(p)
    for ref in out.values():
        del ref["last"]
        ref["chunks"] = {b: [(c[1], c[2]) for c in cs] for b, cs in ref["chunks"].items()}
    return out


def resolved(index, table):
    """A parsed index in the form of expected_index (without bin_of)."""
    out = {}
    for name, ref in zip(index["names"], index["refs"]):
        out[name] = dict(chunks={b: [(resolve(x, table), resolve(y, table)) for x, y in cs] for b, cs in ref["bins"].items()},
                         linear=[resolve(v, table) for v in ref["linear"]])
    return out


def build_index(text, table, kind="tbi", min_shift=14, depth=5):
    """The index of a file, for fixtures: expected_index in virtual offsets."""
    exp = expected_index(text, table, min_shift, depth)
    refs = []
    for name, ref in exp.items():
        lin = [to_voff(t, table) for t in ref["linear"]]
        bins = {b: [(to_voff(x, table), to_voff(y, table)) for x, y in cs] for b, cs in ref["chunks"].items()}
        lo = {}
        for b in bins:   # a .csi keeps, per bin, the linear index's entry for the bin's first window
            s, t = min_shift, ((1 << depth * 3) - 1) // 7
            while b < t:
                s += 3
                t = (t - 1) // 8
            first = (b - t) << (s - min_shift)
            lo[b] = lin[min(first, len(lin) - 1)]
        refs.append(dict(bins=bins, linear=lin, loffset=lo))
    return dict(kind=kind, min_shift=min_shift, depth=depth, names=list(exp), refs=refs)


# ---- a reader ----

def text_range(table, tb, te, touched):
    """text[tb, te) from the members that hold it, noting which were opened."""
    out = []
    for k, (off, size, toff, text) in enumerate(table):
        if toff < te and toff + len(text) > tb:
            touched.add(k)
            out.append(text[max(tb - toff, 0):te - toff])
    return b"".join(out)


def query(data, index, name, beg, end, table=None):
    """The lines of `name` that overlap [beg, end), as a tabix reader finds them: the chunks of the bins that can hold such a
    line, cut below the linear index's entry for beg, inflated, filtered.  Returns (lines, members opened)."""
    table = table if table is not None else member_table(data)
    touched = set()
    if name not in index["names"] or end <= beg:
        return [], touched
    ref = index["refs"][index["names"].index(name)]
    ms, depth = index["min_shift"], index["depth"]
    if index["kind"] == "tbi":
        if beg >> ms >= len(ref["linear"]):
            return [], touched                 # no line reaches that far
        floor = ref["linear"][beg >> ms]
    else:
        floor = 0
    chunks = []
    for b in reg2bins(beg, end, ms, depth):
        for x, y in ref["bins"].get(b, []):
            if y > floor:
                chunks.append((max(x, floor), y))
    lines = []
    for x, y in sorted(chunks):
        tb, te = resolve(x, table), resolve(y, table)
        for line in text_range(table, tb, te, touched).split(b"\n")[:-1]:
            f = line.split(b"\t")
            if f[0].decode() == name and int(f[1]) < end and int(f[2]) > beg:
                lines.append(line)
    return lines, touched


_PARSED = {}


def overlapping(text, name, beg, end):
    """The lines of `text` that overlap [beg, end) of `name`, by a scan of every line (parsed once per text)."""
    key = (len(text), hash(text))
    if key not in _PARSED:
        _PARSED.clear()
        _PARSED[key] = parse_lines(text)
    return [text[p:q - 1] for nm, s, e, p, q in _PARSED[key] if nm == name and s < end and e > beg]
