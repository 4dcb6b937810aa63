"""A bit-level deflate writer for the tests: any stream RFC 1951 allows, and the malformed ones next to them.  zlib's
compressor uses a narrow part of the format (literal and distance length lists spelled apart, two distance codes at least,
short codes on our texts), so the inputs it makes never reach the decoder's long codes, its repeats across the HLIT / HDIST
seam, its incomplete distance sets or most of the (len, dist) pairs of a match copy.  The streams here are assembled by hand:
stored, fixed and dynamic blocks with chosen code lengths, a chosen spelling of the length list, chosen code-length-code
lengths and HCLEN, and a token list of literals and matches.

    crafted_cases()   [(id, BGZF bytes, text)]      valid files; text is the tokens expanded here, CRC32 and ISIZE are zlib's
    crafted_specs()   {id: [[block spec] per member]}  the tables every block was written from
    refused_cases()   [(id, BGZF member, reason)]   malformed members and the decoder's verdict (rsinf::err_name)
    reader_case(text) (BGZF bytes, bit offsets)     a depth text in crafted members, for the readers

Pure Python, zlib and struct."""
import random
import struct
import zlib

SEED = 20251
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
HEAD = b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00"

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in (0, 1)]
CLEN_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32
LADDER = list(range(1, 16)) + [15]          # a complete code with every length 1..15 and two 15-bit codes


# ---------------------------------------------------------------------------------------------------------------------
# tables
# ---------------------------------------------------------------------------------------------------------------------

def canon(lengths):
    """The canonical codes of RFC 1951 3.2.2: code[s] for every s with lengths[s] > 0."""
    count = [0] * 17
    for l in lengths:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for l in range(1, 17):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    codes = [None] * len(lengths)
    for s, l in enumerate(lengths):
        if l:
            codes[s] = nxt[l]
            nxt[l] += 1
    return codes


def kraft(lengths):
    """Sum of 2^-l in units of 2^-15: 32768 for a complete set."""
    return sum(1 << (15 - l) for l in lengths if l)


def flat_lengths(n, used):
    """lengths[0..n): a complete code over `used` (in that order: the first get the shorter codes); one symbol gets one bit."""
    out, k = [0] * n, len(used)
    if k == 1:
        out[used[0]] = 1
        return out
    d = (k - 1).bit_length()
    short = (1 << d) - k
    for i, s in enumerate(used):
        out[s] = d - 1 if i < short else d
    return out


def len_symbol(length, sym=None):
    """(symbol, extra bits, extra value) of a match length; sym forces one of two spellings (258 as 284 + 31)."""
    if sym is None:
        i = 28 if length == 258 else max(j for j in range(28) if LEN_BASE[j] <= length)
    else:
        i = sym - 257
    e = length - LEN_BASE[i]
    assert 0 <= e < (1 << LEN_EXTRA[i]) or (e == 0 and LEN_EXTRA[i] == 0), (length, sym)
    return 257 + i, LEN_EXTRA[i], e


def dist_symbol(dist):
    i = max(j for j in range(30) if DIST_BASE[j] <= dist)
    return i, DIST_EXTRA[i], dist - DIST_BASE[i]


def len_range(sym):
    i = sym - 257
    return LEN_BASE[i], (258 if i == 28 else LEN_BASE[i] + (1 << LEN_EXTRA[i]) - 1 - (i == 27))   # 284 + 31 is left to force


def dist_range(sym):
    return DIST_BASE[sym], DIST_BASE[sym] + (1 << DIST_EXTRA[sym]) - 1


def expand_spelling(spelling):
    """The lengths a spelling gives: an int is a length, ("r16", n) repeats the length before n times (3-6), ("r17", n)
    and ("r18", n) are n zeros (3-10, 11-138)."""
    out = []
    for it in spelling:
        if isinstance(it, int):
            out.append(it)
        elif it[0] == "r16":
            out += [out[-1]] * it[1]
        else:
            out += [0] * it[1]
    return out


def auto_spelling(lengths):
    """Greedy run-length spelling of the whole list, as a compressor that joins the two lists writes it: runs cross the seam."""
    out, i, n = [], 0, len(lengths)
    while i < n:
        j = i
        while j < n and lengths[j] == lengths[i]:
            j += 1
        run, v = j - i, lengths[i]
        if v == 0:
            while run >= 11:
                k = min(run, 138)
                out.append(("r18", k)); run -= k
            if run >= 3:
                out.append(("r17", run)); run = 0
            out += [0] * run
        else:
            out.append(v); run -= 1
            while run >= 3:
                k = min(run, 6)
                out.append(("r16", k)); run -= k
            out += [v] * run
        i = j
    return out


def spelling_runs(spelling):
    """[(kind, first index, count)] of the repeat symbols of a spelling."""
    runs, idx = [], 0
    for it in spelling:
        if isinstance(it, int):
            idx += 1
        else:
            runs.append((it[0], idx, it[1]))
            idx += it[1]
    return runs


# ---------------------------------------------------------------------------------------------------------------------
# the writer
# ---------------------------------------------------------------------------------------------------------------------

class BitWriter:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def bits(self, v, k):
        """k bits of v, least significant first (header fields, extra bits)."""
        self.acc |= (v & ((1 << k) - 1)) << self.n
        self.n += k
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, c, k):
        """A Huffman code of k bits, most significant first."""
        self.bits(int(format(c, "0%db" % k)[::-1], 2), k)

    @property
    def bitpos(self):
        return len(self.out) * 8 + self.n

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)


class Stream:
    """One raw deflate stream.  Tokens: an int is a literal, (len, dist) a match, (len, dist, lsym) a match with its length
    symbol forced; ("bits", v, k), ("lit", sym) and ("dist", sym) write raw bits or a bare symbol (malformed streams).
    text is the tokens expanded (None once a token cannot be: a distance too far); blocks records what each block was
    written from."""

    def __init__(self):
        self.w, self.blocks, self.text = BitWriter(), [], bytearray()

    def payload(self):
        w = self.w
        return bytes(w.out) + (bytes([w.acc]) if w.n else b"")

    def raw(self, v, k):
        self.w.bits(v, k)
        return self

    def stored(self, data, final=False, nlen=None):
        w = self.w
        w.bits(int(final), 1); w.bits(0, 2)
        at = w.bitpos
        w.align()
        w.bits(len(data), 16)
        w.bits(~len(data) & 0xFFFF if nlen is None else nlen, 16)
        w.out += data
        if self.text is not None:
            self.text += data
        self.blocks.append(dict(type="stored", final=final, header_end_bit=at, n=len(data), end_bit=w.bitpos))
        return self

    def fixed(self, tokens, final=False):
        w = self.w
        w.bits(int(final), 1); w.bits(1, 2)
        self._tokens(tokens, FIXED_LIT, FIXED_DIST)
        self.blocks.append(dict(type="fixed", final=final, tokens=tokens, end_bit=w.bitpos))
        return self

    def dynamic(self, tokens, lit_len, dist_len, final=False, spelling=None, cl_len=None, hclen=None, check=True, stop=None):
        """stop="header" / "cl": nothing behind HLIT HDIST HCLEN / behind the code-length-code lengths (malformed streams);
        check=False lets the spelling disagree with the lists (a repeat past the end, a 16 in front)."""
        w = self.w
        lengths = list(lit_len) + list(dist_len)
        if spelling is None:
            spelling = list(lengths)
        if check:
            assert expand_spelling(spelling) == lengths, "the spelling does not give the length lists"
        syms = [(it, 0, 0) if isinstance(it, int) else
                {"r16": (16, 2, it[1] - 3), "r17": (17, 3, it[1] - 3), "r18": (18, 7, it[1] - 11)}[it[0]] for it in spelling]
        if cl_len is None:
            used = sorted({s for s, _, _ in syms})
            cl_len = flat_lengths(19, used if len(used) > 1 else used + [s for s in (0, 1) if s not in used][:1])
        if hclen is None:
            hclen = max(4, max(i for i in range(19) if cl_len[CLEN_ORDER[i]]) + 1)
        assert all(cl_len[CLEN_ORDER[i]] == 0 for i in range(hclen, 19)), "HCLEN cuts a code-length code off"
        w.bits(int(final), 1); w.bits(2, 2)
        w.bits(len(lit_len) - 257, 5); w.bits(len(dist_len) - 1, 5); w.bits(hclen - 4, 4)
        spec = dict(type="dynamic", final=final, tokens=tokens, lit_len=list(lit_len), dist_len=list(dist_len), spelling=spelling,
                    cl_len=list(cl_len), hclen=hclen)
        self.blocks.append(spec)
        if stop == "header":
            return self
        for i in range(hclen):
            w.bits(cl_len[CLEN_ORDER[i]], 3)
        if stop == "cl":
            return self
        cl_codes = canon(cl_len)
        for s, nb, ev in syms:
            w.code(cl_codes[s], cl_len[s])
            w.bits(ev, nb)
        self._tokens(tokens, lit_len, dist_len)
        spec["end_bit"] = w.bitpos
        return self

    def _tokens(self, tokens, lit_len, dist_len):
        w, lc, dc, t = self.w, canon(lit_len), canon(dist_len), self.text
        for tok in tokens:
            if isinstance(tok, int):
                w.code(lc[tok], lit_len[tok])
                if t is not None:
                    t.append(tok)
            elif tok[0] == "bits":
                w.bits(tok[1], tok[2])
            elif tok[0] == "lit":
                w.code(lc[tok[1]], lit_len[tok[1]])
            elif tok[0] == "dist":
                w.code(dc[tok[1]], dist_len[tok[1]])
            elif tok[0] == "noeob":
                continue
            else:
                length, dist = tok[0], tok[1]
                s, nb, ev = len_symbol(length, tok[2] if len(tok) > 2 else None)
                w.code(lc[s], lit_len[s]); w.bits(ev, nb)
                s, nb, ev = dist_symbol(dist)
                w.code(dc[s], dist_len[s]); w.bits(ev, nb)
                if t is not None and dist > len(t):
                    t = self.text = None
                if t is not None:
                    t += t[-dist:len(t) - dist + length] if dist >= length else (bytes(t[-dist:]) * (length // dist + 1))[:length]
        if lit_len[256] and ("noeob",) not in tokens:
            w.code(lc[256], lit_len[256])


def wrap(cdata, isize=None, crc=None):
    """A BGZF member around a deflate stream; CRC32 and ISIZE from zlib's inflate of it unless given."""
    if isize is None or crc is None:
        text = zlib.decompress(cdata, -15)
        isize = len(text) if isize is None else isize
        crc = zlib.crc32(text) & 0xFFFFFFFF if crc is None else crc
    bsize = len(HEAD) + 2 + len(cdata) + 8
    assert bsize <= 65536, bsize
    return HEAD + struct.pack("<H", bsize - 1) + cdata + struct.pack("<II", crc, isize)


def used_symbols(tokens):
    """(literal/length symbols, distance symbols) the tokens use, the end-of-block code included."""
    lit, dist = {256}, set()
    for tok in tokens:
        if isinstance(tok, int):
            lit.add(tok)
        elif isinstance(tok[0], int):
            lit.add(len_symbol(tok[0], tok[2] if len(tok) > 2 else None)[0])
            dist.add(dist_symbol(tok[1])[0])
    return lit, dist


def match_positions(blocks):
    """[(op, len, dist)] of every match of a member, op the output position it starts at."""
    op, out = 0, []
    for b in blocks:
        if b["type"] == "stored":
            op += b["n"]
            continue
        for tok in b["tokens"]:
            if isinstance(tok, int):
                op += 1
            elif isinstance(tok[0], int):
                out.append((op, tok[0], tok[1]))
                op += tok[0]
    return out


# ---------------------------------------------------------------------------------------------------------------------
# valid cases
# ---------------------------------------------------------------------------------------------------------------------

def _rand_bytes(rng, n):
    return rng.getrandbits(8 * n).to_bytes(n, "little") if n else b""


def _fill_to(tokens, op, target):
    """Distance-1 matches of 258 bytes, then a shorter one or two literals, until `target` bytes exist."""
    while op < target:
        k = min(258, target - op)
        if k >= 3:
            tokens.append((k, 1)); op += k
        else:
            tokens.append(tokens[0]); op += 1
    return op


def _ladder_block(rng, cl19=False):
    """One dynamic block whose literal/length and distance codes both have the lengths 1..15 with two 15-bit codes, every
    code used; cl19: HCLEN 19 and a code-length code of 2 to 7 bits, the 7-bit ones on symbols the list uses."""
    lits = rng.sample(range(256), 10)
    lsyms = [285] + rng.sample(range(257, 285), 4)
    syms = lits + [256] + lsyms
    rng.shuffle(syms)
    lit_len = [0] * 286
    for s, l in zip(syms, LADDER):
        lit_len[s] = l
    dsyms = [0] + rng.sample(range(1, 30), 15)
    rng.shuffle(dsyms)
    dist_len = [0] * (max(dsyms) + 1)
    for s, l in zip(dsyms, LADDER):
        dist_len[s] = l
    tokens = [lits[0]] + [(258, 1)] * 127 + lits               # 32768 bytes in front: every distance is within reach
    for i, d in enumerate(dsyms):
        ls = lsyms[i % len(lsyms)]
        tokens.append((rng.randint(*len_range(ls)), rng.randint(*dist_range(d))))
    kw = {}
    if cl19:
        spelling = auto_spelling(lit_len + dist_len)
        freq = {}
        for it in spelling:
            s = it if isinstance(it, int) else int(it[0][1:])
            freq[s] = freq.get(s, 0) + 1
        used = sorted(freq, key=lambda s: -freq[s])
        unused = [s for s in range(19) if s not in freq]
        ladder = [2, 2, 3] + [5] * 9 + [6] * 5 + [7, 7]
        cl_len = [0] * 19
        order = used[:-2] + unused + used[-2:]
        for s, l in zip(order, ladder):
            cl_len[s] = l
        kw = dict(spelling=spelling, cl_len=cl_len, hclen=19)
    return tokens, lit_len, dist_len, kw


def _geometry_member(rng, dist):
    """`dist` random bytes, then a match of every length 3..258 at that distance, in a drawn order."""
    lens = list(range(3, 259))
    rng.shuffle(lens)
    return Stream().fixed(list(_rand_bytes(rng, dist)) + [(l, dist) for l in lens], final=True)


def _build():
    rng = random.Random(SEED)
    cases = []

    def add(cid, streams):
        streams = streams if isinstance(streams, list) else [streams]
        data = b"".join(wrap(s.payload()) for s in streams) + EOF_BLOCK
        cases.append((cid, data, b"".join(bytes(s.text) for s in streams), [s.blocks for s in streams]))

    # ---- code shapes ----
    tokens, lit_len, dist_len, kw = _ladder_block(rng)
    add("codes_1_to_15", Stream().dynamic(tokens, lit_len, dist_len, final=True))
    tokens, lit_len, dist_len, kw = _ladder_block(rng, cl19=True)
    add("hclen19_7bit_clcodes", Stream().dynamic(tokens, lit_len, dist_len, final=True, **kw))

    order = list(range(286))
    rng.shuffle(order)
    lit_len = flat_lengths(286, order)
    dorder = list(range(30))
    rng.shuffle(dorder)
    dist_len = flat_lengths(30, dorder)
    tokens = list(range(256))
    rng.shuffle(tokens)
    _fill_to(tokens, 256, 32768)
    edge = {28: [16385, 24576], 29: [24577, 32768]}
    for d in range(30):
        for dist in edge.get(d, [rng.randint(*dist_range(d))]):
            tokens.append((rng.randint(*len_range(257 + (len(tokens) % 29))), dist))
    for ls in range(257, 286):
        tokens.append((rng.randint(*len_range(ls)), rng.randint(1, 32768)))
    add("hlit286_hdist30_all_codes", Stream().dynamic(tokens, lit_len, dist_len, final=True))

    lits = rng.sample(range(256), 37)
    body = [rng.choice(lits) for _ in range(500)] + lits
    add("hlit257_hdist1", Stream().dynamic(body, flat_lengths(257, lits + [256]), [1], final=True))
    add("no_distance_code", Stream().dynamic(body[::-1], flat_lengths(257, [256] + lits), [0], final=True))

    # HCLEN 5 is the smallest a valid block can have: the first four entries are 16, 17, 18 and 0, which alone spell no
    # code at all (HCLEN 4 is among the refused cases)
    lit_len = [8] * 255 + [0, 8]
    spelling = [8] + [("r16", 6)] * 41 + [("r16", 5), ("r16", 3), 0, 8, 0]
    body = [rng.randrange(255) for _ in range(700)]
    add("hclen5_smallest", Stream().dynamic(body, lit_len, [0], final=True, spelling=spelling, hclen=5))

    s = Stream().stored(b"before ").dynamic([], [0] * 256 + [1], [0]).fixed(list(b"between "))
    s.dynamic([], [0] * 256 + [1], [0]).dynamic([], [0] * 256 + [1], [0], final=True)
    add("lone_end_of_block_code", s)

    # ---- the spelling of the length list ----
    lits = rng.sample(range(97, 123), 14)
    lit_len = flat_lengths(270, lits + [256, 257])               # 16 codes of 4 bits; 258..269 sent as zeros
    dist_len = [0] * 5 + [1, 1]
    spelling = lit_len[:258] + [("r18", 17), 1, 1]
    body = [rng.choice(lits) for _ in range(40)] + [(3, 7), (3, 9), lits[0], (3, 8), (3, 12)]
    add("zero_run_18_across_seam", Stream().dynamic(body, lit_len, dist_len, final=True, spelling=spelling))

    lit_len = flat_lengths(260, lits + [256, 257])               # 258, 259 zero
    dist_len = [0] * 3 + [1, 1]
    spelling = lit_len[:258] + [("r17", 5), 1, 1]
    body = [rng.choice(lits) for _ in range(40)] + [(3, 4), (3, 5), lits[1], (3, 6), (3, 4)]
    add("zero_run_17_across_seam", Stream().dynamic(body, lit_len, dist_len, final=True, spelling=spelling))

    lits = rng.sample(range(48, 58), 10) + rng.sample(range(97, 123), 17)
    lit_len = flat_lengths(286, lits + [256, 282, 283, 284, 285])            # 32 codes of 5 bits, the last four at 282..285
    dist_len = [5] * 28 + [4, 4]
    body = [rng.choice(lits) for _ in range(300)] + [(rng.randint(*len_range(ls)), rng.randint(1, 300)) for ls in (282, 283, 284, 285) * 3]
    body += [(258, 1)] * 130 + [(200, 16385 + 77), (230, 24577 + 5)]
    spelling = lit_len[:283] + [("r16", 6)] + dist_len[3:]
    add("copy_run_16_across_seam", Stream().dynamic(body, lit_len, dist_len, final=True, spelling=spelling))
    spelling = lit_len + [("r16", 6)] + dist_len[6:]
    add("copy_run_16_from_last_literal_length", Stream().dynamic(body, lit_len, dist_len, final=True, spelling=spelling))

    spelling = ([("r18", 138), 4, ("r16", 3), ("r17", 3), 4, ("r16", 6), ("r17", 10), 4, ("r18", 11), 4, ("r18", 81), 4, 4, 4, 1, 1])
    lengths = expand_spelling(spelling)
    lit_len, dist_len = lengths[:259], lengths[259:]
    lits = [i for i in range(256) if lit_len[i]]
    body = [rng.choice(lits) for _ in range(200)] + lits + [(3, 1), (4, 2), (3, 2), (4, 1)]
    add("runs_of_3_6_10_11_138", Stream().dynamic(body, lit_len, dist_len, final=True, spelling=spelling))

    # ---- distance sets ----
    lits = rng.sample(range(256), 20)
    lit_len = flat_lengths(286, lits + [256] + list(range(257, 286)))
    body = list(lits) + [(rng.randint(3, 258), rng.randint(13, 16)) for _ in range(60)]
    add("one_distance_code_of_1_bit", Stream().dynamic(body, lit_len, [0] * 7 + [1], final=True))

    # ---- length 258, both spellings ----
    body = list(_rand_bytes(rng, 300))
    for d in (1, 2, 63, 64, 65, 257, 258, 259, 300):
        body += [(258, d), (258, d, 284), rng.randrange(256)]
    add("length_258_as_285_and_as_284_31", Stream().fixed(body, final=True))

    # ---- copy geometry ----
    add("every_len_at_dist_1_to_130", [_geometry_member(rng, d) for d in range(1, 131)])
    add("every_len_at_dist_255_256_257", [_geometry_member(rng, d) for d in (255, 256, 257)])

    body = []
    for l in list(range(3, 70)) + [127, 128, 129, 257, 258]:
        body += [rng.randrange(256), (l, 1), rng.randrange(256), rng.randrange(256), (l, 2)]
    add("match_after_literal_dist_1_2", Stream().fixed(body, final=True))

    body, prev = list(_rand_bytes(rng, 80)) + [(70, 80)], 70
    for _ in range(150):
        l, d = rng.randint(3, 258), rng.randint(1, prev)
        body.append((l, d))
        prev = l
    add("match_from_previous_match_tail", Stream().fixed(body, final=True))

    s = Stream().fixed([200, 201, 202])                        # three 9-bit literals: the stored header ends at bit 0
    s.stored(_rand_bytes(rng, 500))
    s.fixed([(258, 500), (3, 258 + 500 - 3), (64, 322 + 400), (100, 386 + 100)] + [203], final=False)
    s.stored(_rand_bytes(rng, 70))
    s.fixed([(70, 70), (258, 140), (5, 5)], final=True)
    add("match_from_stored_bytes", s)

    s = Stream().stored(_rand_bytes(rng, 32768))
    body, op = [(258, 32768)], 32768 + 258
    while op < 65536 - 258 - 300:
        l, d = rng.randint(3, 258), rng.randint(1, 32768)
        body.append((l, d)); op += l
    while op < 65536 - 258:
        l = min(258, 65536 - 258 - op)
        body.append((l, rng.randint(1, 32768)) if l >= 3 else rng.randrange(256)); op += l if l >= 3 else 1
    body.append((258, 32768))
    add("dist_32768_at_op_32768_and_end_on_65536", s.fixed(body, final=True))

    # ---- the bit reader ----
    members = []
    for behind in (1, 300):
        for k in range(8):                                       # k 9-bit literals: the stored header ends at bit (5 + k) % 8
            s = Stream().fixed([144 + rng.randrange(112) for _ in range(k)])
            s.stored(_rand_bytes(rng, behind), final=behind == 1)
            if behind != 1:
                s.fixed([150, 97, (20, 40)]).stored(_rand_bytes(rng, 3)).fixed([98], final=True)
            members.append(s)
    add("stored_at_every_bit_offset", members)

    s = Stream().stored(b"").stored(b"").fixed(list(b"first ")).stored(b"").fixed(list(b"second")).stored(b"ab").stored(b"", final=True)
    add("empty_stored_first_middle_final", s)
    add("empty_stored_alone", Stream().stored(b"", final=True))

    add("final_block_padding_0_to_7", [Stream().fixed([97 + j] * 3 + [144 + rng.randrange(112) for _ in range(j)], final=True) for j in range(8)])

    s = Stream()
    for i in range(3000):
        s.fixed([rng.randrange(256)], final=i == 2999)
    add("3000_one_literal_blocks", s)

    # ---- ISIZE and CRC: every slice geometry of the 64-lane CRC, some 210 members in one launch ----
    members = []
    for n in list(range(201)) + [4095, 4096, 4097]:
        data = _rand_bytes(rng, n)
        members.append(Stream().stored(data, final=True) if n % 3 else Stream().fixed(list(data), final=True))
    for n in (65535, 65536):                                     # too large to store in one member: 16 letters, 4- and 5-bit codes
        letters = rng.sample(range(256), 16)
        members.append(Stream().dynamic([letters[rng.getrandbits(4)] for _ in range(n)], flat_lengths(257, letters + [256]), [0], final=True))
    add("isize_0_to_200_4095_4096_4097_65535_65536", members)
    return cases


_CACHE = []


def _built():
    if not _CACHE:
        _CACHE.append(_build())
    return _CACHE[0]


def crafted_cases():
    return [(cid, data, text) for cid, data, text, _ in _built()]


def crafted_specs():
    return {cid: specs for cid, _, _, specs in _built()}


# ---------------------------------------------------------------------------------------------------------------------
# refused cases
# ---------------------------------------------------------------------------------------------------------------------

R_LENGTHS = "invalid Huffman code lengths"
R_SYMBOL = "invalid Huffman code"
FILL = [("bits", 0, 16), ("bits", 0, 16), ("noeob",)]
# zlib takes these: it stops at the end of the deflate stream and knows no ISIZE
ZLIB_ACCEPTS = ("match_one_byte_past_isize", "trailing_byte", "footer_isize_65537")


def refused_cases():
    """(id, member, reason): reason is the decoder's rsinf::err_name, which ends the device's message."""
    abc = flat_lengths(258, [97, 256, 257])                      # 'a' 1 bit, end of block and length 3 two bits
    out = []

    def bad(cid, s, reason, isize=4, crc=0, tail=b""):
        out.append((cid, wrap(s.payload() + tail, isize, crc), reason))

    bad("length_symbol_286_fixed", Stream().fixed([97, ("lit", 286)] + FILL, final=True), R_SYMBOL)
    bad("distance_symbol_30_fixed", Stream().fixed([97, ("lit", 257), ("dist", 30)] + FILL, final=True), R_SYMBOL)
    bad("distance_one_too_far", Stream().fixed([97, 98, 99, 100, 101, (3, 6)], final=True), "distance too far back", isize=8)
    s = Stream().fixed([97, 98, 99, 100, (10, 2)], final=True)
    bad("match_one_byte_past_isize", s, "more data than ISIZE", isize=13, crc=zlib.crc32(bytes(s.text)))
    two = [0] * 257
    two[97] = two[256] = 2
    bad("literal_set_incomplete", Stream().dynamic(FILL, two, [0], final=True), R_LENGTHS)
    over = [0] * 257
    over[97] = over[98] = over[256] = 1
    bad("literal_set_oversubscribed", Stream().dynamic(FILL, over, [0], final=True), R_LENGTHS)
    bad("distance_set_one_code_of_2_bits", Stream().dynamic(FILL, abc, [2], final=True), R_LENGTHS)
    bad("distance_set_oversubscribed", Stream().dynamic(FILL, abc, [1, 1, 1], final=True), R_LENGTHS)
    noeob = [0] * 257
    noeob[97] = noeob[98] = 1
    bad("no_end_of_block_code", Stream().dynamic(FILL, noeob, [0], final=True), R_LENGTHS)
    bad("first_symbol_16", Stream().dynamic(FILL, abc, [1], final=True, spelling=[("r16", 3)] + abc[3:] + [1], check=False), R_LENGTHS)
    bad("repeat_past_hlit_hdist", Stream().dynamic(FILL, abc, [1], final=True, spelling=abc + [("r18", 11)], check=False), R_LENGTHS)
    bad("hlit_287", Stream().dynamic(FILL, abc + [0] * 29, [1], final=True, stop="header").raw(0, 16).raw(0, 16), R_LENGTHS)
    bad("hdist_31", Stream().dynamic(FILL, abc, [0] * 30 + [1], final=True, stop="header").raw(0, 16).raw(0, 16), R_LENGTHS)
    cl = [0] * 19
    cl[0] = cl[1] = 2
    bad("code_length_code_incomplete", Stream().dynamic(FILL, abc, [1], final=True, cl_len=cl, stop="cl").raw(0, 16).raw(0, 16), R_LENGTHS)
    cl = [0] * 19
    cl[0] = cl[18] = 1                                           # HCLEN 4: 16, 17, 18 and 0 only, so every length is 0
    bad("hclen_4_spells_no_code", Stream().dynamic(FILL, [0] * 257, [0], final=True, spelling=[("r18", 138), ("r18", 120)],
                                                   cl_len=cl, hclen=4), R_LENGTHS)
    bad("lone_distance_code_unused_pattern", Stream().dynamic([97, ("lit", 257), ("bits", 1, 1)] + FILL, abc, [1], final=True), R_SYMBOL)
    bad("block_type_3", Stream().raw(1, 1).raw(3, 2).raw(0, 16).raw(0, 16), "invalid deflate block type")
    bad("stored_len_not_nlen", Stream().stored(b"abcd", final=True, nlen=0xFFFA), "stored block length check failed")
    s = Stream().fixed(list(b"abcd"), final=True)
    bad("trailing_byte", s, "bytes between the deflate data and the footer", crc=zlib.crc32(b"abcd"), tail=b"\x00")
    bad("footer_isize_65537", s, "ISIZE", isize=65537, crc=zlib.crc32(b"abcd"))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# a depth text in crafted members
# ---------------------------------------------------------------------------------------------------------------------

def _tokenize(text, dists):
    """Greedy matches at the given distances only, literals elsewhere."""
    out, i, n = [], 0, len(text)
    while i < n:
        best, bd = 0, 0
        for d in dists:
            if d > i:
                continue
            l = 0
            while l < 258 and i + l < n and text[i + l] == text[i + l - d]:
                l += 1
            if l > best:
                best, bd = l, d
        if best >= 3:
            out.append((best, bd)); i += best
        else:
            out.append(text[i]); i += 1
    return out


def reader_case(text, seed=SEED):
    """text (digits, tabs, line ends) as BGZF whose every member is: a dynamic block with 1- to 15-bit literal codes, a lone
    1-bit distance code and an 18 run across the seam; a stored block wherever the bits have it begin; a second such block.
    Returns (BGZF bytes, [bit offset of each stored header's end])."""
    rng = random.Random(seed)
    alphabet = sorted(set(text))
    assert len(alphabet) <= 12 and max(alphabet) < 64
    members, offsets, long_codes, p = [], [], 0, 0
    while p < len(text):
        part = text[p:p + rng.randint(300, 9000)]
        p += len(part)
        a, b = len(part) // 3, len(part) // 3 + rng.randint(0, 40)
        syms = alphabet + [256, 257, 258, 259]                   # lengths 3, 4, 5; longer matches are split by the tokenizer's cap
        syms += list(range(64, 64 + 16 - len(syms)))
        rng.shuffle(syms)
        lit_len = [0] * 270                                      # 260..269 sent as zeros, in one run with the first distance lengths
        for s_, l in zip(syms, LADDER):
            lit_len[s_] = l
        dist_len = [0] * 5 + [1]                                 # distances 7 and 8 only
        spelling = lit_len[:260] + [("r18", 15), 1]
        s = Stream()
        for piece, final in ((part[:a], False), (part[b:], True)):
            toks = []
            for t in _tokenize(piece, (7, 8)):
                if isinstance(t, int):
                    toks.append(t)
                else:                                            # lengths 3..5 only have codes: split
                    l, d = t
                    while l >= 3:
                        k = 5 if l >= 8 or l == 5 else (4 if l in (4, 7) else 3)
                        toks.append((k, d)); l -= k
                    assert l == 0
            s.dynamic(toks, lit_len, dist_len, final=final, spelling=spelling)
            long_codes += sum(1 for t in used_symbols(toks)[0] if lit_len[t] == 15)
            if not final:
                s.stored(part[a:b])
                offsets.append(s.blocks[-1]["header_end_bit"] % 8)
        assert bytes(s.text) == part
        members.append(wrap(s.payload()))
    assert long_codes, "no 15-bit code in use"
    return b"".join(members) + EOF_BLOCK, offsets
