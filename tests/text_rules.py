"""The depth-text readers' number rule, restated once for every test (rsicnv_amd/csrc/text_rules.h),
and the corpus of awkward lines that pins it to the reference (tests/golden/text_rules.npz, tools/make_golden_text_rules.py).

The reference reads a line with `istringstream iss(line); int pos, d; iss >> pos >> d;` (load_data_from_text).  With libstdc++
one extraction skips the blanks, takes an optional sign and a run of digits, gives 0 and fails without a digit, and gives the
clamped bound and fails outside the field's type; after a failure the later extractions of the line leave their (here
zero-initialised) variables alone.  The stream goes on where the previous extraction stopped: no splitting into tokens."""
import hashlib

import numpy as np

BLANK = " \t\r\v\f"


def extract(t, q, bits=32):
    """`iss >> v` on t[q:] for a `bits`-bit signed field: (ok, v, q after it)."""
    e = len(t)
    while q < e and t[q] in BLANK:
        q += 1
    neg = False
    if q < e and t[q] in "+-":
        neg = t[q] == "-"
        q += 1
    s = q
    while q < e and "0" <= t[q] <= "9":
        q += 1
    if q == s:
        return False, 0, q
    v = int(t[s:q])
    v = -v if neg else v
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    if v < lo:
        return False, lo, q
    if v > hi:
        return False, hi, q
    return True, v, q


def chain(t, k, q=0):
    """`iss >> v1 >> ... >> vk` into ints: the k values and q behind the last extraction made."""
    out, good = [], True
    for _ in range(k):
        v = 0
        if good:
            good, v, q = extract(t, q)
        out.append(v)
    return out, q


def per_base(rest):
    """A "pos d" line (the part behind the name): (pos, d)."""
    (pos, d), _ = chain(rest, 2)
    return pos, d


def columns(rest, k):
    """A cohort line's part behind the name: (pos, [d1 .. dk])."""
    vals, _ = chain(rest, k + 1)
    return vals[0], vals[1:]


def bed_fields(rest):
    """A bedGraph line's part behind the name: (start, end, d) read as long long, long long, int; None when start or end
    fails (overflow included) -- such a line stands for no per-base line."""
    ok, start, q = extract(rest, 0, 64)
    if not ok:
        return None
    ok, end, q = extract(rest, q, 64)
    if not ok:
        return None
    _, d, _ = extract(rest, q)
    return start, end, d


def split_name(line):
    """(name, rest) of a named line: leading blanks, then the bytes up to the next blank."""
    q = 0
    while q < len(line) and line[q] in BLANK:
        q += 1
    s = q
    while q < len(line) and line[q] not in BLANK:
        q += 1
    return line[s:q], line[q:]


def expand_line(line):
    """One bedGraph text line (no '\\n') -> the per-base lines "NAME p d" it stands for (small intervals only)."""
    if not line or line[0] == "#":
        return []
    name, rest = split_name(line)
    if not name or name in ("track", "browser"):
        return []
    f = bed_fields(rest)
    if f is None or f[1] <= f[0]:
        return []
    start, end, d = f
    return [f"{name}\t{p}\t{d}" for p in range(start + 1, end + 1)]


def data_lines(text):
    """The lines load_data_from_text does not skip outright: not empty, not starting with '#'."""
    for ln in text.split("\n"):
        if ln and ln[0] != "#":
            yield ln


def restate(items, n, k=1):
    """What a reader gives for one chromosome of length n whose counted lines, in file order, are items: (lo, hi, vals),
    the positions lo..hi (lo >= 1) with the depth values vals (k of them).  Returns (rd: k x n int32, stats).

    The depth is the reference's sequential loop: later lines overwrite earlier ones, the first position >= n ends the
    file.  The counts are the reader's: with positions strictly increasing through the file (the device's proof) every
    position counts, those >= n as beyond; otherwise (fallback) the host loop's, which stop at the first one >= n."""
    rd = np.zeros((k, n), dtype=np.int32)
    lines = stored = beyond = 0
    for lo, hi, vals in items:
        top = min(hi, n - 1)
        if top >= lo:
            rd[:, lo - 1:top] = np.asarray(vals, dtype=np.int64).astype(np.int32)[:, None]
            lines += top - lo + 1
            stored += top - lo + 1
        if hi >= n:
            lines += 1
            beyond += 1
            break
    last, srt = -1, True
    for lo, hi, _ in items:
        if last >= 0 and lo <= last:
            srt = False
        last = hi
    if srt:
        lines = sum(hi - lo + 1 for lo, hi, _ in items)
        beyond = sum(max(0, hi - max(lo - 1, n - 1)) for lo, hi, _ in items)
        stored = lines - beyond
    return rd, dict(lines=lines, stored=stored, beyond=beyond, fallback=0 if srt else 1)


def items_of(rests, form="depth", k=1):
    """Counted items (lo, hi, vals) of a chromosome's line parts behind the name.  form: depth | samples | bedgraph."""
    out = []
    for rest in rests:
        if form == "bedgraph":
            f = bed_fields(rest)
            if f is None:
                continue
            a, b, d = max(f[0], 0), f[1], f[2]
            if b > a:
                out.append((a + 1, b, [d]))
            continue
        pos, vals = columns(rest, k) if form == "samples" else (lambda p, d: (p, [d]))(*per_base(rest))
        if pos >= 1:
            out.append((pos, pos, vals))
    return out


def load_text(text, n):
    """The single-chromosome reader ("pos d" lines): (rd, stats)."""
    rd, st = restate(items_of(data_lines(text)), n)
    return rd[0], st


def load_named(text, lens, form="depth", k=1, skip_bed_headers=None):
    """The genome readers: {name: (rd k x n, stats)} for every name of lens (a dict name -> n) that has data lines.
    Names must be contiguous in the text (the readers refuse the rest)."""
    bed = form == "bedgraph"
    rests = {}
    for ln in data_lines(text):
        name, rest = split_name(ln)
        if not name or (bed and name in ("track", "browser")) or name not in lens:
            continue
        rests.setdefault(name, []).append(rest)
    return {nm: restate(items_of(r, form, k), lens[nm], k) for nm, r in rests.items()}


# ---------------------------------------------------------------------------------------------------------------------
# the corpus: quirk lines, each template placed at an anchor position P of an ordinary sorted file
# ---------------------------------------------------------------------------------------------------------------------
# A template with {P} replaces the anchor's own line; one without is put in front of it.  A case whose quirk overflows pos
# towards +inf ends the reference's read, so each of those has a case of its own.  None of the lines lets an extraction
# after a successful pos reach the end of the line with nothing but blanks: there the reference's `int d` (declared without
# an initial value) would stay indeterminate.
CASES = {
    "d_bounds": ["{P}\t2147483647", "{P}\t2147483648", "{P}\t3000000000", "{P}\t100000000000000000000", "{P}\t-2147483648",
                 "{P}\t-2147483649", "{P} -9999999999999999999999999", "{P}\t000000000000000000000000017",
                 "{P}\t9223372036854775807", "{P}\t9223372036854775808", "{P}\t18446744073709551617"],
    "pos_2e31": ["2147483648\t5"],
    "pos_int_max": ["2147483647\t5"],
    "pos_2e64p1": ["18446744073709551617\t5"],
    "pos_1e22": ["10000000000000000000000\t5"],
    "pos_neg": ["-9223372036854775809\t5", "-2147483649 6", "-2147483648\t7", "-18446744073709551617 8"],
    "tokens": ["{P}abc 3", "{P}.7\t3", "{P}e3 7", "+{P} +3", "-0 4", "000{P}\t0007", "{P}\t+-3", "{P}\t- 3", "{P} \v\f 7",
               "{P}\t3 junk 9", "{P}\t-0", "{P}--4 5", "{P}+\t6", "\t {P}\t\t8\r", "{P}\t12abc"],
    "blanks": ["\r", "\t\t\t", " #{P} 3", "{P}\x00\t4", "{P}\t4\x005", "\x00{P}\t9", " \v{P}\f\f13"],
}
FINAL_NO_NEWLINE = {"tokens", "blanks"}   # their last line (an ordinary one below n) has no '\n'


def background(p):
    """The ordinary line of position p: varied blanks, '\\r' on some, depth from p."""
    d = (p * 7919) % 97
    sep = ("\t", " ", "\t ", "  ")[p % 4]
    lead = " " if p % 23 == 0 else ""
    return f"{lead}{p}{sep}{d}" + ("\r" if p % 11 == 0 else "")


def place(templates, anchors):
    """[(anchor P, the lines that stand at P)]: the template's line for P (in front of P's own line without {P})."""
    out = {}
    for t, P in zip(templates, anchors):
        out[P] = [t.replace("{P}", str(P))] if "{P}" in t else [t, background(P)]
    return out


def case_text(case, n=3001):
    """A golden case's whole text: positions 1 .. n + 2 (the last ones beyond n), anchors spread over the middle.  With a
    final line without '\\n', the file ends at n - 4 instead."""
    tmpl = CASES[case]
    last = n - 4 if case in FINAL_NO_NEWLINE else n + 2
    anchors = [n // 3 + 37 * i for i in range(len(tmpl))]
    at = place(tmpl, anchors)
    lines = ["# text_rules corpus: " + case, ""]
    for p in range(1, last + 1):
        lines += at.get(p, [background(p)])
    return "\n".join(lines) + ("" if case in FINAL_NO_NEWLINE else "\n")


def case_bytes(case, n=3001):
    return case_text(case, n).encode("latin-1")


def text_hash(b):
    return hashlib.sha256(b).hexdigest()


# ---------------------------------------------------------------------------------------------------------------------
# larger files for the readers: quirk lines on chunk boundaries of an ordinary sorted file
# ---------------------------------------------------------------------------------------------------------------------

def embed(rows, templates, prefix="", offset=0, boundary=4097, first=1000, gap=50):
    """rows: the ordinary lines [(text, {"P": .., "S": .., "E": ..})] in file order, the text behind `prefix`.  Each
    template (its {P} / {S} / {E} filled from the row it lands on) replaces that row's line, or goes in front of it when it
    names none of them; the rows are picked so that the template's line starts 0-2 bytes before a multiple of `boundary`
    (a chunk of that many bytes then ends inside it or right at its start).  offset: bytes in front of rows[0]."""
    out = [prefix + t for t, _ in rows]
    lens = np.fromiter((len(s) + 1 for s in out), dtype=np.int64, count=len(out))
    starts = offset + np.concatenate([[0], np.cumsum(lens)[:-1]])
    placed, delta, i0 = {}, 0, first
    for t in templates:
        r = (-(starts[i0:] + delta)) % boundary
        i = i0 + int(np.argmax(r <= 2))
        f = rows[i][1]
        line = t
        for k, v in f.items():
            line = line.replace("{" + k + "}", str(v))
        new = [prefix + line] if line != t or "{" in t else [prefix + line, out[i]]
        placed[i] = new
        delta += sum(len(s) + 1 for s in new) - int(lens[i])
        i0 = i + gap
    res = []
    for i, s in enumerate(out):
        res += placed.get(i, [s])
    return res


def per_base_rows(n, extra=2, k=None):
    """Ordinary "pos d" rows for positions 1 .. n + extra (k depth columns for a cohort file)."""
    rows = []
    for p in range(1, n + extra + 1):
        d = (p * 7919) % 97
        sep = ("\t", " ", "\t ")[p % 3]
        body = f"{p}{sep}{d}" if k is None else f"{p}\t" + "\t".join(str((d + 13 * j) % 89) for j in range(k))
        rows.append((body + ("\r" if p % 11 == 0 else ""), {"P": p}))
    return rows


def bed_rows(n, seed, zero_runs=True, extra=3):
    """Ordinary bedGraph rows "start end d" over [0, n + extra): runs of 1-6 bases; zero runs left out with zero_runs=False
    (genomecov -bg), kept with True (-bga, mosdepth)."""
    rng = np.random.default_rng(seed)
    rows, s = [], 0
    while s < n + extra:
        e = min(s + int(rng.integers(1, 7)), n + extra)
        d = 0 if rng.random() < 0.15 else int(rng.integers(1, 90))
        if d or zero_runs:
            rows.append((f"{s}\t{e}\t{d}", {"S": s, "E": e}))
        s = e
    return rows
