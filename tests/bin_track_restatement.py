"""numpy restatement of the per-bin track (include/rsi_hot.h), written from the definition alone: no break table,
no cumulated shifts.  The removed regions become a boolean mask, the kept reference positions are listed, bin b is the b-th
group of m of them, split where consecutive positions differ by more than 1.  Values are formatted with Python integers.

For a chromosome too long for a mask, `pieces_by_intervals` walks the regions' complement intervals instead; the two forms are
checked against each other on small inputs (tests/test_bin_track_restatement.py)."""
import numpy as np


def _pairs(pairs):
    return [(int(s), int(e)) for s, e in np.asarray(pairs, dtype=np.int64).reshape(-1, 2)]


def pieces_by_mask(nb, m, n, pairs):
    """[(bin, start, end)], 0-based half-open, from the list of kept reference positions."""
    removed = np.zeros(n, dtype=bool)
    for s, e in _pairs(pairs):
        removed[s:e + 1] = True
    ref_of = np.flatnonzero(~removed)
    assert nb * m <= ref_of.size
    out = []
    for b in range(nb):
        pos = ref_of[b * m:(b + 1) * m]
        cuts = np.flatnonzero(np.diff(pos) > 1) + 1
        for part in np.split(pos, cuts):
            out.append((b, int(part[0]), int(part[-1]) + 1))
    return out


def pieces_by_intervals(nb, m, n, pairs):
    """The same list from the kept intervals between the regions: every bin takes its m bases from them in order."""
    kept, at = [], 0
    for s, e in _pairs(pairs):
        if s > at:
            kept.append((at, s))
        at = e + 1
    if at < n:
        kept.append((at, n))
    out, it = [], iter(kept)
    cur = next(it, None)
    for b in range(nb):
        need = m
        while need > 0:
            assert cur is not None, "more bins than kept bases"
            s, e = cur
            take = min(need, e - s)
            out.append((b, s, s + take))
            need -= take
            cur = (s + take, e) if s + take < e else next(it, None)
    return out


def value_text(v, which, median2=0):
    """which 0: %d.  which 1: round_half_up(1000 v / (median2 / 2)) as thousandths with a point, in integers."""
    v = int(v)
    if which == 0:
        return b"%d" % v
    m2 = int(median2)
    assert m2 > 0 and v >= 0
    q = (4000 * v + m2) // (2 * m2)
    return b"%d.%03d" % (q // 1000, q % 1000)


def text(values, m, n, pairs, median2, which, name, by="mask"):
    name = name if isinstance(name, bytes) else name.encode()
    values = np.asarray(values).astype(np.int64)
    pc = (pieces_by_mask if by == "mask" else pieces_by_intervals)(values.size, m, n, pairs)
    return b"".join(b"%s\t%d\t%d\t%s\n" % (name, s, e, value_text(values[b], which, median2)) for b, s, e in pc)


def check_valid(track, n, pairs):
    """What a sorted, non-overlapping bedGraph asks of one chromosome's lines, and the track's own promise: four fields, one name,
    0 <= start < end <= n, every start at or behind the end before it, no removed base under any line.  Returns the lines as
    [(start, end, value bytes)]."""
    rows, last_end, name = [], 0, None
    regions = _pairs(pairs)
    starts = np.array([s for s, _ in regions], dtype=np.int64)
    ends = np.array([e for _, e in regions], dtype=np.int64)
    for ln in track.splitlines(keepends=True):
        assert ln.endswith(b"\n"), ln
        f = ln[:-1].split(b"\t")
        assert len(f) == 4, ln
        name = name if name is not None else f[0]
        assert f[0] == name, ln
        s, e = int(f[1]), int(f[2])
        assert f[1] == b"%d" % s and f[2] == b"%d" % e, ln
        assert 0 <= s < e <= n and s >= last_end, ln
        k = int(np.searchsorted(ends, s, side="left"))      # the first region that ends at or behind s
        assert k == len(regions) or starts[k] >= e, (ln, regions[k])
        last_end = e
        rows.append((s, e, f[3]))
    return rows


def expand_median(track, n, pairs):
    """A `median` track back into one value per covered base, in order (uncovered bases dropped)."""
    rows = check_valid(track, n, pairs)
    if not rows:
        return np.zeros(0, dtype=np.int64)
    return np.concatenate([np.full(e - s, int(v), dtype=np.int64) for s, e, v in rows])
