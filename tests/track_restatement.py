"""numpy restatement of the depth-track writer (include/rsi_hot.h): an integer array as the text of
`bedtools genomecov -bga` -- one line NAME<TAB>start<TAB>end<TAB>value per maximal run of equal values, start 0-based, end
exclusive, zeros included, coordinates offset by pos0."""
import numpy as np


def run_bounds(values):
    """(starts, ends) of the maximal runs of equal values."""
    v = np.asarray(values)
    if v.size == 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    starts = np.concatenate([[0], np.flatnonzero(np.diff(v)) + 1]).astype(np.int64)
    ends = np.concatenate([starts[1:], [v.size]]).astype(np.int64)
    return starts, ends


def lines(values, name, pos0=0):
    name = name if isinstance(name, bytes) else name.encode()
    v = np.asarray(values).astype(np.int64)
    starts, ends = run_bounds(v)
    return [b"%s\t%d\t%d\t%d\n" % (name, int(pos0) + int(s), int(pos0) + int(e), int(v[s])) for s, e in zip(starts, ends)]


def text(values, name, pos0=0):
    return b"".join(lines(values, name, pos0))


def expand(track, name, n):
    """A track's lines of `name` back into the array of n values they stand for (every base must be covered once)."""
    name = name if isinstance(name, bytes) else name.encode()
    out = np.zeros(n, dtype=np.int64)
    covered = 0
    for ln in track.splitlines():
        f = ln.split(b"\t")
        if f[0] != name:
            continue
        s, e = int(f[1]), int(f[2])
        assert s == covered and e > s, ln
        out[s:e] = int(f[3])
        covered = e
    assert covered == n
    return out
