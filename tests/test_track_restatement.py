"""CPU: the numpy restatement the depth-track tests compare against (tests/track_restatement.py), on hand-written cases."""
import numpy as np

import track_restatement as tr


def test_hand_written_runs():
    assert tr.text([5, 5, 0, 0, 0, 7], "chrT") == b"chrT\t0\t2\t5\nchrT\t2\t5\t0\nchrT\t5\t6\t7\n"


def test_single_values_and_single_run():
    assert tr.text([3], "x") == b"x\t0\t1\t3\n"
    assert tr.text([0, 0, 0, 0], "chr1") == b"chr1\t0\t4\t0\n"
    assert tr.text([1, 2], "c") == b"c\t0\t1\t1\nc\t1\t2\t2\n"
    assert tr.text([], "c") == b""


def test_negative_values_and_the_int32_limits():
    v = np.array([-1, -1, 2147483647, -2147483648, 0], dtype=np.int32)
    assert tr.text(v, "n") == b"n\t0\t2\t-1\nn\t2\t3\t2147483647\nn\t3\t4\t-2147483648\nn\t4\t5\t0\n"


def test_coordinate_offset():
    assert tr.text([4, 4, 9], "chrT", pos0=9999999990) == b"chrT\t9999999990\t9999999992\t4\nchrT\t9999999992\t9999999993\t9\n"


def test_zero_runs_are_written_and_runs_are_maximal():
    v = [0, 0, 1, 1, 1, 0, 2, 2]
    ls = tr.lines(v, "z")
    assert len(ls) == 4 and ls[0] == b"z\t0\t2\t0\n" and ls[2] == b"z\t5\t6\t0\n"
    # neighbouring lines never carry the same value
    vals = [int(l.split(b"\t")[3]) for l in ls]
    assert all(a != b for a, b in zip(vals, vals[1:]))


def test_expand_inverts_text():
    rng = np.random.default_rng(5)
    v = np.repeat(rng.integers(-3, 4, 200), rng.integers(1, 9, 200))
    assert np.array_equal(tr.expand(tr.text(v, "chrE"), "chrE", v.size), v)
