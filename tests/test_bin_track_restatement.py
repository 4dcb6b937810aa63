"""CPU: the restatement of the per-bin track (tests/bin_track_restatement.py) against cases written out by hand, one for every
rule of the definition; its two forms against each other; the rounding table of `ratio`; and the inverse -- a
`median` track expanded per base gives every bin's value m times."""
import math
from fractions import Fraction

import numpy as np
import pytest

import bin_track_restatement as bt

INT32_MAX = 2**31 - 1

# (values, m, n, pairs, expected lines as (start, end, value)) -- reference positions worked out by hand
HAND = {
    # 10 bases, nothing removed, m = 3: three bins, the tenth base is the tail
    "plain_tail1": ([5, 6, 7], 3, 10, [], [(0, 3, 5), (3, 6, 6), (6, 9, 7)]),
    # region (3, 4) removes two bases: kept 0 1 2 | 5 6 7 8 9.  m = 3: the break lies exactly at the edge of bins 0 and 1 -> no cut
    "break_at_edge": ([1, 2], 3, 10, [(3, 4)], [(0, 3, 1), (5, 8, 2)]),
    # region (2, 3): kept 0 1 | 4 5 6 7 8 9.  The break is one base inside bin 0 from its end
    "break_one_before_edge": ([1, 2], 3, 10, [(2, 3)], [(0, 2, 1), (4, 5, 1), (5, 8, 2)]),
    # region (4, 5): kept 0 1 2 3 | 6 7 8 9.  The break is one base inside bin 1 from its start
    "break_one_after_edge": ([1, 2], 3, 10, [(4, 5)], [(0, 3, 1), (3, 4, 2), (6, 8, 2)]),
    # every second base removed: kept 0 2 4 6 8 10.  m = 3: each bin in m pieces; m = 1 below: no bin is cut
    "m_pieces": ([9, 8], 3, 11, [(1, 1), (3, 3), (5, 5), (7, 7), (9, 9)],
                 [(0, 1, 9), (2, 3, 9), (4, 5, 9), (6, 7, 8), (8, 9, 8), (10, 11, 8)]),
    "m1_every_bin_borders_a_break": ([4, 5, 6], 1, 5, [(1, 1), (3, 3)], [(0, 1, 4), (2, 3, 5), (4, 5, 6)]),
    # a region from 0: the first bin starts behind it, uncut
    "region_at_0": ([3, 4], 2, 9, [(0, 3)], [(4, 6, 3), (6, 8, 4)]),
    # a region ending at n - 1: five kept bases, two bins of two, a tail of one in front of the region
    "region_to_end": ([3, 4], 2, 9, [(5, 8)], [(0, 2, 3), (2, 4, 4)]),
    # both, and nothing else
    "regions_at_both_ends": ([7], 4, 12, [(0, 2), (8, 11)], [(3, 7, 7)]),
    # a tail of m - 1 bases behind the last bin gets no line, even across a region
    "tail_m_minus_1": ([1], 3, 8, [(4, 5)], [(0, 3, 1)]),
    "no_bins": ([], 3, 2, [], []),
}


def _text(lines, name=b"c"):
    return b"".join(b"%s\t%d\t%d\t%d\n" % (name, s, e, v) for s, e, v in lines)


@pytest.mark.parametrize("case", sorted(HAND))
def test_hand_written_cases(case):
    values, m, n, pairs, lines = HAND[case]
    for by in ("mask", "intervals"):
        assert bt.text(values, m, n, pairs, 0, 0, "c", by=by) == _text(lines), by
    bt.check_valid(_text(lines), n, pairs)


def random_case(rng, nb_max=300, nreg_max=40):
    """values, m, n, pairs: regions at random, some a single kept base apart, sometimes at 0 and at n - 1."""
    m = int(rng.choice([1, 2, 3, 5, 7, 101]))
    nreg = int(rng.integers(0, nreg_max + 1))
    pairs, at = [], 0 if rng.random() < 0.3 else int(rng.integers(1, 2 * m + 2))
    for _ in range(nreg):
        w = int(rng.integers(1, 30))
        pairs.append((at, at + w - 1))
        at += w + (1 if rng.random() < 0.3 else int(rng.integers(1, 3 * m + 2)))
    n = at - 1 if pairs and rng.random() < 0.3 else at + int(rng.integers(0, nb_max * m))
    n = max(n, 1)
    kept = n - sum(e - s + 1 for s, e in pairs)
    nb = min(kept // m, nb_max)
    values = rng.integers(0, 200, size=nb)
    return values, m, n, pairs


def test_the_two_forms_agree_on_random_inputs():
    rng = np.random.default_rng(0xB17)
    for _ in range(60):
        values, m, n, pairs = random_case(rng)
        nb = len(values)
        assert bt.pieces_by_mask(nb, m, n, pairs) == bt.pieces_by_intervals(nb, m, n, pairs)


# v, M2, text: q = round_half_up(1000 v / (M2 / 2))
RATIO_TABLE = [
    (0, 7, b"0.000"),
    (1, 32, b"0.063"),            # 62.5 thousandths: the tie goes up
    (1, 2000, b"0.001"), (1, 4001, b"0.000"), (1, 4000, b"0.001"),   # 0.5 up, just below 0.5 down
    (30, 60, b"1.000"), (45, 60, b"1.500"), (15, 60, b"0.500"),
    (999, 2000, b"0.999"), (1000, 2000, b"1.000"),      # q below and at 1000
    (25, 4, b"12.500"),
    (2, 3, b"1.333"), (1, 3, b"0.667"),
    (INT32_MAX, 1, b"4294967294.000"),
    (INT32_MAX, 2 * INT32_MAX, b"1.000"),
]


@pytest.mark.parametrize("v,m2,exp", RATIO_TABLE)
def test_ratio_rounding_table(v, m2, exp):
    assert bt.value_text(v, 1, m2) == exp
    # against exact rational arithmetic: floor(1000 v / (m2 / 2) + 1/2)
    q = math.floor(Fraction(2000 * v, m2) + Fraction(1, 2))
    assert exp == b"%d.%03d" % (q // 1000, q % 1000)
    assert len(exp) <= 18


def test_median_values_are_plain_integers():
    for v, exp in [(0, b"0"), (9, b"9"), (10, b"10"), (10**9, b"1000000000"), (INT32_MAX, b"2147483647")]:
        assert bt.value_text(v, 0) == exp


def test_median_track_expands_back_to_the_bins():
    rng = np.random.default_rng(0xB18)
    for _ in range(30):
        values, m, n, pairs = random_case(rng)
        t = bt.text(values, m, n, pairs, 0, 0, "chr1")
        per_base = bt.expand_median(t, n, pairs)
        assert per_base.size == len(values) * m
        assert np.array_equal(per_base, np.repeat(np.asarray(values, dtype=np.int64), m))


def test_validity_check_sees_what_it_should():
    ok = b"c\t0\t3\t1\nc\t5\t8\t2\n"
    bt.check_valid(ok, 10, [(3, 4)])
    for bad, pairs in [(b"c\t0\t4\t1\n", [(3, 4)]),                       # covers a removed base
                       (b"c\t5\t8\t2\nc\t0\t3\t1\n", []),                  # not sorted
                       (b"c\t0\t3\t1\nc\t2\t5\t1\n", []),                  # overlapping
                       (b"c\t0\t11\t1\n", []),                             # beyond n
                       (b"c\t3\t3\t1\n", []),                              # empty
                       (b"c\t0\t3\t1\nd\t3\t5\t1\n", [])]:                 # two names
        with pytest.raises(AssertionError):
            bt.check_valid(bad, 10, pairs)
