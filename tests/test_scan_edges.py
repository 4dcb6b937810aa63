"""GPU: one scan pass alone (rsi_hot_debug_scan: k_scan_detect, k_rsi_scan, k_level_stop, k_resolve_runs) on every case of
tests/scan_cases.py, against the reference's status (golden/scan_edges.npz) bit for bit, with the pass's three counters, with
and without the detection pass and with a tile's lengths in one share and in as many as the launcher allows."""
import json
import os
import time

import numpy as np
import pytest

import scan_cases as sc
from scan_restatement import rsistatus_numpy

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scan_edges.npz")


@pytest.fixture(scope="module")
def hot():
    from rsicnv_amd import api
    h = api.RsiHot(0)
    yield h
    h.close()


@pytest.fixture(scope="module")
def expected(oracle_cls):
    """name -> (status, escapes, has_hit): the golden status; for the escape cases the bounded restatement's; zeros for exactness (a),
    whose thresholds no window reaches.  Computed once and shared."""
    z = np.load(GOLDEN)
    names, off, st = json.loads(str(z["names"])), z["off"], z["status"]
    gold = {n: st[off[k]:off[k + 1]] for k, n in enumerate(names)}
    out = {}
    for c in sc.all_cases():
        esc = 0
        if c.ref:
            exp = gold[c.name]
        elif c.group == "escapes":
            exp, esc = rsistatus_numpy(c.T, c.medint, c.RDmedian, c.tmedian, c.tlamda, c.Lmax, oracle_cls().exact_median, bounded=True)
        else:
            exp = np.zeros(c.T.size, dtype=np.int32)
        has_hit = bool((exp != 0).any())
        if not has_hit and c.T.size <= 4000:      # hits that fail the median test or trim to nothing still make the detection pass list a tile
            hits = sc.score_hits(c.T, c.tmedian, c.tlamda, c.Lmax)
            has_hit = bool(hits[0] or hits[1])
        out[c.name] = (exp, esc, has_hit)
    return out


def alternating():
    """Every case, short and long Lmax in turn: a context that has staged a long scan runs a short one next, and back."""
    by_len = sorted(sc.all_cases(), key=lambda c: (c.Lmax, c.name))
    order = []
    while by_len:
        order.append(by_len.pop(0))
        if by_len:
            order.append(by_len.pop())
    return order


def run_every_case(hot, expected, detect_on):
    spent = {}
    for c in alternating():
        exp, esc, has_hit = expected[c.name]
        t0 = time.perf_counter()
        got, info = hot.debug_scan(c.T, c.medint, c.RDmedian, c.tmedian, c.tlamda, c.Lmax)
        spent[c.group] = spent.get(c.group, 0.0) + time.perf_counter() - t0
        diff = np.nonzero(got != exp)[0]
        where = f"{c.name}: {diff.size} bins differ, first at {diff[:5]}, info {list(info)}"
        if c.group == "exact_b":
            assert diff.size == 0 or info[2] > 0, where      # an answer that is not the reference's is flagged
        else:
            assert diff.size == 0, where
            assert info[2] == c.expect["inexact"], where
        assert info[1] == esc, where
        detected = detect_on and sc.detect_runs(c.Lmax)
        # not for exactness (a): its bins are there for the counter alone.  Next to values of 2^19 the float margin of the detection pass
        # (2^-22 of the largest prefix) is wider than a bin of 2^-10 is from the DEL threshold, and scan_thresholds bisects over
        # sums >= 0 (transformed bins are never negative), so a window of negative sum is no one's hit and still listed
        if c.group != "exact_a":
            assert (info[0] > 0) == (detected and has_hit), where
    print("seconds per group:", {g: round(s, 3) for g, s in sorted(spent.items())})


def test_every_case(hot, expected):
    run_every_case(hot, expected, True)
    # the flag of exactness (b) is the sufficient test, not an accident of one case
    for name in sc.case_names("exact_b"):
        c = sc.get_case(name)
        assert hot.debug_scan(c.T, c.medint, c.RDmedian, c.tmedian, c.tlamda, c.Lmax)[1][2] > 0, name


def test_every_case_without_the_detection_pass(hot, expected, monkeypatch):
    monkeypatch.setenv("RSI_HOT_SCAN_DETECT", "0")
    run_every_case(hot, expected, False)


@pytest.mark.parametrize("parts", [1, 8], ids=["one_share", "most_shares"])
def test_every_case_with_the_lengths_split(hot, expected, monkeypatch, parts):
    """RSI_HOT_SCAN_PARTS: a listed tile's lengths in one workgroup, and in as many as there can be (8; a scan of fewer than 8 groups of
    lengths keeps its own number)."""
    assert parts <= max(sc.max_parts(c.Lmax) for c in sc.all_cases()) == 8
    monkeypatch.setenv("RSI_HOT_SCAN_PARTS", str(parts))
    run_every_case(hot, expected, True)
