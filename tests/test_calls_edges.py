"""GPU: the three list stages behind the scan, each alone with the production device tester attached (rsi_hot_debug_block_stage / _merge /
_calls: test_block_segments, merge_neighbours, call_from_segments of host_calls.cpp), on every case of tests/calls_cases.py, in both
storages where the values fit in bytes and, for the block stage, through the dense and the sparse status form:

  the lists against the reference's own answers (golden/calls_edges.npz) and against the restatement of the reference's serial loops
  (tests/calls_cases.py, which tests/test_calls_cases.py pins to the compiled reference): integers and grid-valued columns bit for bit,
  p1, cnvsd and score at the project's rtol = 1e-6;
  the tester-on result against the tester-off result of the same hook with == on every field: a shortcut changes no bit;
  the road of every first-round block test and the counters (batch hits, tests judged from a result launched ahead, tests launched alone,
  host fallbacks, waits, range-sum calls, means answered from the batch of sums, means taken again) against the restatement's prediction.

detectcnv's own body (bins -> bases, the stage order, the score, the N-region filter) has no reference function of its own: the `raw` calls
are compared with the restatement, whose stages the golden file pins one by one, and the whole-run goldens pin the order as a whole.

Neither the reference nor libref.so is read here."""
import time

import numpy as np
import pytest

import calls_cases as K

pytestmark = pytest.mark.gpu
COUNTERS = ("spec_hits", "single_tests", "host_fallbacks", "block_batch_hits", "waits", "sum_launches", "sum_reused", "sum_redone")


@pytest.fixture(scope="module")
def hot():
    from rsicnv_amd import api
    h = api.RsiHot(0)
    yield h
    h.close()


@pytest.fixture(scope="module")
def golden():
    return K.load_golden()


def records(L):
    from rsicnv_amd import api
    out = np.zeros(len(L), dtype=api.CALL_RECORD)
    for i, c in enumerate(L):
        for k in K.FIELDS:
            out[i][k] = c[k]
    return out


def check(got, want, tag, skip=()):
    assert len(got) == len(want), (tag, len(got), len(want))
    for i, w in enumerate(want):
        for k in K.EXACT:
            if k not in skip:
                assert got[i][k].item() == w[k], (tag, i, k, got[i][k].item(), w[k])
        for k in K.CLOSE:
            if k not in skip:
                assert np.isclose(got[i][k].item(), w[k], rtol=1e-6, atol=1e-300), (tag, i, k, got[i][k].item(), w[k])


def same_bits(a, b):
    return len(a) == len(b) and all(np.array_equal(a[k], b[k]) for k in a.dtype.names)


def counters(info):
    return {k: info[k] for k in COUNTERS}


def run_block(hot, c, golden, seen):
    want, rec = K.restated(c)
    got = {}
    for sparse in (False, True):
        segs, road, info = hot.debug_block_stage(c.depth, c.status, records(c.cands), c.span_all, c.RDmedian, tester=True, sparse=sparse, **c.P)
        tag = (c.name, c.claim, "sparse" if sparse else "dense")
        check(segs, golden[c.name]["out"], tag)
        check(segs, want, tag)
        assert road.tolist() == rec["road"], (tag, road.tolist(), rec["road"])
        assert counters(info) == {k: rec["info"][k] for k in COUNTERS}, (tag, info, rec["info"])
        got[sparse] = segs
        off, road_off, info_off = hot.debug_block_stage(c.depth, c.status, records(c.cands), c.span_all, c.RDmedian, tester=False, sparse=sparse, **c.P)
        assert same_bits(segs, off), tag
        assert set(road_off.tolist()) == {1} and not any(counters(info_off).values()), (tag, info_off)
    assert same_bits(got[False], got[True]), c.name
    seen["batch hits"] += rec["road"].count(0)
    seen["batch refusals by reach"] += rec["road"].count(2)


def run_merge(hot, c, golden, seen):
    want, Kc, rec = K.restated(c)
    base = None
    for storage in K.storages(c):
        out, info = hot.debug_merge(c.depth, storage, records(c.cands), c.RDmedian, tester=True, **c.P)
        tag = (c.name, c.claim, storage)
        check(out, golden[c.name]["out"], tag)
        check(out, want, tag)
        assert counters(info) == {k: Kc[k] for k in COUNTERS}, (tag, info, Kc)
        off, info_off = hot.debug_merge(c.depth, storage, records(c.cands), c.RDmedian, tester=False, **c.P)
        assert same_bits(out, off), tag
        assert not any(counters(info_off).values()), (tag, info_off)
        assert base is None or same_bits(out, base), tag          # bytes against int32
        base = out
    tally(seen, Kc, rec)


def run_calls(hot, c, golden, seen):
    blocks, raw, kept, Kc, rec = K.restated(c)
    g = golden[c.name]
    base = None
    for storage in K.storages(c):
        got = hot.debug_calls(c.depth, storage, records(c.cands), c.noncode, c.RDmedian, c.RDsd, tester=True, **c.P)
        tag = (c.name, c.claim, storage)
        check(got[0], blocks, tag)
        check(got[1], raw, tag)
        check(got[2], kept, tag)
        check(got[2], g["kept"], tag)
        # the reference's own tests in order, for the calls that survive the N-region filter (coordinates and score are detectcnv's lines)
        alive = [t for t, x in zip(g["tested"], rec["tested"]) if x["status"] != -9]
        check(got[1], alive, tag, skip=("start", "end", "score"))
        if len(c.noncode):
            back = dict(zip(*(a.tolist() for a in g["expand"])))
            assert [(int(x["start"]), int(x["end"])) for x in got[1]] == [(back[x["start"]], back[x["end"]]) for x in rec["tested"] if x["status"] != -9], tag
        assert counters(got[3]) == {k: Kc[k] for k in COUNTERS}, (tag, got[3], Kc)
        off = hot.debug_calls(c.depth, storage, records(c.cands), c.noncode, c.RDmedian, c.RDsd, tester=False, **c.P)
        assert all(same_bits(a, b) for a, b in zip(got[:3], off[:3])), tag
        assert not any(counters(off[3]).values()), (tag, off[3])
        assert base is None or all(same_bits(a, b) for a, b in zip(got[:3], base)), tag
        base = got[:3]
    tally(seen, Kc, rec)


def tally(seen, Kc, rec):
    seen["speculative hits"] += Kc["spec_hits"]
    seen["speculative refusals"] += sum(1 for s in rec["spec"] if s[2] != "hit")
    seen["speculative refusals that matter"] += sum(1 for s in rec["spec"] if s[2] != "hit" and not s[3])
    seen["sum slots reused"] += Kc["sum_reused"]
    seen["sum slots redone"] += sum(1 for s in rec["sums"] if s[2] is not None and not all(s[1]))


def alternating(cases):
    by_size = sorted(cases, key=lambda c: (len(c.cands), c.depth.size, c.name))
    order = []
    while by_size:
        order.append(by_size.pop(0))
        if by_size:
            order.append(by_size.pop())
    return order


def test_every_case_twice_on_one_context(hot, golden):
    """All cases of all three stages on ONE context, short and long lists in turn, everything twice; then the vacuity guard: the file as
    a whole makes every shortcut both taken and refused (the counts are the restatement's, which every run above was held to)."""
    run = dict(block=run_block, merge=run_merge, calls=run_calls)
    seen = {}
    t0 = time.perf_counter()
    for rnd in range(2):
        seen = {k: 0 for k in ("batch hits", "batch refusals by reach", "speculative hits", "speculative refusals", "speculative refusals that matter",
                               "sum slots reused", "sum slots redone")}
        for c in alternating(K.all_cases()):
            run[c.stage](hot, c, golden, seen)
    print(f"{len(K.all_cases())} cases twice: {time.perf_counter() - t0:.3f} s with the restatement; {seen}")
    assert all(v >= 1 for v in seen.values()), seen


def test_bad_arguments_leave_the_context_usable(hot, golden):
    from rsicnv_amd import api

    def refused(f, *a, **kw):
        with pytest.raises(api.RsiError) as err:
            f(*a, **kw)
        assert err.value.code == -2

    b = K.get_case("block_24_del")
    segs = records(b.cands)
    bad = segs.copy()
    bad[3]["end"] = b.depth.size
    refused(hot.debug_block_stage, b.depth, b.status, bad, b.span_all, b.RDmedian, **b.P)                    # a segment behind the bins
    bad = segs.copy()
    bad[0]["type"] = 2
    refused(hot.debug_block_stage, b.depth, b.status, bad, b.span_all, b.RDmedian, **b.P)                    # a type the reference exits on
    refused(hot.debug_block_stage, b.depth, np.zeros_like(b.status), segs, b.span_all, b.RDmedian, sparse=True, **b.P)      # no run for the sparse form
    refused(hot.debug_block_stage, b.depth, b.status, segs, b.span_all, b.RDmedian, **dict(b.P, chklen=0.0))
    m = K.get_case("merge_overlap_union_del")
    L = records(m.cands)
    bad = L.copy()
    bad[1]["start"], bad[1]["end"] = 9000, 8000
    refused(hot.debug_merge, m.depth, 1, bad, m.RDmedian, **m.P)                                             # end < start
    refused(hot.debug_merge, m.depth, 2, L, m.RDmedian, **m.P)                                               # a storage that does not exist
    wide = m.depth.copy()
    wide[7] = 256
    refused(hot.debug_merge, wide, 1, L, m.RDmedian, **m.P)                                                  # beyond a byte under storage 1
    c = K.get_case("calls_regions_del")
    S = records(c.cands)
    refused(hot.debug_calls, c.depth, 1, S, [(5000, 5999), (0, 999)], c.RDmedian, c.RDsd, **c.P)             # regions out of order
    refused(hot.debug_calls, c.depth, 1, S, [(700, 700)], c.RDmedian, c.RDsd, **c.P)                         # a region of one base: the reference exits
    bad = S.copy()
    bad[0]["start"] = bad[0]["end"] = c.depth.size // c.P["m"] + 1
    refused(hot.debug_calls, c.depth, 1, bad, c.noncode, c.RDmedian, c.RDsd, **c.P)                          # a segment that starts behind the array
    seen = {k: 0 for k in ("batch hits", "batch refusals by reach", "speculative hits", "speculative refusals", "speculative refusals that matter",
                           "sum slots reused", "sum slots redone")}
    run_block(hot, b, golden, seen)
    run_merge(hot, m, golden, seen)
    run_calls(hot, c, golden, seen)
