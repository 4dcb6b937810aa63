"""CPU: the cases of tests/calls_cases.py are what they claim to be, and the restatement of the three list stages they are judged by equals
the compiled reference's answers (golden/calls_edges.npz): integers and the grid-valued columns bit for bit, p1, cnvsd and score at the
project's rtol = 1e-6.  The restatement also proves what the device shortcuts of host_calls.cpp rest on: a first-round block test the batch
may answer has the same judgement against the stale list as against the list as it stands, and so has every test launched ahead whose plan
still holds.  Nothing here touches the library's device code.

detectcnv's body is not restated in the reference driver: its bins -> bases loop, the stage order, the score and the N-region filter
exist in calls_cases.calls_stage only, each stage pinned to the reference function it calls, and stay pinned as a whole by the whole-run
goldens (tests/golden/cfg*.npz)."""
import math
import os
import re

import numpy as np
import pytest

import calls_cases as K
import cand_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEL, DUP = K.DEL, K.DUP


@pytest.fixture(scope="module")
def golden():
    return K.load_golden()


def both(name):
    return [K.get_case(f"{name}_{tag}") for _, tag in K.KINDS]


def agree(want, got, tag, skip=()):
    """want: the reference's list; got: the restatement's."""
    assert len(want) == len(got), (tag, len(want), len(got))
    for i, (w, g) in enumerate(zip(want, got)):
        for k in K.EXACT:
            if k not in skip:
                assert w[k] == g[k], (tag, i, k, w[k], g[k])
        for k in K.CLOSE:
            if k not in skip:
                assert np.isclose(w[k], g[k], rtol=1e-6, atol=1e-300), (tag, i, k, w[k], g[k])


def test_the_constants_are_the_librarys():
    hc = open(os.path.join(ROOT, "rsicnv_amd", "csrc", "host_calls.cpp")).read()
    m = re.search(r"kBlockBatchMin\s*=\s*(\d+)\s*;", hc)
    assert m and int(m.group(1)) == K.BLOCK_BATCH_MIN
    m = re.search(r"kChainMax\s*=\s*(\d+)\s*;", hc)
    assert m and int(m.group(1)) == cc.CHAIN_MAX


def test_every_case_in_both_kinds_and_all_in_the_golden_file(golden):
    names = {c.name for c in K.all_cases()}
    assert set(golden) == names                       # none excluded
    stems = {}
    for n in names:
        stem, tag = n.rsplit("_", 1)
        stems.setdefault(stem, set()).add(tag)
    for stem, tags in stems.items():
        if "rescue" not in stem:                      # (the rescue's two values differ by kind)
            assert tags == {"del", "dup"}, stem
    for c in K.all_cases():
        assert c.depth.size <= (4000 if c.stage == "block" else 300_000) and c.depth.min() >= 0, c.name
        assert c.P["m"] == 101 or c.P["m"] == 1 or "minlen" in c.name, c.name      # (m = 1: bins are bases, edges can sit anywhere)
    assert {c.stage for c in K.all_cases()} == {"block", "merge", "calls"}


def test_the_references_loops_stay_inside_its_arrays():
    """What tools/make_golden_calls.py asserts again before it runs the reference: every neighbourhood test of every stage has a
    neighbourhood longer than its candidate, takes no value past `capacity` and reads the depth inside it; every edge refinement stays
    inside the reference's vector; every range mean_tp is asked for lies inside the array, and so does every region's expansion."""
    tests = 0
    for c in K.all_cases():
        for tester in (True, False):
            r = K.restated(c, tester)
            for t in r[-1]["tests"]:
                assert K.inside(t, c.depth.size), (c.name, t["plan"])
                assert t["plan"]["top"] >= -1 and t["plan"]["capacity"] >= 1, c.name
                tests += 1
        if c.stage == "calls":
            assert all(K.sc.stays_inside(x) for x in K.restated(c)[-1]["sharpen"]) != bool(c.expect.get("crossed_refine")), c.name
            assert all(e > s for s, e in c.noncode), c.name          # expand_coordinate exits on end <= start
        for x in c.cands:
            if c.stage != "calls":
                assert 0 <= x["start"] <= x["end"] < c.depth.size, c.name
    assert tests > 500


def test_restatement_equals_the_reference(golden):
    for c in K.all_cases():
        g = golden[c.name]
        r = K.restated(c)
        if c.stage in ("block", "merge"):
            agree(g["out"], r[0], c.name)
            continue
        rec = r[-1]
        if c.expect.get("crossed_refine"):       # the reference's second call has no defined behaviour: not in the golden file
            assert "refined" not in g, c.name
        else:
            agree(g["refined"], rec["before_order"], (c.name, "refined"))
        agree(K.order_by_start(g["merged"]), rec["merged"], (c.name, "merged"))
        agree(g["tested"], rec["judged"], (c.name, "tested"), skip=("score",))      # the score is detectcnv's own line
        agree(g["kept"], r[2], (c.name, "kept"))
        if len(c.noncode):
            nc = [tuple(int(x) for x in reg) for reg in c.noncode]
            pos, want = g["expand"]
            assert [K.to_reference(nc, int(p)) for p in pos] == [int(w) for w in want], c.name
            assert set(K.junction_positions(nc, c.depth.size)) <= set(int(p) for p in pos)
        for x in rec["tested"]:
            assert x["score"] == (x["cnvmed"] - c.RDmedian) * math.sqrt(float(x["end"] - x["start"] + 1) / float(c.P["m"])), c.name


def test_tester_on_and_off_restate_the_same_answer():
    for c in K.all_cases():
        on, off = K.restated(c, True), K.restated(c, False)
        lists = (on[0],) if c.stage != "calls" else on[:3]
        for a, b in zip(lists, (off[0],) if c.stage != "calls" else off[:3]):
            assert len(a) == len(b) and all(K.same(x, y) for x, y in zip(a, b)), c.name


def test_no_decision_rests_on_the_tolerance():
    """Every neighbourhood test: cand_cases' rule (the sign of nu is that of a combination of grid values, far from 0; the spread's
    floor is taken for a variance of exactly 0 or one far from it).  The stages' own decisions on columns compared with a tolerance:
    the merge's p1 against p1 and against P.p, sd_filters' p1 and cnvsd thresholds -- each a thousand tolerances from its threshold,
    or between values that are the same bits because they come from the same statistics.  Everything else the stages decide on is an
    integer, a grid value or the caller's own number."""
    far = lambda a, b: abs(a - b) > 1e-3 * max(abs(a), abs(b))
    for c in K.all_cases():
        r = K.restated(c)
        for t in r[-1]["tests"]:
            if t["nu"] is None:
                continue
            assert abs(t["nu_num"]) > 1e-3 * t["nu_scale"], (c.name, t["nu_num"])
            assert t["ref_var"] >= 0 and t["cnv_var"] >= 0, c.name
            assert t["ref_var"] == 0.0 or t["nwin"] * 2.0 ** -53 * float(t["means"].max()) ** 2 < 1e-2 * abs(t["ref_var"] - 1e-6), (c.name, t["ref_var"])
        if c.stage != "block":
            for i, how, p_first, p_second, _ in r[-1]["overlap"]:
                if p_first is None:
                    continue
                # (both dropped: which one stays is no decision; the tie case: both are the caller's own number, untouched)
                assert far(p_first, p_second) or min(p_first, p_second) > c.P["p"] or c.expect.get("tie"), (c.name, p_first, p_second)
                assert far(min(p_first, p_second), c.P["p"]), c.name
        if c.stage == "calls":
            sd = c.RDsd / 1.2
            for x in r[1]:
                assert far(x["p1"], 0.2) and far(x["p1"], 0.05), c.name
                assert x["cnvsd"] == 0.0 or (far(x["cnvsd"], 1.3 * sd) and far(x["cnvsd"], sd) and far(x["cnvsd"] * c.RDmedian, 2.5 * x["cnvmed"] * sd) and
                                             far(x["cnvsd"] * c.RDmedian, 2.0 * x["cnvmed"] * sd)), c.name


# ---- what the shortcuts rest on ---------------------------------------------------------------------------------------------------------------
def test_a_batch_result_that_may_be_used_is_the_serial_one():
    """For every first-round block test the batch may answer (road 0) the judgement against the list as it stood equals the judgement
    against the list as it stands; over the file, some that must be refused differ."""
    used = refused_equal = refused_differ = 0
    for c in K.all_cases():
        if c.stage != "block":
            continue
        _, rec = K.restated(c)
        for i, road in enumerate(rec["road"]):
            if road == 0:
                assert K.same(rec["stale"][i], rec["serial"][i]), (c.name, i)
                used += 1
            elif road in (2, 3):
                if K.same(rec["stale"][i], rec["serial"][i]):
                    refused_equal += 1
                else:
                    refused_differ += 1
    assert used > 200 and refused_differ >= 2 and refused_equal >= 2


def test_a_result_launched_ahead_that_may_be_used_is_the_serial_one():
    hits = chains = fields = differ = 0
    for c in K.all_cases():
        if c.stage == "block":
            continue
        for where, i, how, equal in K.restated(c)[-1]["spec"]:
            hits += how == "hit"
            chains += how == "chains"
            fields += how == "fields"
            differ += not equal
            # ('hit' is judged from the very plan it was launched with: the device's answer to the same question)
    assert hits >= 40 and chains >= 6 and fields >= 1 and differ >= 6


# ---- the claims ---------------------------------------------------------------------------------------------------------------------------------
def test_block_batch_threshold_and_refusals():
    for nseg in (23, 24):
        for c in both(f"block_{nseg}"):
            out, rec = K.restated(c)
            assert len(c.cands) == nseg and rec["batch"] == (nseg >= 24) and rec["road"] == [0 if nseg >= 24 else 1] * nseg, c.name
            assert rec["info"]["block_batch_hits"] == c.expect["hits"] and rec["info"]["waits"] == (1 if nseg >= 24 else 0)
            assert all(x["geno"] == 1 and x["status"] == 1 for x in out), c.name
    for name in ("block_unsorted", "block_holds_rejected"):
        for c in both(name):
            _, rec = K.restated(c)
            assert len(c.cands) >= 24 and not rec["batch"] and rec["sorted"] is False and set(rec["road"]) == {1}, c.name
    for c in both("block_cut"):
        _, rec = K.restated(c)
        cut = [t["plan"]["cut"] & 1 for t in rec["tests"][:60]]
        assert cut == [0] * 49 + [1] * 11 and rec["road"] == [0] * 49 + [3] * 11, c.name


def test_block_reach():
    for c in both("block_reach_outside"):
        _, rec = K.restated(c)
        i, j = c.expect["rejected"], c.expect["probe"]
        assert rec["serial"][i]["status"] == -9 and rec["rejected_before"][j] == c.cands[i]["end"] == rec["reach"][j] - 1, c.name
        assert rec["road"][j] == 0 and set(rec["road"]) == {0} and rec["serial_reach"][j] == rec["reach"][j], c.name
    for name in ("block_reach_inside_by_one", "block_reach_inside"):
        for c in both(name):
            _, rec = K.restated(c)
            i, j = c.expect["rejected"], c.expect["probe"]
            assert rec["serial"][i]["status"] == -9 and rec["rejected_before"][j] == c.cands[i]["end"] > rec["reach"][j], c.name
            if name == "block_reach_inside_by_one":      # on the boundary: the rejected segment's last bin is the walk's last position and fills
                assert rec["serial_reach"][j] == c.cands[i]["end"], c.name          # its last slot, one bin left of where `outside` stops;
                assert rec["reach"][j] == c.cands[i]["start"] - 2, c.name           # the stale walk jumped from it and took one bin behind it
            assert rec["road"][j] == 2 and rec["road"].count(0) == len(rec["road"]) - 1, c.name
            if name == "block_reach_inside":          # the stale judgement is another: the refusal matters.  (With one bin of the rejected
                assert rec["stale"][j]["refmed"] != rec["serial"][j]["refmed"] and not K.same(rec["stale"][j], rec["serial"][j]), c.name    # segment
                # walked through the neighbourhood's variance differs too, but p1 is 0 either way and the quantiles stay in their buckets.)
    for c in both("block_rejected_first"):
        _, rec = K.restated(c)
        assert rec["serial"][0]["status"] == -9 and rec["road"][1] == 2 and c.cands[0]["end"] >= rec["reach"][1], c.name
        assert K.same(rec["stale"][1], rec["serial"][1]), c.name                  # list index 0 is never skipped: refused on the safe side


def test_block_second_round():
    seen = set()
    for c in K.all_cases():
        if "block_rescue" not in c.name:
            continue
        out, rec = K.restated(c)
        j = c.expect["probe"]
        x = rec["serial"][j]
        assert x["status"] == -9 and x["geno"] == 0 and rec["rescued"][j] == c.expect["rescued"], c.name
        bound = 0.7 * x["refmed"] if x["type"] == DEL else 1.3 * x["refmed"]
        assert (x["cnvmed"] < bound if x["type"] == DEL else x["cnvmed"] > bound) == c.expect["rescued"] and abs(x["cnvmed"] - bound) < 1.0, c.name
        assert (out[j]["geno"], out[j]["p1"]) == ((1, c.P["p"]) if c.expect["rescued"] else (0, x["p1"])), c.name
        seen.add((x["type"], c.expect["rescued"]))
    assert len(seen) == 4
    for name in ("longest", "none", "level0"):
        for c in both(f"block_levels_{name}"):
            out, rec = K.restated(c)
            n1 = rec["nested"][1]
            runs = c.expect["runs"]
            tested = {(x["start"], x["end"]) for x in n1["levels"]}
            assert (runs["A"][0], runs["A"][1]) in tested and (runs["B"][0], runs["B"][1]) in tested, c.name
            assert (runs["D"][0], runs["D"][1]) not in tested, c.name             # the last run of a level is never emitted
            assert 3 in [abs(v) for v in n1.get("absent", [])], c.name            # level 3 is absent
            assert n1["restored"] == c.expect["restored"], c.name
            if c.expect["chosen"]:
                s, e, _ = runs[c.expect["chosen"]]
                assert (out[1]["start"], out[1]["end"], out[1]["geno"]) == (s, e, 1), c.name
            else:
                assert K.same(out[1], rec["serial"][1]) and all(x["geno"] == 0 for x in n1["levels"]), c.name
            if name == "longest":
                passing = {(x["start"], x["end"]) for x in n1["levels"] if x["geno"]}
                assert passing == {(runs["A"][0], runs["A"][1]), (runs["B"][0], runs["B"][1])}, c.name
            assert bool(n1.get("level0_skipped")) == (name == "level0" or c.cands[1]["type"] == DUP), c.name
            # the sparse form is asked in front of its first range, behind its last, between two, and inside
            ranges = K.sparse_ranges(c.status)
            kinds = {K.sparse_lookup_kind(ranges, i) for i in rec["reads"]}
            assert kinds == {"before", "after", "between", "inside"}, (c.name, kinds)


def test_merge_overlaps_and_near_pairs():
    for c in both("merge_types_differ") + both("merge_off"):
        out, Kc, rec = K.restated(c)
        assert len(out) == 2 and Kc["tests"] == 0 and not rec["overlap"] and not rec["near"], c.name
    for name in ("merge_overlap_union", "merge_overlap_first_wins", "merge_overlap_second_wins", "merge_overlap_both_dropped",
                 "merge_overlap_equal_p1", "merge_overlap_chain", "merge_overlap_tie"):
        for c in both(name):
            out, Kc, rec = K.restated(c)
            assert [o[1] for o in rec["overlap"]] == c.expect["overlap"] and len(out) == c.expect["out"], (c.name, rec["overlap"])
            if "union" in c.expect:
                assert (out[0]["start"], out[0]["end"]) == c.expect["union"], c.name
            if c.expect.get("equal_p1"):
                assert rec["overlap"][0][2] == rec["overlap"][0][3] > c.P["p"], c.name
            if c.expect.get("tie"):       # equal p1 at most P.p: the first stays, and it shows in the output
                _, how, p_first, p_second, geno = rec["overlap"][0]
                assert p_first == p_second == 0.001 <= c.P["p"] and geno == 1 and out[0]["status"] == 0, c.name
                assert (out[0]["start"], out[0]["end"]) == (c.cands[0]["start"], c.cands[0]["end"]) != (c.cands[1]["start"], c.cands[1]["end"]), c.name
            if "wins" in name:
                lo, hi = sorted(rec["overlap"][0][2:4])
                assert lo < c.P["p"] < hi and out[0]["p1"] == lo, c.name
            if "both_dropped" in name:
                assert min(rec["overlap"][0][2:4]) > c.P["p"], c.name
    for w1, w2 in ((400, 200), (200, 400)):
        for gap in (699, 700, 701):
            for c in both(f"merge_gap_{w1}_{w2}_{gap}"):
                _, _, rec = K.restated(c)
                a, b = c.cands
                assert (a["end"] - a["start"], b["end"] - b["start"], b["start"] - a["end"]) == (w1, w2, gap), c.name
                assert max(w1, w2) * c.P["chklen"] * 0.7 == 700.0 and (rec["near"] == [0]) == (gap <= 700) == c.expect["near"], c.name
    for which in (0, 1):
        for c in both(f"merge_geno0_{which}"):
            out, Kc, rec = K.restated(c)
            assert not rec["near"] and len(out) == 2 and Kc["sum_launches"] == 0, c.name
    for side in ("joins", "apart"):
        for c in both(f"merge_depth_rule_{side}"):
            out, Kc, rec = K.restated(c)
            assert rec["near"] == [0] and rec["sums"][0][3] == c.expect["rule"] and Kc["tests"] == (1 if c.expect["rule"] else 0), c.name
            assert len(out) == (1 if c.expect["rule"] else 2), c.name


def test_merge_stale_sums_and_stale_tests():
    for c in both("merge_chain_redone"):
        out, Kc, rec = K.restated(c)
        assert rec["near"] == [0, 1], c.name
        pair, used, stale, serial = rec["sums"][1]
        assert pair == 1 and used == (False, True, False) and stale is not None and stale != serial, c.name       # the stale sums would have given another answer
        assert rec["sums"][0][1] == (True, True, True) and rec["spec"][0][2] == "hit", c.name
        assert Kc["sum_redone"] == 2 and Kc["sum_reused"] == 6 + 3 + 1, c.name
        if serial:                                                                          # the pair's test, launched ahead for other members, is refused
            assert rec["spec"][1][:3] == ("merge", 1, "fields"), c.name
    for c in both("merge_chains_changed"):
        out, Kc, rec = K.restated(c)
        by_pair = {s[0]: s for s in rec["sums"]}
        assert by_pair[2][1] == (True, True, True) and by_pair[2][2] == by_pair[2][3], c.name    # pair (2, 3)'s sums still hold
        refused = [s for s in rec["spec"] if s[1] == 2]
        assert refused == [("merge", 2, "chains", False)], (c.name, rec["spec"])                 # ... its test does not, and would have been another
        assert by_pair[1][2] is None and not by_pair[1][3], c.name                                                     # the third stays apart from the merged pair
        assert len(out) == 2 and Kc["spec_hits"] == 1 and Kc["single_tests"] == 1, c.name


def test_calls_lists_and_speculation():
    for c in both("calls_clamp_drop"):
        blocks, raw, kept, Kc, rec = K.restated(c)
        assert rec["dropped"] == c.expect["dropped"] and len(blocks) == 6 and len(rec["based"]) == 4, c.name
        assert rec["based"][-1]["end"] == c.depth.size - 1 and c.cands[-1]["end"] * c.P["m"] + c.P["m"] // 2 > c.depth.size - 1, c.name
        assert rec["sharpen"][-1][0]["early"] == "end", c.name          # the refinement leaves the clamped call alone
    want = dict(middle=["hit", "hit", "chains", "chains"], first=["hit"] * 4, before_last=["hit", "hit", "hit", "chains"], last=["hit"] * 4)
    for where, roads in want.items():
        for c in both(f"calls_final_rejects_{where}"):
            blocks, raw, kept, Kc, rec = K.restated(c)
            w = c.expect["weak"]
            assert [s[2] for s in rec["spec"] if s[0] == "final"] == roads and rec["judged"][w]["status"] == -9 and len(raw) == 3, (c.name, rec["spec"])
            assert Kc["spec_hits"] == roads.count("hit") and Kc["single_tests"] == roads.count("chains"), c.name
            if "chains" in roads:
                first = next(s for s in rec["spec"] if s[2] == "chains")
                assert first[1] == w + 1 and first[3] is False, c.name        # the result launched ahead for w + 1 is another than the serial one
    for c in both("calls_starts_cross"):
        blocks, raw, kept, Kc, rec = K.restated(c)
        a, b = rec["based"]
        a2, b2 = rec["before_order"]
        assert a["start"] < b["start"] and a2["start"] > b2["start"] and b2["start"] == b["start"], c.name
        assert [x["start"] for x in rec["sharpened"]] == [b2["start"], a2["start"]], c.name


def test_calls_regions_and_filters():
    for c in both("calls_regions"):
        blocks, raw, kept, Kc, rec = K.restated(c)
        nc = [tuple(int(x) for x in r) for r in c.noncode]
        assert nc[0][0] == 0 and len(nc) == 3, c.name
        for p in K.junction_positions(nc, c.depth.size):
            q = K.to_reference(nc, p)
            assert not any(s <= q <= e for s, e in nc), c.name             # never a position inside a region
        j = 20000 - 2000                                                   # the third junction, compacted
        assert (K.to_reference(nc, j - 1), K.to_reference(nc, j)) == (19999, 20100), c.name
        x = rec["tested"][c.expect["spanning"]]
        assert x["start"] < j <= x["end"] and x["status"] == -9 and rec["judged"][c.expect["spanning"]]["status"] == 1 and len(raw) == 2, c.name
        assert all(r["start"] == K.to_reference(nc, t["start"]) for r, t in zip(raw, rec["tested"])), c.name
    for span in (499, 500, 800, 801, 999, 1000, 901, 902):
        for c in both(f"calls_{'minlen' if span in (901, 902) else 'span'}_{span}"):
            blocks, raw, kept, Kc, rec = K.restated(c)
            assert len(raw) == 1 and raw[0]["end"] - raw[0]["start"] == span == rec["filters"][0][0], (c.name, raw[0]["start"], raw[0]["end"])
            minlen = max(2 * c.P["m"], 500)
            del_rescue = raw[0]["type"] == DEL and span > 800
            assert rec["filters"][0][2] == del_rescue, c.name
            assert bool(kept) == ((span >= 1000 or del_rescue) and span >= minlen), (c.name, span)
            if span < 900:
                assert rec["sharpen"][0][0]["win"][0][4] > 0 and rec["sharpen"][0][0]["win"][1][4] > 0, c.name      # both edges were carried onto the steps
    assert [bool(K.restated(K.get_case(f"calls_minlen_{s}_del"))[2]) for s in (901, 902)] == [False, True]


def test_calls_at_the_junctions_and_a_crossed_refinement(golden):
    """A call's refined edge on j - 1, j and j + 1 of each junction of to_reference, the region that starts at 0 included: the edges are
    where the case says, a call with j inside (first, last] is dropped by the N-region filter, the others come out expanded as the
    reference's expand_coordinate expands them (golden `expand`) -- a call that ends on j - 1 ends one base in front of the region."""
    seen = set()
    for c in K.all_cases():
        if "calls_junction" not in c.name:
            continue
        blocks, raw, kept, Kc, rec = K.restated(c)
        first, last = c.expect["edges"]
        j = c.expect["junction"]
        nc = [tuple(int(x) for x in r) for r in c.noncode]
        t = rec["tested"][0]
        assert (t["start"], t["end"]) == (first, last) and rec["judged"][0]["status"] == 1, c.name
        if c.expect.get("unrefined"):
            assert rec["sharpen"][0][0]["early"] == "start", c.name
        else:
            assert rec["sharpen"][0][0]["win"][0][4] > 0 and rec["sharpen"][0][0]["win"][1][4] > 0, c.name
        assert c.expect["kept"] == (not (first < j <= last)) == (len(raw) == 1) == (t["status"] != -9), c.name
        back = dict(zip(*(a.tolist() for a in golden[c.name]["expand"])))
        if raw:
            assert (raw[0]["start"], raw[0]["end"]) == (back[first], back[last]), c.name
            region = next(r for r in nc if r[1] + 1 - sum(e - s + 1 for s, e in nc if e <= r[1]) == j)
            if last == j - 1:
                assert raw[0]["end"] == region[0] - 1, c.name
            if first == j:
                assert raw[0]["start"] == region[1] + 1, c.name
        seen.add((j, first - j if abs(first - j) <= 1 else None, last - j if abs(last - j) <= 1 else None))
    assert seen == {(j, a, None) for j in (4000, 18000) for a in (-1, 0, 1)} | {(j, None, a) for j in (4000, 18000) for a in (-1, 0, 1)} | \
        {(0, 0, None), (0, 1, None)}
    for c in both("calls_refined_crossed"):
        blocks, raw, kept, Kc, rec = K.restated(c)
        b = rec["before_order"][0]
        assert b["end"] < b["start"] and not K.sc.stays_inside(rec["sharpen"][0]), c.name
        assert (rec["sharpened"][0]["start"], rec["sharpened"][0]["end"]) == (b["end"], b["start"]), c.name      # the swap
