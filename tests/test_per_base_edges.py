"""GPU: the per-base phase alone (RsiHot.debug_per_base) on the cases of tests/per_base_cases.py -- every threshold of k4_plan and
of the K4 launchers from both sides, the smallest chromosomes, the N-run layouts -- against the compiled reference's answers in
golden/per_base_edges.npz: per-base arrays, regions, bin medians and sums bit for bit, the scalars exactly (RDsd: rel 1e-12, as
tests/test_fallback_paths.py), and the route AND the form inside it as the run itself reports them (phase and kernel names, the
"k4.form ..." entries the launchers fill).

(a) every case on one context, in an order that alternates short and long; (b) the cases whose route a switch changes, under
RSI_HOT_K4SPLIT=0, RSI_HOT_JOINT=0 and RSI_HOT_K4W=0; (c) the K4 queued behind K2j / the -NOGC histogram pass across shape edges, short
chromosomes and long region lists, with the accepted / rejected marker derived from the rule in pipeline.hip.

Wall time on an MI355X: 2.5 s for the file's 268 tests (pytest's own figure; 4 s with the interpreter's start), 4 ... 66 kb per run
through the per-base phase; the slowest is the first, which loads the library (1.5 s)."""
import os

import numpy as np
import pytest

import per_base_cases as pc
from golden_util import sha

pytestmark = pytest.mark.gpu

K4_MARKS = ("k4.split", "a5.k4w 16-bit tile", "a5.nogc byte path", "k4j.float rescale")
FORM_KEYS = (("vr", "k4.form vr"), ("sw7", "k4.form sw7"), ("parts", "k4.form parts"), ("tile_bins", "k4.form tile bins"),
             ("tmpl", "k4.form int32 template"))


@pytest.fixture(scope="module")
def hot():
    from rsicnv_amd import api
    h = api.RsiHot(0)
    h.set_timing(1)
    yield h
    h.close()


def _capval(g):
    return int(g["chrom"][2] * g["flags"]["cap"]) if g["flags"]["cap"] > 1 else None       # loaddata.cpp:238


def check_case(hot, cid, env=()):
    """One case through the hook, everything compared; returns the run's phases (name -> value)."""
    from rsicnv_amd import api
    _, fasta, depth, flags, exclude, ex = pc.get_case(cid)
    g = pc.load_golden()[cid]
    params = api.make_params(**flags)
    if ex["error"]:
        with pytest.raises(api.RsiError) as e:
            hot.debug_per_base(params, depth, fasta, exclude)
        assert ex["error"] in str(e.value)
        assert hot.last_stats["n_compact"] == g["n_compact"] and hot.last_stats["nbins"] == g["nbins"] < 8
        return dict(hot.phase_times())
    st = hot.debug_per_base(params, depth, fasta, exclude)
    phases, kernels = dict(hot.phase_times()), [k for k, _ in hot.kernel_times()]
    assert np.array_equal(hot.fetch("noncode"), g["noncode"]), "noncode"
    if flags["gcadjust"]:
        assert sha(hot.fetch("rd_gc")) == g["rd_gc_sha"], "rd_gc"
    rdc = hot.fetch("rd_concat")
    assert sha(rdc) == g["rd_concat_sha"], "rd_concat"
    medint, m = hot.fetch("binmedint"), flags["m"]
    assert sha(medint) == g["binmedint_sha"], "binmedint"
    if g["binmedint"] is not None:
        assert np.array_equal(medint, g["binmedint"]), "binmedint"
    assert np.array_equal(hot.fetch("binsum"), rdc[:medint.size * m].reshape(medint.size, m).sum(axis=1, dtype=np.int64)), "binsum"
    assert (st["n"], st["n_compact"], st["nbins"], st["n_noncode"]) == (depth.size, g["n_compact"], g["nbins"], g["noncode"].size // 2)
    print(f"{cid}: RDmedian {st['RDmedian']} RDsd {st['RDsd']!r} / {g['chrom'][1]!r} cap median {st['cap_median']} rdmean {st['gc_rdmean']!r}")
    assert st["RDmedian"] == g["chrom"][0] and st["cap_median"] == g["chrom"][2] and st["gc_rdmean"] == g["chrom"][3]
    assert st["RDsd"] == pytest.approx(g["chrom"][1], rel=1e-12)
    if flags["gcadjust"]:
        assert st["byte_escapes"] == int((depth >= 255).sum())
    # the route, and no other K4 kernel; the form inside it as the launcher reported it
    f = pc.form_for(_capval(g), m, g["n_compact"], g["noncode"].size // 2, bool(flags["gcadjust"]), env)
    want = set()
    if f["route"] == "stream":
        want.add("k4.split")
    if f["route"] == "wide16":
        want.add("a5.k4w 16-bit tile")
    if f["route"] in ("stream", "bytes") and not flags["gcadjust"]:
        want.add("a5.nogc byte path")
    assert {k for k in K4_MARKS if k in phases} == want, (f, phases)
    assert kernels.count("cap_compact_bin") == (2 if "spec.k4j rejected" in phases else 1), kernels   # (a rejected queued launch, then the real one)
    queued_k4m = "spec.k4j rejected" in phases and "K4SPLIT" not in env      # the queued launch is K4s + K4m unless that is switched off
    assert kernels.count("bin_median") == int(f["route"] == "stream") + int(queued_k4m), kernels
    if "JOINT" in env and flags["gcadjust"]:
        assert "gc_joint_hist" not in kernels and "gc_hist" in kernels and "value_hist8" in kernels, kernels
    for key, name in FORM_KEYS:
        if f[key] is not None:
            assert phases.get(name) == float(f[key]), (name, f, phases)
        elif key != "vr":
            assert name not in phases, (name, f, phases)
    return phases


@pytest.mark.parametrize("cid", pc.run_order())
def test_case_against_the_reference(hot, cid):
    check_case(hot, cid)


def test_a_chromosome_below_the_smallest_is_refused(hot):
    from rsicnv_amd import api
    _, fasta, depth, flags, _, _ = pc.get_case("n4040_gc")
    with pytest.raises(api.RsiError) as e:
        hot.debug_per_base(api.make_params(**flags), depth[:4039], fasta[:4039])
    assert "RSI_ERR_TOO_SMALL" in str(e.value)
    with pytest.raises(api.RsiError) as e:
        hot.debug_per_base(api.make_params(m=3001, cap=4.0), depth, fasta)
    assert "RSI_ERR_UNSUPPORTED" in str(e.value)
    check_case(hot, "n4040_gc")


def _route_changes(switch):
    out = []
    for cid in pc.run_order():
        _, _, _, flags, _, ex = pc.get_case(cid)
        if ex["error"] is None and pc.form_for(ex["capval"], flags["m"], ex["ncompact"], ex["nreg"], bool(flags["gcadjust"]), (switch,))["route"] != ex["route"]:
            out.append(cid)
    return out


@pytest.mark.parametrize("switch,cid", [(s, c) for s in ("K4SPLIT", "JOINT", "K4W") for c in _route_changes(s)])
def test_case_behind_a_switch(hot, switch, cid):
    """K4j and K4' (RSI_HOT_K4SPLIT=0), the three-pass chain's K4' (RSI_HOT_JOINT=0) and the int32 K4 (RSI_HOT_K4W=0) at the same edges."""
    os.environ["RSI_HOT_" + switch] = "0"
    try:
        check_case(hot, cid, env=(switch,))
    finally:
        del os.environ["RSI_HOT_" + switch]


def _sequences(m, g):
    caps = [f"seq_m{m}_cap{c}{g}" for c in pc.SEQ_CAPS]
    lens = [f"seq_m{m}_{w}{g}" for w in ("cap120", "short", "cap120", "reg49", "reg129", "cap120")]
    return caps, lens


@pytest.mark.parametrize("m,gc", [(m, 1) for m in pc.SEQ_M] + [(101, 0)])
def test_queued_k4_across_shape_edges(m, gc):
    """The K4 launched behind K2j in the shape of the context's previous cap: accepted only under the rule of pipeline.hip (per_base_phase:
    `spec` and `spec_done`) -- a previous byte cap under the same flags; then the same shape, a byte cap, n' >= 8 m, at most 128 regions --
    and a rejected launch leaves nothing behind: the run right after each rejection is compared like every other."""
    from rsicnv_amd import api
    hot = api.RsiHot(0)
    hot.set_timing(1)
    G = pc.load_golden()
    try:
        for seq in _sequences(m, "" if gc else "_nogc"):
            for cid in seq:
                g, ex = G[cid], pc.get_case(cid)[5]
                phases = check_case(hot, cid)
                prev = getattr(hot, "_prev_cap", None)       # the cap of this context's last chromosome that a byte form took
                capval, nreg = _capval(g), g["noncode"].size // 2
                launched = prev is not None and 1 <= prev < 254
                fits = 1 <= capval < 254 and pc.byte_shape(prev or 0) == pc.byte_shape(capval) and g["n_compact"] >= 8 * m and nreg <= 128
                want = None if (ex["error"] or not launched) else ("spec.k4j accepted" if fits else "spec.k4j rejected")
                got = [k for k in ("spec.k4j accepted", "spec.k4j rejected") if k in phases]
                assert got == ([want] if want else []), (cid, prev, capval, phases)
                if not ex["error"] and 1 <= capval < 254:
                    hot._prev_cap = capval
    finally:
        hot.close()
