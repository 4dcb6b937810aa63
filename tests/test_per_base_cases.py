"""CPU: the cases of tests/per_base_cases.py are what golden/per_base_edges.npz was made from, the oracle reproduces the reference's
answers on every one of them (nothing else pins oracle/rsi_oracle.cpp at chromosomes of 4040 bases, eight bins or a cap of 63), and
every case lands on the route, form and residue it was built for -- recomputed here from the ORACLE's cap median, n' and regions
with the kernels' thresholds restated as constants, so that a changed seed which moves a case off its edge fails here.
GPU (the one test marked so): per_base_cases.gc_wide_case(), the redo rung a depth of 2^21 takes, against the oracle."""
import numpy as np
import pytest

import per_base_cases as pc
from golden_util import sha

# ---- the thresholds, restated (source line of each in the comment) ----
K_BYTE_SAT = 254          # kernels.h: constexpr int kByteSat = 254 (cap_compact8_applies: capval < kByteSat)
K_WIDE_END = 32767        # kernels_base.hip, cap_compact16_applies: capval < 32767
K_BYTE_M_MAX = 440        # kernels_base.hip, cap_compact8_applies / cap_compact16_applies: m <= 440
K_REG_INLINE = 48         # kernels.h: constexpr int kRegInline = 48
K_REG_LDS = 128           # per_base_device.h: constexpr int kRegLds = 128
K_MIN_BINS_FACTOR = 8     # kernels_k4s.hip, k4s_config_fits: ncompact >= m * 8; pipeline.hip: nb < 8 is RSI_ERR_TOO_SMALL
K_SUB = 2048              # kernels_k4s.hip: one K4s sub-tile per wave trip
K_MIN_N = 4040            # pipeline.hip, run_enter: n / 20 <= 201 is refused (gccontent.cpp:66-71)
K_M_MAX = 3000            # pipeline.hip, run_enter: m > 3000 is refused


def vr_of(capval):        # kernels.h, byte_shape: 64 -> 128 at 64, 128 -> 256 at 128
    return 64 if capval <= 63 else 128 if capval <= 127 else 256


def sw7_of(capval):       # kernels.h, byte_shape: capval <= 127
    return capval <= 127


def parts_of(m):          # kernels_k4s.hip, launch_bin_median8: m <= 52 ? 2 : m <= 104 ? 4 : m <= 216 ? 8 : 16
    return 2 if m <= 52 else 4 if m <= 104 else 8 if m <= 216 else 16


def tile_bins_of(m):      # kernels_base.hip, k48_bins_per_tile: m <= 52 ? 128 : m <= 104 ? 64 : m <= 216 ? 32 : 16
    return 128 if m <= 52 else 64 if m <= 104 else 32 if m <= 216 else 16


def int32_form(m):        # kernels_base.hip, k4_geometry and launch_cap_compact_bin (256 threads)
    tb = 64
    while tb > 4 and tb * m * 4 > 48 * 1024:
        tb //= 2
    quads = (tb * m + 3) // 4
    maxv, ept = -(-quads // 256), -(-m // (256 // tb))
    return tb, (413 if maxv <= 4 and ept <= 13 else 826 if maxv <= 8 and ept <= 26 else 1352 if ept <= 52 else 1300)


def landing(capval, m, nreg, gc):
    """route, vr, sw7, parts, tile_bins, tmpl, reg_class for what the oracle derived (kernels_base.hip, k4_plan: default switches)."""
    reg = "inline" if nreg <= K_REG_INLINE else "lds" if nreg <= K_REG_LDS else "hbm"
    if capval is not None and 1 <= capval < K_BYTE_SAT and m <= K_BYTE_M_MAX:
        if nreg <= K_REG_LDS:
            return ("stream", vr_of(capval), sw7_of(capval), parts_of(m), None, None, reg)
        return ("joint" if gc else "bytes", vr_of(capval), sw7_of(capval), None, tile_bins_of(m), None, reg)
    if capval is not None and K_BYTE_SAT <= capval < K_WIDE_END and m <= K_BYTE_M_MAX:
        return ("wide16", 512, None, None, tile_bins_of(m), None, reg)
    tb, tmpl = int32_form(m)
    return ("int32", None, None, None, tb, tmpl, reg)


@pytest.fixture(scope="module")
def oracle_runs(oracle_cls):
    """Every case through the oracle's per-base stages, once: {id: dict of its arrays and scalars}."""
    import oracle
    O = oracle_cls()
    out = {}
    for cid in pc.case_ids():
        case = pc.get_case(cid)
        fasta, depth = pc.checker_inputs(case)
        O.run_per_base(oracle.make_params(**case[3]), depth, fasta)
        ch = O.f64("chrom")
        out[cid] = dict(rd_gc=O.i32("rd_gc"), rd_cap=O.i32("rd_cap"), rd_concat=O.i32("rd_concat"), noncode=O.i32("noncode"),
                        binmedint=O.i32("binmedint"), RDmedian=ch[0], RDsd=ch[1],
                        cap_median=ch[2] if case[3]["cap"] > 1 else 0.0, gc_rdmean=ch[3] if case[3]["gcadjust"] else 0.0)
    return out


def test_the_golden_file_holds_exactly_these_cases():
    G = pc.load_golden()
    assert sorted(G) == sorted(pc.case_ids())
    assert len(pc.case_ids()) == len(set(pc.run_order())) + len([c for c in pc.case_ids() if c.startswith("seq_")])


@pytest.mark.parametrize("cid", pc.case_ids())
def test_inputs_hash_to_the_golden_file(cid):
    g = pc.load_golden()[cid]
    _, fasta, depth, flags, _, _ = pc.get_case(cid)
    assert flags == g["flags"]
    assert sha(fasta) == g["fasta_sha"] and sha(depth) == g["depth_sha"]
    assert fasta.dtype == np.uint8 and depth.dtype == np.int32 and K_MIN_N <= depth.size <= 300_000 and flags["m"] < K_M_MAX


@pytest.mark.parametrize("cid", pc.case_ids())
def test_oracle_reproduces_the_reference(cid, oracle_runs):
    g, o = pc.load_golden()[cid], oracle_runs[cid]
    assert np.array_equal(o["noncode"], g["noncode"]), "regions"
    for name in ("rd_gc", "rd_cap", "rd_concat"):
        assert sha(o[name]) == g[name + "_sha"], name
    assert o["rd_concat"].size == g["n_compact"] and o["binmedint"].size == g["nbins"]
    assert sha(o["binmedint"]) == g["binmedint_sha"]
    if g["binmedint"] is not None:
        assert np.array_equal(o["binmedint"], g["binmedint"])
    assert (o["RDmedian"], o["RDsd"], o["cap_median"], o["gc_rdmean"]) == tuple(g["chrom"])


@pytest.mark.parametrize("cid", pc.case_ids())
def test_case_lands_where_it_was_built_to_land(cid, oracle_runs):
    _, _, depth, flags, _, ex = pc.get_case(cid)
    o, m = oracle_runs[cid], flags["m"]
    capval = int(o["cap_median"] * flags["cap"]) if flags["cap"] > 1 else None       # loaddata.cpp:238
    ncompact, nreg = o["rd_concat"].size, o["noncode"].size // 2
    assert ncompact == ex["ncompact"] and nreg == ex["nreg"]
    assert (ncompact // m < K_MIN_BINS_FACTOR) == (ex["error"] == "RSI_ERR_TOO_SMALL")
    if ex["error"]:
        return
    if ex["cap_exact"]:
        assert capval == ex["capval"]
    got = landing(capval, m, nreg, bool(flags["gcadjust"]))
    want = (ex["route"], ex["vr"], ex["sw7"], ex["parts"], ex["tile_bins"], ex["tmpl"], ex["reg_class"])
    assert got == want
    assert got == landing(ex["capval"], m, ex["nreg"], bool(flags["gcadjust"])), "the intended cap value is of another class"


def _landed(oracle_runs, pred):
    """ids of the cases (errors left out unless asked for) whose oracle-derived numbers satisfy pred(capval, m, n, n', nreg, flags, ex)."""
    hit = []
    for cid in pc.case_ids():
        _, _, depth, flags, _, ex = pc.get_case(cid)
        o = oracle_runs[cid]
        capval = int(o["cap_median"] * flags["cap"]) if flags["cap"] > 1 else None
        if pred(capval, flags["m"], depth.size, o["rd_concat"].size, o["noncode"].size // 2, flags, ex):
            hit.append(cid)
    return hit


def test_every_boundary_has_a_case_on_each_side(oracle_runs):
    """The issue's table, row by row, from what the oracle derived."""
    def have(pred, what):
        assert _landed(oracle_runs, lambda *a: a[6]["error"] is None and pred(*a)), what
    for gc in (1, 0):
        byte_m = lambda m: m <= K_BYTE_M_MAX
        for cv in (63, 64, 127, 128, 253, 254):
            have(lambda c, m, n, nc, nr, f, ex: c == cv and byte_m(m) and f["gcadjust"] == gc, f"cap value {cv}, gcadjust {gc}")
        have(lambda c, m, n, nc, nr, f, ex: c is None and f["gcadjust"] == gc, f"no cap, gcadjust {gc}")
    for cv in (32766, 32767):
        have(lambda c, m, n, nc, nr, f, ex: c == cv, f"cap value {cv}")
    byte_cap = lambda c: c is not None and 1 <= c < K_BYTE_SAT
    for gc in (1, 0):                       # m classes x the three byte cap classes: every k_bin_median8<SW7, PARTS>, and RAW K4s
        for m0 in (51, 53, 103, 105, 215, 217, 439):
            for lo, hi in ((1, 63), (64, 127), (128, 253)):
                have(lambda c, m, n, nc, nr, f, ex: m == m0 and byte_cap(c) and lo <= c <= hi and nr <= K_REG_LDS and f["gcadjust"] == gc,
                     f"m {m0}, cap {lo}..{hi}, gcadjust {gc}")
        have(lambda c, m, n, nc, nr, f, ex: m == 441 and byte_cap(c) and f["gcadjust"] == gc, f"m 441 under a byte cap, gcadjust {gc}")
    for m0 in (51, 101, 201, 401):          # K4w in each bins-per-tile class
        have(lambda c, m, n, nc, nr, f, ex: tile_bins_of(m) == tile_bins_of(m0) and c is not None and K_BYTE_SAT <= c < K_WIDE_END, f"K4w, m {m0}")
    for m0 in (51, 53, 103, 105, 191, 193, 441, 2999):   # the int32 K4's templates
        have(lambda c, m, n, nc, nr, f, ex: m == m0 and landing(c, m, nr, True)[0] == "int32", f"int32 K4, m {m0}")
    assert {int32_form(m0)[1] for m0 in (51, 53, 103, 105, 191, 193, 441, 2999)} == {413, 826, 1352}   # <13, 0> needs m > 3000: unreachable
    for k in (0, 48, 49, 128, 129):
        for gc in (1, 0):
            have(lambda c, m, n, nc, nr, f, ex: nr == k and f["gcadjust"] == gc, f"{k} regions, gcadjust {gc}")
    for k in (49, 129):                     # the LDS-mirrored and the HBM list through K4w's and the int32 K4's staging and walk
        for route in ("wide16", "int32"):
            have(lambda c, m, n, nc, nr, f, ex: nr == k and landing(c, m, nr, True)[0] == route, f"{k} regions, {route}")
    assert _landed(oracle_runs, lambda c, m, n, nc, nr, f, ex: nc - 8 * m == -1 and ex["error"] == "RSI_ERR_TOO_SMALL")
    for d in (0, 1):
        have(lambda c, m, n, nc, nr, f, ex: nc - 8 * m == d, f"n' = 8 m + {d}")
    for v in (K_SUB - 1, K_SUB, K_SUB + 1):
        have(lambda c, m, n, nc, nr, f, ex: nc == v, f"n' = {v}")
    for r in (0, 30):
        have(lambda c, m, n, nc, nr, f, ex: nc % 31 == r, f"n' mod 31 = {r}")
    have(lambda c, m, n, nc, nr, f, ex: nc % m == 0, "n' mod m = 0")
    have(lambda c, m, n, nc, nr, f, ex: nc % m == m - 1, "n' mod m = m - 1")
    have(lambda c, m, n, nc, nr, f, ex: n == K_MIN_N, "the smallest n")
    for r in (0, 1, 19):
        have(lambda c, m, n, nc, nr, f, ex: n % 20 == r and nr == 0, f"n mod 20 = {r} without N")
    for r in range(4):
        have(lambda c, m, n, nc, nr, f, ex: n % 4 == r, f"n mod 4 = {r}")
    for r in (0, 63):
        have(lambda c, m, n, nc, nr, f, ex: n % 64 == r, f"n mod 64 = {r}")


def test_layout_cases_are_laid_out_as_named(oracle_runs):
    n = pc.get_case("nrun_at_0")[1].size
    assert oracle_runs["nrun_at_0"]["noncode"][0] == 0
    assert oracle_runs["nrun_to_end"]["noncode"][-1] == n - 1
    both = oracle_runs["nrun_both_ends_nogc"]["noncode"]
    assert both[0] == 0 and both[-1] == n - 1
    fasta = pc.get_case("nrun_end_word64")[1]
    ends = np.flatnonzero((fasta[:-1] == ord("N")) & (fasta[1:] != ord("N"))) + 1      # first base behind each N run
    assert ends[0] % 64 == 0
    assert (oracle_runs["nrun_end_word64"]["noncode"][3] + 1) % 64 == 0                # and a padded region that ends on a mask word
    nc = oracle_runs["nrun_cut_2048"]["noncode"]
    assert nc[0] % K_SUB == 0 and (nc[2] - (nc[1] - nc[0] + 1)) % K_SUB == 0            # both cuts on a sub-tile, compacted coordinates


@pytest.mark.parametrize("cid", [f"m{m}_cap{t}_{g}" for g in ("gc", "nogc") for m in (51, 105, 439) for t in pc.CAP_CLASSES])
def test_a_bin_holds_the_cap_its_neighbours_and_has_it_as_median(cid, oracle_runs):
    _, _, _, flags, _, _ = pc.get_case(cid)
    o, m = oracle_runs[cid], flags["m"]
    capval = int(o["cap_median"] * flags["cap"])
    assert o["noncode"].size == 0                     # compacted index = index
    pre = o["rd_gc"][:o["binmedint"].size * m].reshape(-1, m)
    ok = [(row == capval - 1).any() and (row == capval).any() and (row == capval + 1).any() and med == capval
          for row, med in zip(pre, o["binmedint"])]
    assert any(ok)


@pytest.mark.parametrize("cid", ["escape_edges_cap253_gc", "escape_edges_cap120_gc", "escape_edges_cap253_nogc"])
def test_escape_values_sit_at_the_cut_and_on_the_last_base(cid):
    _, fasta, depth, flags, _, _ = pc.get_case(cid)
    (a, b), = pc.merged_regions(depth.size, [(8000, 100)], flags["m"])
    assert sorted(depth[a - 3:a]) == [254, 255, 256] == sorted(depth[b + 1:b + 4]) == sorted(depth[-3:])
    assert (fasta[a - 3:a] != ord("N")).all() and depth[-1] == 255


@pytest.mark.gpu
def test_gc_wide_redo_against_the_oracle(oracle_cls):
    """GPU: a depth of 2^21 under RSI_HOT_JOINT=0 sends the three-pass chain round again with the two-atomic K2 (pipeline.hip, per_base_phase:
    "a2-3.gc wide redo"); per-base arrays, bin medians and the chromosome's scalars as the oracle's per-base stages give them (RDsd: rel
    1e-12, the bar of tests/test_per_base_edges.py and tests/test_fallback_paths.py for the same number)."""
    import os
    import oracle
    from rsicnv_amd import api
    fasta, depth, flags = pc.gc_wide_case()
    assert depth.size == K_MIN_N and (depth == 1 << 21).sum() == 1 and (depth == (1 << 21) - 1).sum() == 1 and depth.max() == 1 << 21
    O = oracle_cls()
    O.run_per_base(oracle.make_params(**flags), depth, fasta)
    ch = O.f64("chrom")
    hot = api.RsiHot(0)
    hot.set_timing(1)
    os.environ["RSI_HOT_JOINT"] = "0"
    try:
        st = hot.debug_per_base(api.make_params(**flags), depth, fasta)
        phases, kernels = dict(hot.phase_times()), [k for k, _ in hot.kernel_times()]
        got = {name: hot.fetch(name) for name in ("rd_gc", "rd_concat", "binmedint")}
    finally:
        del os.environ["RSI_HOT_JOINT"]
        hot.close()
    print(f"phases {sorted(phases)} kernels {kernels} RDmedian {st['RDmedian']} RDsd {st['RDsd']!r} / {ch[1]!r} cap median {st['cap_median']} rdmean {st['gc_rdmean']!r}")
    assert "a2-3.gc wide redo" in phases and "gc_hist_wide" in kernels and "gc_joint_hist" not in kernels, (phases, kernels)
    for name in ("rd_gc", "rd_concat", "binmedint"):
        assert np.array_equal(got[name], O.i32(name)), name
    assert (st["RDmedian"], st["cap_median"], st["gc_rdmean"]) == (ch[0], ch[2], ch[3])
    assert st["RDsd"] == pytest.approx(ch[1], rel=1e-12)
    assert st["byte_escapes"] == 2
