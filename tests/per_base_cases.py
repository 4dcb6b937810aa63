"""Inputs for the per-base phase at its route boundaries and smallest sizes (tests/test_per_base_cases.py on the CPU,
tests/test_per_base_edges.py on the GPU; the reference's answers: tools/make_golden_per_base.py -> golden/per_base_edges.npz).

numpy only, seeded.  A case is (id, fasta, depth, flags, exclude, expect):

* flags    keyword arguments of make_params (m, cap, gcadjust);
* exclude  None, or (start, end) intervals the run treats as N (the CPU checkers get the same bases painted 'N');
* expect   what the case was BUILT for: capval (the cap value, None without a cap; cap_exact False: only its class is meant, the
           chromosome is so short or so full of N that the median of the uncompacted array moves), ncompact (n'), nreg, error (None or the status
           a chromosome of fewer than eight bins gets), and -- derived here from those intended numbers by form_for(), the restatement of
           k4_plan and the launchers -- route, vr, sw7, parts (K4m) or tile_bins, tmpl (the int32 K4's template, 100 MV + EP),
           reg_class.  tests/test_per_base_cases.py recomputes all of it from the ORACLE's cap median, n' and regions with the
           thresholds restated there: a case that a changed seed moves off its edge fails on the CPU.

The depth is spread like a Poisson depth symmetrically around mu, independent of the sequence, so that the GC adjustment moves
values by a percent or two and the median of the adjusted array is mu; the cap value (int)(median * cap) is then put on its edge through mu and the
`cap` flag (63 = (int)(30 * 63.5 / 30)), or, for the queued-K4 sequences that need ONE flag set, through mu alone at -cap 2.

Left out: kS4MaxTrips (kernels_k4s.hip), the 335 Mb beyond which K4s takes its long grid.  It cannot be small;
tests/test_full_size.py stays its only cover.
"""
import numpy as np

PAD_MIN = 50            # get_noseq_regions pads by max(50, m / 4) (loaddata.cpp:243-273)
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def pad_of(m):
    return max(PAD_MIN, m // 4)


def merged_regions(n, runs, m):
    """(start, end) inclusive of the removed regions for N runs [(start, length)]: padded, clamped, merged when they touch."""
    dx, out = pad_of(m), []
    for s, ln in sorted(runs):
        a, b = max(0, s - dx), min(n - 1, s + ln - 1 + dx)
        if out and a <= out[-1][1] + 1:
            out[-1][1] = max(out[-1][1], b)
        else:
            out.append([a, b])
    return out


def byte_shape(capval):
    vr = 64
    while vr < 256 and vr <= capval:
        vr <<= 1
    return vr, capval <= 127


def parts_of(m):
    return 2 if m <= 52 else 4 if m <= 104 else 8 if m <= 216 else 16


def form_for(capval, m, ncompact, nreg, gc, env=()):
    """Route and form for the intended numbers: k4_plan and the launchers restated (kernels_base.hip, kernels_k4s.hip).
    env: the switches that are off (names without the RSI_HOT_ prefix)."""
    f = dict(route="int32", vr=None, sw7=None, parts=None, tile_bins=None, tmpl=None,
             reg_class="inline" if nreg <= 48 else "lds" if nreg <= 128 else "hbm")
    capped = capval is not None
    bytes_fit = capped and 1 <= capval < 254 and m <= 440
    split = "K4SPLIT" not in env and bytes_fit and nreg <= 128
    if bytes_fit and (gc or "NOGC_BYTES" not in env):
        f["vr"], f["sw7"] = byte_shape(capval)
        if gc and "JOINT" in env:
            f["route"] = "bytes"
        elif split:
            f["route"] = "stream"
        else:
            f["route"] = "joint" if gc else "bytes"
        if f["route"] == "stream":
            f["parts"] = parts_of(m)
        else:
            f["tile_bins"] = 64 // parts_of(m) * 4
        f["raw"] = not gc
        return f
    if capped and "K4W" not in env and 254 <= capval < 32767 and m <= 440:
        f.update(route="wide16", vr=512, tile_bins=64 // parts_of(m) * 4)
        return f
    tb = 64
    while tb > 4 and tb * m * 4 > 48 * 1024:
        tb >>= 1
    quads = ((tb * m + 3) & ~3) // 4
    maxv, ept = (quads + 255) // 256, (m + 256 // tb - 1) // (256 // tb)
    f["tile_bins"] = tb
    f["tmpl"] = 413 if maxv <= 4 and ept <= 13 else 826 if maxv <= 8 and ept <= 26 else 1352 if ept <= 52 else 1300
    return f


def _build(seed, n, mu, runs=(), spikes=(), stretch=None, noise=None):
    rng = np.random.default_rng(seed)
    fasta = ACGT[rng.integers(0, 4, size=n)].copy()
    if noise is None:   # symmetric around mu, spread as a Poisson depth: the median is mu with a margin of 2 % of the bases each side
        depth = np.maximum(int(mu) + np.rint(rng.normal(0.0, np.sqrt(mu), size=n)), 0).astype(np.int32)
    else:       # deep coverage: mu + a symmetric step of at most `noise`, the median is mu itself
        depth = (int(mu) + rng.integers(-noise, noise + 1, size=n)).astype(np.int32)
    if stretch is not None:     # (start, length, lo, hi): values lo .. hi uniformly, for the bins whose median is the cap
        s, ln, lo, hi = stretch
        depth[s:s + ln] = rng.integers(lo, hi + 1, size=ln)
    for pos, val in spikes:
        depth[pos] = val
    for s, ln in runs:
        fasta[s:s + ln] = ord("N")
        depth[s:s + ln] = 0
    return fasta, depth


def _even_runs(k, first, step, length=3):
    return [(first + i * step, length) for i in range(k)]


def _spec(cid, n, m, mu, cap, gc=1, runs=(), capval=None, error=None, exclude=None, cap_exact=True, seed=None, **kw):
    return dict(id=cid, n=n, m=m, mu=mu, cap=cap, gc=gc, runs=list(runs), capval=capval, error=error, exclude=exclude,
                cap_exact=cap_exact and error is None, seed=seed, kw=kw)


def _capflag(target, med):
    return (target + 0.5) / med


M_EDGES = (51, 53, 103, 105, 215, 217, 439)
CAP_CLASSES = (60, 100, 200)            # <= 63, 64 .. 127, 128 .. 253
SEQ_M = (51, 101, 201, 401)             # one m per PARTS class
SEQ_CAPS = (120, 130, 126, 60, 70, 250, 260, 250, 120)   # -cap 2: medians 60, 65, 63, 30, 35, 125, 130, 125, 60


def _specs():
    S = []
    # ---- the cap value across every threshold, GC-adjusted and -NOGC (m = 101) ----
    for gc in (1, 0):
        g = "gc" if gc else "nogc"
        for t in (63, 64, 127, 128, 253, 254):
            sp = [(5000 + 7 * k, t - 2 + k) for k in range(6)] + [(9000 + k, 300) for k in range(40)]
            S.append(_spec(f"cap{t}_{g}", 30_011, 101, 30, _capflag(t, 30), gc, capval=t, spikes=sp))
        S.append(_spec(f"nocap_{g}", 30_011, 101, 30, -1.0, gc, capval=None))
    for t in (32766, 32767):    # K4w's upper end: deep coverage, the raw depth is the value
        S.append(_spec(f"cap{t}_nogc", 30_011, 101, 10922, _capflag(t, 10922), 0, capval=t, noise=2,
                       spikes=[(7000 + k, 40_000) for k in range(200)]))
    S.append(_spec("cap1000_gc_deep", 30_011, 101, 400, _capflag(1000, 400), 1, capval=1000, noise=3, cap_exact=False,
                   spikes=[(7000 + k, 1500) for k in range(200)]))
    # ---- m classes x byte cap classes: every k_bin_median8<SW7, PARTS>; -NOGC: RAW K4s ----
    for gc in (1, 0):
        g = "gc" if gc else "nogc"
        for m in M_EDGES:
            for t in CAP_CLASSES:
                n = 12 * m + 12_000 + (m % 7)
                # a stretch whose bins hold the cap, one below and one above it, most values above: the median is the cap itself
                # (the depth sits just below the cap, a quarter of the values are capped; the cap's class is what these cases are for)
                mu = {60: 57, 100: 95, 200: 190}[t]
                S.append(_spec(f"m{m}_cap{t}_{g}", n, m, mu, _capflag(t, mu), gc, capval=t, cap_exact=False, stretch=(1000, 3 * m, t - 3, t + 12)))
    S.append(_spec("m441_cap100_gc", 12 * 441 + 4040, 441, 30, _capflag(100, 30), 1, capval=100))
    S.append(_spec("m441_cap100_nogc", 12 * 441 + 4040, 441, 30, _capflag(100, 30), 0, capval=100))
    S.append(_spec("m2999_cap100_gc", 30_000, 2999, 30, _capflag(100, 30), 1, capval=100))
    # ---- K4w in each bins-per-tile class; the int32 K4's templates (no cap) ----
    for m in (51, 101, 201, 401):
        S.append(_spec(f"k4w_m{m}", 20 * m + 12_000, m, 30, _capflag(300, 30), 1, capval=300,
                       spikes=[(3000 + 3 * k, 290 + k) for k in range(30)]))
    for m in (51, 53, 103, 105, 191, 193, 441, 2999):
        S.append(_spec(f"int32_m{m}", max(10 * m, 4040) + 4040, m, 30, -1.0, 1, capval=None))
    # ---- removed regions: 0, 48 / 49 (kernel arguments -> device memory), 128 / 129 (LDS mirror -> HBM) ----
    for k in (48, 49, 128, 129):
        for gc in (1, 0):
            S.append(_spec(f"reg{k}_{'gc' if gc else 'nogc'}", 400 * k + 6000, 101, 30, 4.0, gc, runs=_even_runs(k, 3000, 400), capval=120))
    # the same lists through the region staging and the segment walk of K4w (a cap of 300) and of the int32 K4 (no cap); seeds of their
    # own, so that the cases behind them keep theirs
    for j, k in enumerate((49, 129)):
        S.append(_spec(f"reg{k}_k4w", 400 * k + 6000, 101, 30, _capflag(300, 30), 1, runs=_even_runs(k, 3000, 400), capval=300, seed=0x9E2B00 + 2 * j))
        S.append(_spec(f"reg{k}_int32", 400 * k + 6000, 101, 30, -1.0, 1, runs=_even_runs(k, 3000, 400), capval=None, seed=0x9E2B01 + 2 * j))
    S.append(_spec("reg49_exclude", 400 * 49 + 6000, 101, 30, 4.0, 1, capval=120,
                   exclude=[(3000 + 400 * i, 3003 + 400 * i) for i in range(49)]))
    # ---- n' around 8 m (m = 439: 3512) and around one K4s sub-tile of 2048 (m = 51) ----
    for d in (-1, 0, 1):
        S.append(_spec(f"n8m{d:+d}", 4100, 439, 30, 4.0, 1, runs=[(1500, 4100 - (3512 + d) - 2 * pad_of(439))], capval=120,
                       error="RSI_ERR_TOO_SMALL" if d < 0 else None, cap_exact=False))
        S.append(_spec(f"sub2048{d:+d}", 4040, 51, 30, 4.0, 1, runs=[(1000, 4040 - (2048 + d) - 2 * pad_of(51))], capval=120, cap_exact=False))
    # ---- residue classes of n' (no N: n' = n), m = 101 ----
    for cid, n in (("mod31_0", 31 * 1300), ("mod31_30", 31 * 1300 - 1), ("modm_0", 101 * 400), ("modm_m1", 101 * 400 - 1)):
        S.append(_spec(cid, n, 101, 30, 4.0, 1, capval=120))
    # ---- the smallest n, n mod 20 (tail quirks), n mod 4 and mod 64 (streaming tails, last mask word); no N ----
    for n in (4040, 4041, 4059, 4159, 4160):
        for gc in (1, 0):
            S.append(_spec(f"n{n}_{'gc' if gc else 'nogc'}", n, 51, 30, 4.0, gc, capval=120))
    # ---- layout of the N runs: at base 0, up to n - 1, ending on a mask word, a cut on a sub-tile in compacted coordinates ----
    n = 20_037
    S.append(_spec("nrun_at_0", n, 101, 30, 4.0, 1, runs=[(0, 700), (9000, 10)], capval=120))
    S.append(_spec("nrun_to_end", n, 101, 30, 4.0, 1, runs=[(9000, 10), (n - 700, 700)], capval=120))
    S.append(_spec("nrun_both_ends_nogc", n, 101, 30, 4.0, 0, runs=[(0, 64), (n - 64, 64)], capval=120))
    S.append(_spec("nrun_end_word64", n, 101, 30, 4.0, 1, runs=[(5000, 6400 - 5000), (12_000, 12_800 - 50 - 12_000)], capval=120, cap_exact=False))
    S.append(_spec("nrun_cut_2048", n, 101, 30, 4.0, 1, runs=[(3 * 2048 + 50, 333), (5 * 2048 + 50 + 433, 20)], capval=120))
    # ---- 254, 255, 256 (K2j's escape code and its neighbours) next to a cut and on the last base: K4s' exact pass ----
    for t, gc in ((253, 1), (120, 1), (253, 0)):
        cut = [(8000, 100)]
        a, b = 8000 - 50, 8099 + 50
        sp = [(a - 3, 254), (a - 2, 255), (a - 1, 256), (b + 1, 256), (b + 2, 255), (b + 3, 254),
              (n - 3, 254), (n - 2, 256), (n - 1, 255), (0, 255), (1, 254)]
        S.append(_spec(f"escape_edges_cap{t}_{'gc' if gc else 'nogc'}", n, 101, 30, _capflag(t, 30), gc, runs=cut, capval=t, spikes=sp))
    # ---- the queued K4's sequences (test c): caps through the depth at -cap 2, then lengths and regions at one cap ----
    for m in SEQ_M:
        nlong = 24_000 + m
        for gc in (1, 0) if m == 101 else (1,):
            g = "" if gc else "_nogc"
            for med in sorted(set(c // 2 for c in SEQ_CAPS)):
                S.append(_spec(f"seq_m{m}_cap{2 * med}{g}", nlong, m, med, 2.0, gc, capval=2 * med))
            p = pad_of(m)
            S.append(_spec(f"seq_m{m}_short{g}", 4100, m, 60, 2.0, gc, runs=[(200, 4100 - (8 * m - 1) - 2 * p)], capval=120, error="RSI_ERR_TOO_SMALL"))
            step = 2 * p + 203
            S.append(_spec(f"seq_m{m}_reg49{g}", 49 * step + 8 * m + 5000, m, 60, 2.0, gc, runs=_even_runs(49, 2000, step), capval=120, cap_exact=False))
            S.append(_spec(f"seq_m{m}_reg129{g}", 129 * step + 8 * m + 5000, m, 60, 2.0, gc, runs=_even_runs(129, 2000, step), capval=120, cap_exact=False))
    k = 0       # a case without a seed of its own: numbered among those, in list order
    for sp in S:
        if sp["seed"] is None:
            sp["seed"], k = 0x9E1B00 + k, k + 1
    return S


def _case(sp):
    fasta, depth = _build(sp["seed"], sp["n"], sp["mu"], sp["runs"], **{"spikes": sp["kw"].get("spikes", ()), "stretch": sp["kw"].get("stretch"),
                                                                        "noise": sp["kw"].get("noise")})
    flags = dict(m=sp["m"], cap=sp["cap"], gcadjust=sp["gc"])
    runs = sp["runs"] if sp["exclude"] is None else [(s, e - s) for s, e in sp["exclude"]]
    regs = merged_regions(sp["n"], runs, sp["m"])
    ncompact = sp["n"] - sum(b - a + 1 for a, b in regs)
    expect = dict(capval=sp["capval"], cap_exact=sp["cap_exact"], ncompact=ncompact, nreg=len(regs), error=sp["error"])
    expect.update(form_for(sp["capval"], sp["m"], ncompact, len(regs), bool(sp["gc"])))
    return (sp["id"], fasta, depth, flags, sp["exclude"], expect)


_CACHE = {}


def case_ids():
    if "specs" not in _CACHE:
        _CACHE["specs"] = _specs()
        assert len({s["id"] for s in _CACHE["specs"]}) == len(_CACHE["specs"])
    return [s["id"] for s in _CACHE["specs"]]


def get_case(cid):
    """The case of that id (built once per process; the arrays are shared: leave them unchanged)."""
    ids = case_ids()
    if cid not in _CACHE:
        _CACHE[cid] = _case(_CACHE["specs"][ids.index(cid)])
    return _CACHE[cid]


def gc_wide_case():
    """(fasta, depth, flags) for the rung of the per-base phase's redo ladder that no case above takes: the smallest GC-adjusted
    chromosome (n4040_gc) with one depth of exactly 2^21, where the packed accumulators of the three-pass chain's K2 overflow and the
    chain is issued again in its two-atomic form (RSI_HOT_JOINT=0: "a2-3.gc wide redo", gc_hist_wide), and one of 2^21 - 1 next to
    the threshold.  Not one of the golden cases: it is compared with the oracle's per-base stages."""
    _, fasta, depth, flags, _, _ = get_case("n4040_gc")
    depth = depth.copy()
    depth[1000], depth[3000] = 1 << 21, (1 << 21) - 1
    return fasta, depth, flags


def checker_inputs(case):
    """What the CPU checkers (oracle, reference) read for the case: excluded bases painted 'N' (they know no mask)."""
    _, fasta, depth, _, exclude, _ = case
    if exclude is None:
        return fasta, depth
    f = fasta.copy()
    for s, e in exclude:
        f[s:e] = ord("N")
    return f, depth


def standalone_ids():
    return [c for c in case_ids() if not c.startswith("seq_")]


def run_order():
    """The order test (a) runs the cases in on one context: sorted by length, then taken alternately from the short and the long end,
    so that buffers grow and shrink in use and consecutive cases differ in shape."""
    ids = sorted(standalone_ids(), key=lambda c: (get_case(c)[1].size, c))
    out = []
    while ids:
        out.append(ids.pop(0))
        if ids:
            out.append(ids.pop())
    return out


def load_golden():
    """golden/per_base_edges.npz as {id: dict}: flags, the sha256 strings, n_compact, nbins, noncode, binmedint (None above 4096
    bins: binmedint_sha only), chrom = [RDmedian, RDsd, cap median, mean of the positive depths]."""
    import json
    import os
    if "golden" not in _CACHE:
        z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "per_base_edges.npz"), allow_pickle=False)
        meta, ids = json.loads(str(z["meta"])), json.loads(str(z["ids"]))
        no, bo = z["noncode_off"], z["binmedint_off"]
        for k, cid in enumerate(ids):
            g = meta[cid]
            g["chrom"] = z["chrom"][k]
            g["noncode"] = z["noncode"][no[k]:no[k + 1]]
            g["binmedint"] = z["binmedint"][bo[k]:bo[k + 1]] if bo[k + 1] - bo[k] == g["nbins"] else None
        _CACHE["golden"] = meta
    return _CACHE["golden"]
