"""GPU: the 0.01-grid quantile chain (K6, partition_stat_tp) on its own, in each form the scan's thresholds take, held with == to
the NumPy restatement (tests/grid_restatement.py, pinned to the oracle by tests/test_grid_restatement.py).

Through rsi_hot_debug_grid_median / _mad_i32 every case runs the production functions on a host array and reports which form
ran: the device chain (min/max + plan, histogram + walk) with 16- or 32-bit LDS counters, the host-driven form, and the
chain's flags (empty, non-finite, degenerate, too wide).  Each test asserts the forms it is about, besides the values."""
import numpy as np
import pytest

import grid_cases
import grid_restatement as gr

pytestmark = pytest.mark.gpu

EMPTY, NONFINITE, DEGENERATE, TOOWIDE = 1, 2, 4, 8   # kernels.h: kGrid*
NONFINITE_MSG = "non-finite value in the transformed bins"   # RSI_ERR_UNSUPPORTED (-5)


@pytest.fixture(scope="module")
def hot():
    from rsicnv_amd import api
    h = api.RsiHot(0)
    yield h
    h.close()


def record(s):
    """(flags, buckets) the chain's plan gives the selected float32 values s."""
    if s.size == 0:
        return EMPTY, 0
    if not np.all(np.isfinite(s)):
        return NONFINITE, 0
    npb = gr.span(s)[2]
    if npb is None:
        return DEGENERATE, 0
    if npb > gr.CAP:
        return TOOWIDE, 0
    return 0, npb


def expected(case, mode):
    """(out, info) the hook must return for this case and mode."""
    if mode == "med":
        dev = gr.abs_dev(case.xi.astype(np.float32), case.center)
        out = gr.med_mad_i32(case.xi, case.center)
        f1, n1 = record(dev)
        host = 1 if f1 == TOOWIDE else 0
        return out, [-1, 0, f1, n1, int(case.xi.size <= grid_cases.PACK16_LAST), host, 0, 0]
    s = gr.selected(case.x, case.mask)
    if not hasattr(case, "pair"):
        case.pair = gr.pair(case.x, case.mask) if np.all(np.isfinite(s)) else None   # (the modes share it)
    if mode == "host":
        return case.pair, [-1, 0, -1, 0, -1, 2, 0, 0]
    pack16 = int(case.x.size <= grid_cases.PACK16_LAST)
    if mode == "mad":
        f1, n1 = record(gr.abs_dev(s, case.center))
        return gr.mad(case.x, case.center, case.mask), [-1, 0, f1, n1, pack16, 1 if f1 == TOOWIDE else 0, 0, 0]
    out = case.pair
    f0, n0 = record(s)
    # the MAD chain reads its centre from the median record, which holds 0 when the plan flagged it
    f1, n1 = record(gr.abs_dev(s, out[0] if f0 == 0 else 0.0)) if f0 != EMPTY else (EMPTY, 0)
    host = 2 if TOOWIDE in (f0, f1) else 1 if f0 == DEGENERATE else 0
    return out, [f0, n0, f1, n1, pack16, host, 0, 0]


def run(hot, case, mode):
    if mode == "med":
        return hot.debug_grid_median(case.xi, mode="med", center=case.center)
    return hot.debug_grid_median(case.x, case.mask, mode=mode, center=case.center)


def check(hot, case, mode):
    out, info = run(hot, case, mode)
    exp_out, exp_info = expected(case, mode)
    for i, what in enumerate(("median", "count", "MAD", "count")):
        assert out[i] == exp_out[i], f"{case.name} [{mode}] {what}: device {out[i]!r} != restatement {exp_out[i]!r}"
    info = [int(v) for v in info]
    assert info == exp_info, f"{case.name} [{mode}] info {info} != {exp_info}"
    return out, info


def check_all(hot, cases):
    infos = []
    for case in cases:
        for mode in case.modes:
            infos.append((case, mode) + check(hot, case, mode))
    return infos


def test_half_points(hot):
    """Values at ymin + (k + 1/2) * 0.01 and on grid points, each also one float ulp either side."""
    check_all(hot, grid_cases.half_points())


def test_tiny_inputs(hot):
    """n = 1 .. 4, partial runs of eight and partial workgroups, and a large odd and even n."""
    infos = check_all(hot, grid_cases.tiny())
    assert any(i[3][0] == DEGENERATE for i in infos) and any(i[3][0] == 0 for i in infos)


def test_crossing(hot):
    """n // 2 reached exactly at the end of a bucket, in the first and the last bucket, and on the first and last bucket of a
    thread's stretch (and sub-stretch) in grid_walk_block, for grids from 9 to 2^20 buckets."""
    infos = check_all(hot, grid_cases.crossings())
    assert max(i[3][1] for i in infos if i[1] == "pair") >= (1 << 20) - 1


def test_signs(hot):
    """Negative values, -0.0 beside +0.0 (their order keys differ), subnormals."""
    check_all(hot, grid_cases.signs())


def test_degenerate(hot):
    """A range under 0.01: the mean in index order, on a sum whose order shows; the MAD then around that mean."""
    infos = check_all(hot, grid_cases.degenerate())
    pair = [i for i in infos if i[1] == "pair"]
    assert pair and all(i[3][0] == DEGENERATE for i in pair)
    assert all(i[3][5] == 1 for i in pair)   # the MAD again around the mean, host-driven


def test_empty_selection(hot):
    x = np.random.default_rng(1).normal(30.0, 5.0, 10_007).astype(np.float32)
    for mode in ("pair", "mad", "host"):
        case = grid_cases.GridCase("all_masked", x, mask=np.ones(x.size, np.int32), center=30.0)
        out, info = check(hot, case, mode)
        assert list(out) == [0.0, 0.0, 0.0, 0.0] or (mode == "mad" and list(out) == [30.0, 0.0, 0.0, 0.0])
        if mode != "host":
            assert info[2] == EMPTY and info[0] in (EMPTY, -1)
        check_all(hot, [grid_cases.GridCase("after_empty", x, modes=("pair", "mad", "host"), center=31.0)])


def _after_error(hot, rng):
    """A normal array on the same context, the device chains first (a stale min/max record would show there)."""
    x = rng.normal(25.0, 4.0, 30_011).astype(np.float32)
    check_all(hot, [grid_cases.GridCase("after_error", x, modes=("pair", "mad", "host"), center=24.0),
                    grid_cases.GridCase("after_error_med", xi=np.round(x).astype(np.int32), modes=("med",), center=25.0)])


def test_non_finite(hot):
    """inf, -inf and NaN in the selection fail with the pipeline's message, in every form; the context stays usable."""
    from rsicnv_amd import api
    rng = np.random.default_rng(0xBAD)
    base = rng.normal(30.0, 5.0, 50_001).astype(np.float32)
    for bad in (np.inf, -np.inf, np.nan, (np.nan, np.inf)):
        for where in ((0,), (50_000,), (4097,), (17, 40_000)):
            x = base.copy()
            vals = bad if isinstance(bad, tuple) else (bad,) * len(where)
            for w, v in zip(where, vals * len(where)):
                x[w] = v
            for mode in ("pair", "mad", "host"):
                with pytest.raises(api.RsiError) as e:
                    hot.debug_grid_median(x, mode=mode, center=30.0)
                assert e.value.code == -5 and NONFINITE_MSG in str(e.value), (bad, where, mode)
                _after_error(hot, rng)
    # a masked non-finite value is no error (tests/grid_cases.py: mask_hides_nonfinite)
    small = base[:300].copy()
    small[7] = np.nan
    with pytest.raises(api.RsiError):
        hot.debug_grid_median(small, mode="pair")
    m = np.zeros(small.size, np.int32)
    m[7] = 1
    check(hot, grid_cases.GridCase("nan_masked", small, mask=m), "pair")


def test_too_wide(hot):
    """Ranges at the chain's limit: 2^20 buckets run on the device, 2^20 + 1 take the host-driven form."""
    infos = {(i[0].name, i[1]): i[3] for i in check_all(hot, grid_cases.too_wide())}
    assert infos[("cap_below", "pair")][:2] == [0, gr.CAP] and infos[("cap_below", "pair")][5] == 0
    assert infos[("cap_above", "pair")][0] == TOOWIDE and infos[("cap_above", "pair")][5] == 2
    assert infos[("cap_below_low_median", "pair")][:2] == [0, gr.CAP]
    assert infos[("cap_above_low_median", "pair")][0] == TOOWIDE
    assert infos[("far_beyond_cap", "pair")][0] == TOOWIDE and infos[("far_beyond_cap", "mad")][2] == TOOWIDE


def test_counter_widths(hot):
    """The last nb whose busiest histogram workgroup counts 65 535 values (16-bit LDS counters) and the first past it, and the
    former bound's last 16-bit size, each with nearly every value in one bucket: a wrapped counter loses 65 536 of them."""
    infos = check_all(hot, grid_cases.counter_widths())
    chain = [(c, m, info) for c, m, _, info in infos if m != "host"]
    for c, m, info in chain:
        assert info[4] == c.pack16, (c.name, m, list(info))
    assert {info[4] for _, _, info in chain} == {0, 1}


def test_lds_window(hot):
    """Grids longer than the LDS window, its 64 samples placing it away from the bulk, across part of it, at the bottom, with
    half or all of the samples masked."""
    infos = check_all(hot, grid_cases.lds_window())
    assert all(i[3][1] > grid_cases.KLDSBINS for i in infos if i[1] == "pair")


def test_masks_and_centres(hot):
    check_all(hot, grid_cases.masks_centres())
    # the MAD centred through device memory (the pair) equals the MAD around the same centre given by the caller
    rng = np.random.default_rng(0xCE)
    for n in (3, 1000, 77_777, 250_000):
        x = rng.normal(50.0, 12.0, n).astype(np.float32)
        m = (rng.random(n) < 0.2).astype(np.int32)
        for mask in (None, m):
            pair, _ = hot.debug_grid_median(x, mask, mode="pair")
            mad, _ = hot.debug_grid_median(x, mask, mode="mad", center=pair[0])
            assert (pair[2], pair[3]) == (mad[2], mad[3]) and mad[0] == pair[0]


def test_random_arrays(hot):
    """200 seeded arrays, 1 to 300 000 values: normal, integer-valued (also as -MED bin medians), bimodal, heavy-tailed."""
    infos = check_all(hot, grid_cases.random_arrays())
    modes = {i[1] for i in infos}
    assert modes == {"pair", "mad", "host", "med"}
    assert any(i[3][0] == TOOWIDE for i in infos if i[1] == "pair")


def test_context_state(hot):
    """Modes alternated on one fresh context: a min/max record, an arrival counter or a bucket array left behind by one call
    (or regrown by the host-driven form) would show in the next."""
    from rsicnv_amd import api
    rng = np.random.default_rng(0x57A7E)
    wide = grid_cases.too_wide()
    window = grid_cases.lds_window()
    deg = grid_cases.degenerate()
    tiny = grid_cases.tiny()
    ints = rng.poisson(30.0, 40_000).astype(np.int32)
    seq = [(grid_cases.GridCase("small", rng.normal(10.0, 1.0, 5000)), "pair"),
           (wide[-1], "host"),                        # 8 M buckets: the host-driven form grows the bucket array
           (window[-1], "pair"),
           (tiny[2], "mad"),
           ("nan", "pair"),
           (grid_cases.GridCase("ints_med", xi=ints, center=30.0), "med"),
           (deg[0], "pair"),
           (wide[2], "pair"),                         # too wide: the chain, then the host-driven form
           (grid_cases.GridCase("masked_out", rng.normal(5.0, 1.0, 999), mask=np.ones(999, np.int32)), "pair"),
           (window[0], "mad"),
           ("inf", "mad"),
           (grid_cases.GridCase("ints_f", ints.astype(np.float32), center=29.0), "pair"),
           (tiny[0], "pair"),
           (wide[1], "pair"),
           (grid_cases.half_points()[-1], "pair")]
    h = api.RsiHot(0)
    try:
        for rep in range(2):
            for case, mode in (seq if rep == 0 else seq[::-1]):
                if isinstance(case, str):
                    x = rng.normal(10.0, 1.0, 4096).astype(np.float32)
                    x[123] = np.nan if case == "nan" else np.inf
                    with pytest.raises(api.RsiError):
                        h.debug_grid_median(x, mode=mode, center=10.0)
                    continue
                check(h, case, mode)
    finally:
        h.close()
