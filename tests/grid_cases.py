"""Inputs of the 0.01-grid quantile tests (tests/test_grid_quantiles.py on the device, tests/test_grid_restatement.py against the
oracle).  Every builder returns GridCase objects; the modes are those of RsiHot.debug_grid_median: "pair" (device chain,
median then MAD), "mad" (device chain, MAD around `center`), "host" (host-driven form), "med" (-MED: int32 input, MAD
around `center`)."""
import numpy as np

import grid_restatement as gr

F32 = np.float32
KTHREADS, KHISTRUN, KLDSBINS = 256, 8, 12288   # kernels_bin.hip: workgroup size, values per run, LDS buckets of the histogram


class GridCase:
    def __init__(self, name, x=None, mask=None, modes=("pair", "host"), center=0.0, xi=None):
        self.name, self.mask, self.modes, self.center = name, mask, tuple(modes), float(center)
        self.x = None if x is None else np.ascontiguousarray(x, dtype=np.float32)
        self.xi = None if xi is None else np.ascontiguousarray(xi, dtype=np.int32)
        if self.mask is not None:
            self.mask = np.ascontiguousarray(self.mask, dtype=np.int32)

    def __repr__(self):
        return f"GridCase({self.name})"

    def oracle_arrays(self):
        """The float32 arrays whose partition_stat_tp median a mode takes: the selection, and the deviations of each MAD."""
        out = []
        if self.xi is not None:
            return [gr.abs_dev(self.xi.astype(np.float32), self.center)]
        s = gr.selected(self.x, self.mask)
        if s.size == 0 or not np.all(np.isfinite(s)):
            return out
        out.append(s)
        if "pair" in self.modes or "host" in self.modes:
            out.append(gr.abs_dev(s, gr.median(s)[0]))
        if "mad" in self.modes:
            out.append(gr.abs_dev(s, self.center))
        return out


def at_bucket(ymin, b):
    """A float32 value in bucket b of a grid anchored at the float32 ymin."""
    v = F32(float(F32(ymin)) + b * gr.DY)
    assert int(gr.buckets([v], float(F32(ymin)))[0]) == b
    return v


def from_buckets(ymin, counts, seed):
    """Values placed bucket by bucket (counts: {bucket: how many}), shuffled."""
    vals = np.concatenate([np.full(c, at_bucket(ymin, b), dtype=np.float32) for b, c in sorted(counts.items()) if c])
    np.random.default_rng(seed).shuffle(vals)
    return vals


# ---- bucket half-points and grid points --------------------------------------------------------------------------------
def half_points():
    cases = []
    for ymin in (0.0, 1.0, 37.21, -5.5, 1234.5):
        y = F32(ymin)
        for k in (0, 1, 2, 7, 99, 100, 101, 517, 1000, 4095, 12287, 12288, 54321):
            half = F32(float(y) + (k + 0.5) * gr.DY)
            grid = F32(float(y) + k * gr.DY)
            for tag, v in (("half", half), ("grid", grid)):
                for side, w in (("-", np.nextafter(v, F32(-np.inf))), ("=", v), ("+", np.nextafter(v, F32(np.inf)))):
                    if w < y:
                        continue
                    top = F32(float(w) + 3 * gr.DY)
                    m = 3   # n = 7, n // 2 = 3: two copies of ymin, then w: the count reaches 3 in w's bucket
                    x = np.array([y] * (m - 1) + [w] + [top] * (m + 1), dtype=np.float32)
                    cases.append(GridCase(f"{tag}{side}_y{ymin}_k{k}", np.random.default_rng(k).permutation(x)))
    # one long array of nothing but half-points and their neighbours: every bucket edge at once
    rng = np.random.default_rng(0x4A1F)
    k = rng.integers(0, 20000, 150_001)
    v = (F32(2.0) + (k + 0.5) * gr.DY).astype(np.float32)
    v = np.where(rng.random(v.size) < 1 / 3, np.nextafter(v, F32(-np.inf)), np.where(rng.random(v.size) < 0.5, v, np.nextafter(v, F32(np.inf))))
    cases.append(GridCase("half_points_long", np.concatenate([[F32(2.0)], v]).astype(np.float32)))
    return cases


# ---- tiny and plain large inputs ---------------------------------------------------------------------------------------
def tiny():
    rng = np.random.default_rng(0x71)
    c = [GridCase("n1", [3.7]), GridCase("n1_neg", [-12.25]), GridCase("n2", [3.7, 5.2]), GridCase("n2_rev", [5.2, 3.7]),
         GridCase("n2_close", [3.7, 3.705]), GridCase("n2_grid_step", [3.0, 3.01]), GridCase("n3", [5.0, 3.7, 9.1]),
         GridCase("n3_close", [5.0, 5.004, 5.001]), GridCase("n4", [9.1, 3.7, 5.0, 4.2]), GridCase("n4_pairs", [1.0, 1.0, 2.0, 2.0])]
    c.append(GridCase("large_odd", rng.normal(30.0, 6.0, 200_001)))
    c.append(GridCase("large_even", rng.normal(30.0, 6.0, 200_000)))
    for n in (5, 6, 7, 8, 9, 15, 16, 17, 255, 256, 257, 2047, 2048, 2049):   # partial runs of eight, partial workgroups
        c.append(GridCase(f"n{n}", rng.normal(10.0, 2.0, n)))
    return c


# ---- where the running count crosses n // 2 ----------------------------------------------------------------------------
def walk_chunk(npb):
    """grid_walk_block's stretch of buckets per thread: ceil(np / 256) rounded up to whole quads, and the sub-stretch per
    thread when the crossing stretch is read again."""
    chunk = ((npb + KTHREADS - 1) // KTHREADS + 3) & ~3
    return chunk, (chunk + KTHREADS - 1) // KTHREADS


def crossing_case(name, ymin, top, b, seed, exact_end=False, n=2001):
    """n values over the buckets 0 .. top (both occupied), the count reaching n // 2 in bucket b -- with the bucket's last
    value when exact_end."""
    rng = np.random.default_rng(seed)
    k = n // 2
    if b == 0:
        below, at = 0, (k if exact_end else k + 3)
    elif b == top:
        below, at = k - 1, n - (k - 1)
    else:
        below = k - 2 if exact_end else k - 1
        at = 2 if exact_end else int(rng.integers(1, 6))
    above = n - below - at
    counts = {b: at}
    for lo, hi, cnt, must in ((0, b - 1, below, 0), (b + 1, top, above, top)):
        if cnt:
            for p in [must] + list(rng.integers(lo, hi + 1, cnt - 1)):
                counts[int(p)] = counts.get(int(p), 0) + 1
    x = from_buckets(ymin, counts, seed)
    cum = np.cumsum(np.bincount(gr.buckets(x, float(F32(ymin))).astype(np.int64)))
    assert gr.median_bucket(x) == b and (not exact_end or cum[b] == k), name
    return GridCase(name, x)


def crossings():
    c = [GridCase("exact_end_first", from_buckets(3.0, {0: 5, 7: 5}, 1)),          # 10 values, n // 2 = 5 reached by bucket 0 alone
         GridCase("exact_end_mid", from_buckets(3.0, {0: 2, 5: 3, 50: 5}, 2)),
         GridCase("exact_end_mid_odd", from_buckets(3.0, {0: 2, 5: 3, 50: 6}, 3)),
         GridCase("first_bucket", from_buckets(-2.0, {0: 9, 3: 4, 400: 4}, 4)),
         GridCase("last_bucket", from_buckets(1.0, {0: 1, 800: 9}, 5))]
    # np - 1 itself occupied: (ymax - ymin) / 0.01 with a fractional part of at least one half
    y = F32(0.0)
    top = F32(8.007)
    assert int(gr.buckets([top], 0.0)[0]) == gr.span([y, top])[2] - 1
    c.append(GridCase("last_bucket_np_minus_1", np.array([y] + [top] * 9, dtype=np.float32)))
    # the crossing on the first and the last bucket of a thread's stretch in grid_walk_block, and of a sub-stretch
    seed = 100
    for top_b in (7, 258, 1028, 4998, 12288, 299_998, (1 << 20) - 2):
        npb = gr.span([at_bucket(5.0, 0), at_bucket(5.0, top_b)])[2]
        chunk, per = walk_chunk(npb)
        picks = {0, 1, chunk - 1, chunk, 2 * chunk - 1, 5 * chunk, 5 * chunk + per - 1, 5 * chunk + per, 7 * chunk + 3 * per - 1,
                 (top_b // chunk) * chunk, (top_b // chunk) * chunk - 1, top_b - 1, top_b}
        for b in sorted(p for p in picks if 0 <= p <= top_b):
            for exact in ((False, True) if b < top_b else (False,)):
                seed += 1
                c.append(crossing_case(f"cross_np{npb}_b{b}{'_exact' if exact else ''}", 5.0, top_b, b, seed, exact_end=exact))
    return c


# ---- signs ------------------------------------------------------------------------------------------------------------
def signs():
    rng = np.random.default_rng(0x5160)
    tiny_sub = np.nextafter(F32(0.0), F32(1.0))
    return [GridCase("negative", rng.normal(-50.0, 10.0, 50_001)),
            GridCase("across_zero", rng.normal(0.0, 3.0, 40_000)),
            GridCase("negative_ints", -rng.poisson(20.0, 30_001).astype(np.float32)),
            GridCase("zeros_mixed", rng.permutation(np.array([-0.0, 0.0] * 50 + [0.5] * 30 + [1.0] * 21, dtype=np.float32))),
            GridCase("zeros_first_neg", np.array([-0.0, 0.0, 0.0, 2.0, 3.0], dtype=np.float32)),
            GridCase("zeros_first_pos", np.array([0.0, -0.0, -0.0, 2.0, 3.0], dtype=np.float32)),
            GridCase("zeros_only", np.array([-0.0, 0.0, -0.0, 0.0, 0.0, -0.0], dtype=np.float32)),
            GridCase("subnormal_min", np.array([-tiny_sub, 0.003, 0.004, 0.5, 0.6], dtype=np.float32)),
            GridCase("subnormals", np.array([tiny_sub * 3, -tiny_sub, 0.0, 0.02, 0.03, 1e-38, 0.01], dtype=np.float32))]


# ---- below the grid step: the mean in index order ----------------------------------------------------------------------
def degenerate():
    rng = np.random.default_rng(0xDE6)
    # values of like magnitude add up exactly in double whatever the order: these span thirty decades
    x = ((rng.random(300_001) - 0.5) * 0.009 * 10.0 ** -rng.integers(0, 30, 300_001)).astype(np.float32)
    d = x.astype(np.float64)
    assert gr.index_order_mean(x) != float(np.sum(d)) / d.size and gr.index_order_mean(x) != float(np.sum(d[::-1])) / d.size
    y = (F32(-7.125) + rng.random(65_537) * 0.0099).astype(np.float32)
    flat = (F32(1000.0) + rng.random(300_001) * 0.009).astype(np.float32)
    return [GridCase("degenerate_order", x, modes=("pair", "host", "mad"), center=0.001),
            GridCase("degenerate_flat", flat, modes=("pair", "host", "mad"), center=1000.004),
            GridCase("degenerate_neg", y, modes=("pair", "host", "mad"), center=-3.0),
            GridCase("degenerate_two", [5.0, 5.005]),
            GridCase("constant", np.full(1000, 7.25, dtype=np.float32)),
            GridCase("degenerate_masked", np.concatenate([flat[:5000], [50.0, -50.0]]).astype(np.float32),
                     mask=np.concatenate([np.zeros(5000, np.int32), [1, 1]]).astype(np.int32))]


# ---- ranges at the chain's bucket limit --------------------------------------------------------------------------------
def wide_edges():
    """The largest float32 ymax (ymin = 0) whose grid has CAP buckets, and the next float32, whose grid has CAP + 1."""
    v = F32(10485.74)
    while int(float(np.nextafter(v, F32(np.inf))) / gr.DY + 2) <= gr.CAP:
        v = np.nextafter(v, F32(np.inf))
    while int(float(v) / gr.DY + 2) > gr.CAP:
        v = np.nextafter(v, F32(-np.inf))
    nxt = np.nextafter(v, F32(np.inf))
    assert int(float(v) / gr.DY + 2) == gr.CAP and int(float(nxt) / gr.DY + 2) == gr.CAP + 1
    return v, nxt


def too_wide():
    rng = np.random.default_rng(0x31DE)
    below, above = wide_edges()
    c = []
    for tag, top in (("below", below), ("above", above)):
        body = (rng.random(4001) * float(top)).astype(np.float32)
        x = np.concatenate([[F32(0.0), top], body]).astype(np.float32)
        c.append(GridCase(f"cap_{tag}", rng.permutation(x), modes=("pair", "host", "mad"), center=-1.0))
        x2 = np.concatenate([[F32(0.0), top], rng.normal(30.0, 4.0, 4001).astype(np.float32)]).astype(np.float32)   # median near the bottom
        c.append(GridCase(f"cap_{tag}_low_median", rng.permutation(x2), modes=("pair", "host", "mad"), center=5000.0))
    c.append(GridCase("far_beyond_cap", np.concatenate([[F32(-20000.0)], rng.normal(30.0, 4.0, 3000), [F32(60000.0)]]).astype(np.float32),
                      modes=("pair", "host", "mad"), center=30.0))
    return c


# ---- the two LDS counter widths ----------------------------------------------------------------------------------------
PACK16_LAST = 16_254_975     # the busiest workgroup of launch_hist_walk counts 65 535 values
PACK16_OLD_LAST = 16_774_912  # what the former bound, nb / grid + kHistRun < 65536, still gave 16-bit counters


def one_bucket(nb, seed):
    """All values in one bucket but a few, the few outside the first workgroup's share."""
    x = np.full(nb, F32(3.0), dtype=np.float32)
    x[2048:2053] = np.array([3.5, 2.0, 4.25, 3.0, 9.0], dtype=np.float32)
    xi = np.full(nb, 30, dtype=np.int32)
    xi[2048:2052] = np.array([31, 29, 35, 40], dtype=np.int32)
    return x, xi


def counter_widths():
    c = []
    for nb, pack16 in ((PACK16_LAST, 1), (PACK16_LAST + 1, 0), (PACK16_OLD_LAST, 0), (PACK16_OLD_LAST + 1, 0)):
        x, xi = one_bucket(nb, nb)
        case = GridCase(f"nb{nb}", x, modes=("pair", "host"))
        case.pack16 = pack16
        c.append(case)
        mc = GridCase(f"nb{nb}_med", xi=xi, modes=("med",), center=30.0)
        mc.pack16 = pack16
        c.append(mc)
    return c


# ---- the LDS window of a long grid -------------------------------------------------------------------------------------
def sample_positions(nb):
    """hist_body's 64 sample positions: the middle of each 64th of the array."""
    return np.array([((2 * lane + 1) * nb) >> 7 for lane in range(64)], dtype=np.int64)


def lds_window():
    rng = np.random.default_rng(0x1D5)
    c = []
    nb = 100_000
    x = rng.normal(35.0, 8.0, nb).clip(10.0, 60.0).astype(np.float32)
    x[0] = 10.0
    far = x.copy()
    far[sample_positions(nb)] = 500.0               # the window lands on [np - 12288, np): the bulk all through global atomics
    c.append(GridCase("window_far", far, modes=("pair", "host", "mad"), center=35.0))
    u = (rng.random(nb) * 200.0).astype(np.float32)
    u[0], u[1] = 0.0, 200.0
    split = u.copy()
    split[sample_positions(nb)] = 150.0              # the window covers buckets 7714 .. 20001 of 20002: part of the bulk
    c.append(GridCase("window_split", split, modes=("pair", "host", "mad"), center=20.0))
    low = u.copy()
    low[sample_positions(nb)] = 0.5                  # the window at the bottom, the median above it
    c.append(GridCase("window_low", low))
    half = np.zeros(nb, np.int32)
    half[sample_positions(nb)[::2]] = 1              # half the samples masked: the window still placed by the other half
    c.append(GridCase("window_half_samples_masked", far, mask=half, modes=("pair", "host", "mad"), center=35.0))
    lone = far.copy()
    lone[7] = 400.0
    every = np.zeros(nb, np.int32)
    every[sample_positions(nb)] = 1                  # no valid sample: the window stays at bucket 0, the outlier's bucket global
    c.append(GridCase("window_no_valid_sample", lone, mask=every, modes=("pair", "host", "mad"), center=35.0))
    big = rng.normal(3000.0, 900.0, 600_001).clip(0.0, 9000.0).astype(np.float32)   # 900 001 buckets: far more than the window
    c.append(GridCase("window_wide_grid", big, modes=("pair", "host", "mad"), center=1000.0))
    return c


# ---- masks and centres -------------------------------------------------------------------------------------------------
def masks_centres():
    rng = np.random.default_rng(0x3A5C)
    c = []
    x = rng.normal(40.0, 9.0, 120_003).astype(np.float32)
    for dens in (0.01, 0.3, 0.97):
        m = (rng.random(x.size) < dens).astype(np.int32) * int(rng.integers(1, 5))
        c.append(GridCase(f"mask_{dens}", x, mask=m, modes=("pair", "host", "mad"), center=37.5))
    m = np.ones(x.size, np.int32)
    m[[5, 77_777]] = 0
    c.append(GridCase("mask_two_left", x, mask=m, modes=("pair", "host", "mad"), center=0.0))
    m = np.ones(x.size, np.int32)
    m[1234] = 0
    c.append(GridCase("mask_one_left", x, mask=m, modes=("pair", "host", "mad"), center=41.0))
    y = x.copy()
    y[[10, 500, 9000]] = [np.nan, np.inf, -np.inf]
    m = np.zeros(x.size, np.int32)
    m[[10, 500, 9000]] = 1
    c.append(GridCase("mask_hides_nonfinite", y, mask=m, modes=("pair", "host", "mad"), center=40.0))
    z = x.copy()
    z[[3, 4]] = [-1e6, 1e6]
    m = np.zeros(x.size, np.int32)
    m[[3, 4]] = -1
    c.append(GridCase("mask_hides_wide", z, mask=m, modes=("pair", "host", "mad"), center=40.0))
    return c


# ---- seeded random arrays ----------------------------------------------------------------------------------------------
def random_arrays(count=200):
    c = []
    for i in range(count):
        rng = np.random.default_rng(0xA77A + i)
        n = int(np.exp(rng.uniform(0.0, np.log(300_000))))
        kind = ("normal", "integer", "bimodal", "heavy")[i % 4]
        if kind == "normal":
            x = rng.normal(rng.uniform(-20, 80), rng.uniform(0.01, 15), n)
        elif kind == "integer":
            x = rng.poisson(rng.uniform(0.5, 80), n).astype(np.float64)
        elif kind == "bimodal":
            x = np.where(rng.random(n) < rng.uniform(0.2, 0.8), rng.normal(20, 3, n), rng.normal(rng.uniform(25, 60), 5, n))
        else:
            x = np.minimum(rng.lognormal(2.5, rng.uniform(0.5, 2.4), n), 30_000.0) * rng.choice([-1.0, 1.0])   # often too wide
        x = x.astype(np.float32)
        mask = None
        if i % 5 == 3:
            mask = (rng.random(n) < 0.3).astype(np.int32)
        modes = ("pair", "host", "mad")
        c.append(GridCase(f"rand{i}_{kind}_n{n}", x, mask=mask, modes=modes, center=float(np.round(np.median(x)))))
        if kind == "integer":
            xi = x.astype(np.int32)
            c.append(GridCase(f"rand{i}_med_n{n}", xi=xi, modes=("med",), center=float(int(np.median(xi)))))
    return c


def finite_groups():
    """Every group of finite, non-empty cases: what the restatement is pinned to the oracle on."""
    return {"half_points": half_points, "tiny": tiny, "crossings": crossings, "signs": signs, "degenerate": degenerate,
            "too_wide": too_wide, "counter_widths": counter_widths, "lds_window": lds_window, "masks_centres": masks_centres,
            "random_arrays": random_arrays}
