"""Seeded cases of the plot data and a plain numpy restatement of what plot_icnv (plotcnv.cpp:245-610) puts into a
call's .dat and .gp file: the planner (geometry, band, one query per printed row), the window sums of the running mean, the
quantiles, and both files' text.  Arrays come from seeds and are never stored.  Shared by tests/test_plot_host.py (restatement =
golden = the host writer), tests/test_plot_device.py (device = host writer = golden) and tools/make_golden_plot_edges.py."""
import collections
import math

import numpy as np

M, MINMLEN, CHKLEN = 101, 3.01, 2.5          # the run's defaults: a neighbourhood of 2.5 x max(length, 304) on either side
TILE = 256                                   # values per window-sum tile the device tests run with
POINTS = 30000                               # plot::pts
TYPES = ("DEL", "DUP", "UNKNOWN")
REFUSALS = {0: "ok", 1: "beyond", 2: "size error", 3: "empty body", 4: "no band"}

# calls: (start, end, type) as in the output rows.  golden: the compiled reference's own bytes exist for the case's plannable calls
# (its _median allocates a counter per unit of the array's span: only arrays whose span is below 10^6 qualify).
Case = collections.namedtuple("Case", "name n build calls golden")


def _poisson(seed, n, mean=30):
    return np.random.default_rng(seed).poisson(mean, size=n).astype(np.int32)


def _few(seed, n):
    """Few distinct values in long runs: a wide walk whose text compresses well."""
    rng = np.random.default_rng(seed)
    return np.repeat(rng.integers(20, 40, size=n // 50 + 1), 50)[:n].astype(np.int32)


def _spikes(n):
    """30 everywhere, 90 at every 997th value: a running mean that moves in rare small steps."""
    a = np.full(n, 30, dtype=np.int32)
    a[::997] = 90
    return a


def _with(a, edits):
    a = a.copy()
    for lo, hi, v in edits:
        a[lo:hi] = v
    return a


def _alternating(n):
    a = _poisson(0x706C09, n)
    a[400:2600] = 1 << 24
    a[400:2600:300] = 0
    return a


def _flat_ref(n):
    a = np.full(n, 9, dtype=np.int32)
    a[1299:1700] = _poisson(0x706C08, 401, 20)
    return a


def cases():
    C = []
    C.append(Case("tiny", 3000, lambda: _poisson(0x706C01, 3000),
                  [(1500, 1500, 0), (1500, 1501, 1), (1500, 1600, 0), (1700, 1650, 1), (1500, 1500, 0)], True))        # length 1 (band 1), 2 (band 3), below m * minmlen, START > END, a duplicate
    C.append(Case("pieces", 2000, lambda: _poisson(0x706C02, 2000),
                  [(256, 700, 0), (257, 700, 1), (258, 700, 0), (514, 900, 1),                                    # a front piece of 255, 256, 257, 513 values
                   (1300, 1744, 0), (1300, 1743, 1), (1300, 1742, 0), (1100, 1486, 1)], True))                       # a back piece of 255, 256, 257, 513
    C.append(Case("band_is_nref", 1023, lambda: _poisson(0x706C03, 1023), [(256, 766, 0)], True))                    # 255 + 256 values under a band of 511
    C.append(Case("band_above_nref", 1000, lambda: _poisson(0x706C04, 1000),
                  [(2, 999, 0), (2, 998, 1), (6, 994, 0), (6, 993, 1), (3, 996, 0)], True))                          # nref 1, 2, 10, 11, 5
    C.append(Case("edges", 5000, lambda: _poisson(0x706C05, 5000),
                  [(1, 400, 0), (4000, 4999, 1), (4000, 5000, 0), (5001, 5100, 1), (4990, 5003, 0), (0, 300, 0), (-5, -2, 1)], True))   # no front piece, no back piece, END = n, beyond, start 0, negative
    C.append(Case("walk_1", 30001, lambda: _few(0x706C11, 30001), [(12000, 17999, 0)], True))                        # span 30000: step exactly 1
    C.append(Case("walk_1_00003", 30002, lambda: _few(0x706C12, 30002), [(12000, 17999, 1)], True))                  # span 30001
    C.append(Case("walk_1_5", 45001, lambda: _few(0x706C13, 45001), [(18000, 27000, 0)], False))
    C.append(Case("walk_2_6", 78001, lambda: _spikes(78001), [(31000, 46999, 1)], True))
    C.append(Case("zeros", 4000, lambda: _with(_poisson(0x706C06, 4000), [(1000, 3000, 0)]),
                  [(1800, 2200, 0), (900, 1100, 1), (2900, 3100, 0)], True))                                         # body and neighbourhood all zero; zeros on one side
    C.append(Case("flat_body", 3000, lambda: _with(_poisson(0x706C07, 3000), [(1000, 1400, 7)]), [(1001, 1400, 0)], True))
    C.append(Case("flat_neighbourhood", 3000, lambda: _flat_ref(3000), [(1300, 1700, 1)], True))                     # its "median" is the mean
    C.append(Case("wide_2p24", 3000, lambda: _alternating(3000), [(1300, 1699, 1), (1400, 1656, 0)], False))          # 0 beside 2^24 under bands of 401 and 257
    C.append(Case("wide_int_max", 2000, lambda: _with(_poisson(0x706C0A, 2000), [(500, 502, (1 << 31) - 1)]),
                  [(1000, 1001, 0)], False))                                                                          # 2^31 - 1 twice under band 3
    return collections.OrderedDict((c.name, c) for c in C)


def many_calls(n, count, seed, max_len=300):
    """count calls on an array of n values, with overlaps, duplicates and a few refused ones."""
    rng = np.random.default_rng(seed)
    start = rng.integers(1, n - 1, size=count)
    length = rng.integers(1, max_len + 1, size=count)
    calls = [(int(s), int(min(s + l - 1, n + 3 * (k % 97 == 0))), int(k % 2)) for k, (s, l) in enumerate(zip(start, length))]
    for k in range(0, count, 50):
        calls[k] = calls[(k * 7) % count]   # duplicates
    return calls


# ---- the restatement -----------------------------------------------------------------------------------------------------------

def g(x):
    """A double through the reference's `ostream << double`: %g, and the sign glibc prints in front of a NaN."""
    x = float(x)
    if math.isnan(x):
        return "-nan" if math.copysign(1.0, x) < 0 else "nan"
    return "%g" % x


def quantiles(v):
    """_lowerquartile / _median / _upperquartile on ints (partition_stat_tp, wufunctions.cpp:364-424): of n sorted values s[],
    s[max(n/4,1)-1], s[max(n/2,1)-1], s[max(3n/4,1)-1]; for all-equal values the median is the mean."""
    s = np.sort(np.asarray(v, dtype=np.int64))
    n = len(s)
    return tuple(float(s[max(r, 1) - 1]) for r in (n // 4, n // 2, n * 3 // 4))


def plan(start, end, n, m=M, minmlen=MINMLEN, chklen=CHKLEN):
    """The planner: a dict, or the refusal's number."""
    cs, ce = (start, end) if start <= end else (end, start)
    size = n
    if cs > size or ce > size:
        return 1
    d = ce - cs + 1
    if d < m * minmlen:
        d = int(m * minmlen)
    i1, i2 = int(cs - chklen * d), int(ce + chklen * d)
    i1 = max(i1, 1)
    i1 = min(i1, size - 1)
    i2 = min(i2, size - 1)
    c1, c2 = max(cs - 1, 0), ce - 1
    c1 = min(c1, size - 1)
    c2 = min(c2, size - 1)
    nref = abs(cs - i1 + i2 - ce)
    a0, b0 = i1 - 1, ce
    a1, b1 = max(cs - 1, a0), max(i2, b0)
    if i1 < 1 or (a1 - a0) + (b1 - b0) != nref or nref == 0 or b0 < 0:
        return 2
    if c2 - c1 + 1 <= 0:
        return 3
    d = abs(ce - cs) + 1
    band = d + ((d + 1) % 2)
    if band > nref:
        band = nref // 2 + ((nref // 2 + 1) % 2)
    while band > nref:
        band -= 2
    if band <= 0:
        return 4
    step = max((i2 - i1 + 1) / POINTS, 1.0)
    rows = [[], [], []]          # (pos, depth index or -1, neighbourhood index or -1)
    i = 0
    past = False                 # block 0 reaches position cs with no back piece: the reference indexes its running mean one past the end (its Array aborts)
    ir = i1 + 0.00001
    while ir < cs + 0.000011:
        i = int(ir)
        ic = i - 1
        past = past or (0 <= ic < size and i - i1 >= nref)
        rows[0].append((i, -1, -1) if ic < 0 or ic >= size else (i, ic, min(i - i1, nref - 1)))
        ir += step
    ir = cs + 0.00001
    while ir <= ce + 0.000011:
        ic = int(ir - 1)
        rows[1].append((i, -1, -1) if ic < 0 or ic >= size else (int(ir), ic, -1))
        ir += step
    ir = ce + 1.00001
    while ir <= i2 + 0.000011:
        ic = int(ir - 1)
        rows[2].append((i, -1, -1) if ic < 0 or ic >= size else (int(ir), ic, min(max(int(ir - i1 - d), 0), nref - 1)))
        ir += step
    imid1 = max(cs - 3 - i1, 0)
    imid2 = max(min(ce + 1 - i1 - d, nref - 1), 0)
    return dict(cs=cs, ce=ce, i1=i1, i2=i2, c1=c1, c2=c2, a=(a0, a1), b=(b0, b1), nref=nref, band=band, rows=rows, mid=(imid1, imid2), past=past)


def window_sum(pre, r, band, nref):
    h = band // 2
    c = min(max(r, h), nref - 1 - h)
    return int(pre[c + h + 1] - pre[c - h])


def files(rd, P, length, typ, p1, title, chrom_median, version, datfile, imgfile, fmt="ps"):
    """(.dat text, .gp text) of a planned call."""
    rd = np.asarray(rd)
    ref = np.concatenate([rd[P["a"][0]:P["a"][1]], rd[P["b"][0]:P["b"][1]]]).astype(np.int64)
    pre = np.concatenate([[0], np.cumsum(ref)])
    band, nref = P["band"], P["nref"]
    mean = lambda r: g(np.float32(window_sum(pre, r, band, nref) / band))
    clq, cmed, cuq = quantiles(rd[P["c1"]:P["c2"] + 1])
    rlq, rmed, ruq = quantiles(ref)
    with np.errstate(all="ignore"):
        refmean = np.float64(int(pre[-1])) / np.float64(nref)
        ymax = int(rmed * 2.25)
        y2max = np.float64(ymax) / refmean / np.float64(2.0)
    ymax = int(rmed * 2) if cmed < rmed else int(cuq + 1.5 * (ruq - rlq))
    cs, ce, i1, i2 = P["cs"], P["ce"], P["i1"], P["i2"]
    out = ["#%d ~ %d  %d  %s  %s\n" % (cs, ce, length, TYPES[typ if 0 <= typ <= 2 else 2], g(p1))]
    rdmax = 0
    for b in range(3):
        for pos, ic, r in P["rows"][b]:
            if ic < 0:
                out.append("%d\t0\tNaN\n" % pos)
                continue
            v = int(rd[ic])
            out.append("%d\t%d\t%s\n" % (pos, v, mean(r) if r >= 0 else "NaN"))
            if ic > 0 and v > rdmax:
                rdmax = v
        out.append("\n\n")
    out.append("%d\t%s\n%d\t%s\n\n\n" % (cs, mean(P["mid"][0]), ce, mean(P["mid"][1])))
    for q in (cmed, clq, cuq):
        out.append("%d\t%s\n%d\t%s\n\n\n" % (cs, g(q), ce, g(q)))
    for q in (rmed, rlq, ruq):
        out.append("%d\t%s\n%d\t%s\n\n\n" % (i1, g(q), i2, g(q)))
    out.append("NaN\tNaN\nNaN\tNaN\n\n\n")
    dat = "".join(out)

    term = {"ps": "postscript color enhanced solid", "eps": "postscript eps enhanced solid"}.get(fmt, "png xffffff x222222")
    title = title.replace("~", "-")
    if ymax > rdmax:
        ymax = rdmax + rdmax // 10
    d = (i2 - i1 + 1) // 6
    x1, x2 = i1 + d // 2, i2 - d // 2
    L = []
    if version > 4.19:
        L += ['f="%s"' % datfile, "set datafile missing 'NaN'", 'info="%s "' % title, "set terminal " + term, 'set output "%s"' % imgfile, "#set nokey",
              "##set label 1 info at graph  0.25, graph  0.9", "set title info offset 0,-0.5", "set xrange [%d:%d]" % (x1, x2),
              "set xtics %d,%d,%d" % (x1, d, x2), "set yrange [0:%d]" % ymax, "set y2range[0:%s]" % g(y2max), "set ytics nomirror", "plot \\",
              'f in 0 u 1:2 w p pt 7 ps 0.5 lt rgb "blue" t "Neighbor", \\', 'f in 1 u 1:2 w p pt 7 ps 0.5 lt rgb "red" t "CNV", \\',
              'f in 2 u 1:2 w p pt 7 ps 0.5 lt rgb "blue" not, \\', 'f in 0 u 1:3 w l lt 1 lw 8 lc rgb "green" t "Runmean", \\',
              'f in 2 u 1:3 w l lt 1 lw 8 lc rgb "green" not, \\', 'f in 3 u 1:2 w l lt 0 lw 8 lc rgb "green" not, \\',
              'f in 4 u 1:2 w l lt 1 lw 8 lc rgb "cyan" t "CNV med", \\', 'f in 5 u 1:2 w l lt 0 lw 8 lc rgb "cyan" t "CNV 1st,3rd quart", \\',
              'f in 6 u 1:2 w l lt 0 lw 8 lc rgb "cyan" not, \\', '%s w l lt 0 lw 8 lc rgb "green" t "Neighbor 1st,3rd quar", \\' % g(rlq),
              '%s w l lt 0 lw 8 lc rgb "green" not, \\' % g(ruq)]
        if chrom_median > 0:
            L.append('%s w l lt 4 lw 4 t "CHROM med", \\' % g(chrom_median))
        L.append("f in 10 u 1:2 not")
    else:
        f = '"%s"' % datfile
        L += ['#f="%s"' % datfile, '#info="%s "' % title, "set terminal " + term, 'set output "%s"' % imgfile, "#set nokey",
              'set title "%s" 0,-0.5' % title, "set xrange [%d:%d]" % (x1, x2), "set xtics %d,%d,%d" % (x1, d, x2), "set yrange [0:%d]" % ymax,
              "set ytics nomirror", "set y2range[0:%s]" % g(y2max), "plot \\",
              f + " in 0 u 1:2 w p pt 7 ps 0.5 lt 3 not, \\", f + " in 1 u 1:2 w p pt 7 ps 0.5 lt 1 not, \\", f + " in 2 u 1:2 w p pt 7 ps 0.5 lt 3 not, \\",
              f + ' in 0 u 1:3 w l lt 2 lw 8 t "runmean", \\', f + " in 2 u 1:3 w l lt 2 lw 8 not, \\", f + " in 3 u 1:2 w l lt 2 lw 2 not, \\",
              f + ' in 4 u 1:2 w l lt 5 lw 8 t "CNV med", \\', f + ' in 5 u 1:2 w l lt 5 lw 4 t "CNV 1st,3rd quart", \\',
              f + " in 6 u 1:2 w l lt 5 lw 4 not, \\", '%s w l lt 2 lw 2 t "Neighbor 1st,3rd quart", \\' % g(rlq), "%s w l lt 2 lw 2 not , \\" % g(ruq)]
        if chrom_median > 0:
            L.append('%s w l lt 4 lw 4 t "WG mean", \\' % g(chrom_median))
        L.append(f + " in 10 u 1:2 not")
    L += ["set output", "quit"]
    return dat, "\n".join(L) + "\n"


def chrom_median(rd):
    return quantiles(rd)[1]


def base_of(start, end, typ, folder="plots", chrom="chrS"):
    return "%s/rsi_%s_%d_%d_%s" % (folder, chrom, start, end, TYPES[typ])


def title_of(start, end, typ, chrom="chrS"):
    return "%s:%d~%d %d %s" % (chrom, start, end, end - start + 1, TYPES[typ])


def pack(text):
    """A file's text as it lies in tests/golden/plot_edges.npz: LZMA, as bytes."""
    import lzma
    return np.frombuffer(lzma.compress(text.encode(), preset=9), dtype=np.uint8)


def unpack(a):
    import lzma
    return lzma.decompress(np.asarray(a, dtype=np.uint8).tobytes()).decode()


def p1_of(k):
    return 1.25e-7 * (1 + k)
