"""GPU: plot data from the device.  The hook on every case of plot_cases with tiles of 256 values: every number of
every call equals the host fill's, both files of every call equal the host writer's byte for byte and, where
tests/golden/plot_edges.npz has them, the compiled reference's own; batches of 0, 1 and 3000 calls, lists that grow and shrink on
one context, a workspace that forces several batches, the launch counts; the expansion kernel; a 2 Mb synthetic chromosome with
gaps whose run's figures equal the host road's in byte and int32 storage, through the library and through the command line
(-plots device, with -samples too); and `rsicnv view` on a depth file and on the BAM it was dumped from."""
import contextlib
import os
import shutil
import subprocess

import numpy as np
import pytest

import bam_util as bu
import plot_cases as pc
from test_genome_text import write_fasta

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "rsicnv_amd", "bin", "rsicnv")
GOLDEN = os.path.join(ROOT, "tests", "golden", "plot_edges.npz")
CASES = pc.cases()


@pytest.fixture(scope="module")
def hot(hotlib):
    from rsicnv_amd import api
    h = api.RsiHot(0)
    yield h
    h.close()


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN, allow_pickle=False)


@contextlib.contextmanager
def inside(path):
    old = os.getcwd()
    os.makedirs(os.path.join(str(path), "plots"), exist_ok=True)
    os.chdir(str(path))
    try:
        yield
    finally:
        os.chdir(old)


def same(a, b):
    """a == b as a plain flag: an assert on two texts of 30 000 lines would have pytest work out their difference line by line."""
    return a == b


def planned(case, m=pc.M, minmlen=pc.MINMLEN, chklen=pc.CHKLEN, calls=None):
    from rsicnv_amd import api
    b = api.PlotBatch(case.n if hasattr(case, "n") else case, m, minmlen, chklen)
    for k, (s, e, t) in enumerate(case.calls if calls is None else calls):
        c = api.RsiCall()
        c.start, c.end, c.type, c.length, c.p1 = s, e, t, abs(e - s) + 1, pc.p1_of(k)
        b.add(s, e, t, call=c)
    return b


def write_all(batch, calls, where, version, tag=""):
    """Every call's files under where/plots; {k: (dat, gp)} of the written ones."""
    out = {}
    with inside(where):
        for k, (s, e, t) in enumerate(calls):
            base = pc.base_of(s, e, t) + tag
            if batch.write(k, pc.title_of(s, e, t), base + ".dat", base + ".gp", base + ".ps", gnuplot_version=version):
                out[k] = (open(base + ".dat").read(), open(base + ".gp").read())
                os.unlink(base + ".dat"); os.unlink(base + ".gp")
            else:
                assert not os.path.exists(base + ".dat") and not os.path.exists(base + ".gp")
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_every_case_equals_the_host_writer_and_the_reference(hot, golden, tmp_path, name):
    case = CASES[name]
    rd = case.build()
    dev, host = planned(case), planned(case)
    hot.debug_plot(rd, dev, tile=pc.TILE)
    host.fill_host(rd)
    assert [dev.refusal(k) for k in range(len(dev))] == [0 if isinstance(pc.plan(s, e, case.n), dict) else pc.plan(s, e, case.n) for s, e, _ in case.calls]
    assert dev.compare(host) == 0 and dev.chrom_median() == pc.chrom_median(rd)
    version = float(golden["version"][0])
    for v in (5.0, version):
        got, want = write_all(dev, case.calls, tmp_path / "dev", v), write_all(host, case.calls, tmp_path / "host", v)
        assert same(got, want) and sorted(got) == [k for k in range(len(dev)) if dev.refusal(k) == 0]
    st = hot.plot_stats()
    assert st["calls"] == len(got) and st["batches"] == (1 if got else 0) and st["queries"] == dev.queries()
    if case.golden:
        assert float(golden[name + "_rdmed"][0]) == dev.chrom_median()
        seen = 0
        for k, (dat, gp) in got.items():
            if f"{name}_{k}_dat" in golden:
                assert same(pc.unpack(golden[f"{name}_{k}_dat"]), dat) and same(pc.unpack(golden[f"{name}_{k}_gp"]), gp), (name, k)
                seen += 1
        assert seen >= 1


@pytest.mark.parametrize("tile", [0, 7, 1000, 4096])
def test_other_tiles(hot, tile):
    for name in ("pieces", "band_above_nref", "wide_2p24", "zeros"):
        case = CASES[name]
        rd = case.build()
        dev, host = planned(case), planned(case)
        hot.debug_plot(rd, dev, tile=tile)
        host.fill_host(rd)
        assert dev.compare(host) == 0, (name, tile)
    from rsicnv_amd import api
    with pytest.raises(api.RsiError):
        hot.debug_plot(rd, dev, tile=4097)


@pytest.fixture(scope="module")
def many():
    n = 80_000
    rd = np.random.default_rng(0x706C20).poisson(30, size=n).astype(np.int32)
    calls = pc.many_calls(n, 3000, 0x706C21)
    host = planned(n, 5, 2.0, 2.0, calls)
    host.fill_host(rd)
    return n, rd, calls, host


def test_batches_of_0_1_and_3000_calls(hotlib, many):
    from rsicnv_amd import api
    n, rd, calls, host = many
    h = api.RsiHot(0)
    try:
        st = h.plot_stats()
        assert st["launches"] == 0 and st["bytes"] == 0
        empty = planned(n, 5, 2.0, 2.0, [])
        h.debug_plot(rd, empty, tile=pc.TILE)
        refused = planned(n, 5, 2.0, 2.0, [(n + 5, n + 9, 0)])
        h.debug_plot(rd, refused, tile=pc.TILE)
        st = h.plot_stats()
        assert st["launches"] == 0 and st["bytes"] == 0 and st["batches"] == 0       # nothing to fill: nothing allocated, nothing launched
        assert refused.compare(refused) == 0 and refused.chrom_median() == 0.0
        one, one_host = planned(n, 5, 2.0, 2.0, calls[1:2]), planned(n, 5, 2.0, 2.0, calls[1:2])
        h.debug_plot(rd, one, tile=pc.TILE)
        one_host.fill_host(rd)
        assert one.compare(one_host) == 0 and h.plot_stats()["batches"] == 1
        big = planned(n, 5, 2.0, 2.0, calls)
        assert sum(big.refusal(k) != 0 for k in range(len(big))) >= 1
        for count in (3000, 2, 3000):                                                # a list that shrinks and grows on one context
            b = planned(n, 5, 2.0, 2.0, calls[:count])
            h.debug_plot(rd, b, tile=pc.TILE, workspace_bytes=1 << 31)
            assert h.plot_stats()["batches"] == 1
            ref = host if count == 3000 else planned(n, 5, 2.0, 2.0, calls[:count])
            if count != 3000:
                ref.fill_host(rd)
            assert b.compare(ref) == 0, count
        launches_3000 = h.plot_stats()["launches"]
        ten = planned(n, 5, 2.0, 2.0, calls[:10])
        h.debug_plot(rd, ten, tile=pc.TILE, workspace_bytes=1 << 31)
        assert h.plot_stats()["launches"] == launches_3000 and h.plot_stats()["batches"] == 1
        # the default workspace cuts the list into batches; the launch count follows the batches alone
        h.debug_plot(rd, big, tile=pc.TILE)
        st = h.plot_stats()
        assert big.compare(host) == 0 and st["batches"] >= 3
        per_batch = launches_3000 - 5                                                # the array's median: geno's 3 + one pass of 2
        assert st["launches"] == 5 + st["batches"] * per_batch
    finally:
        h.close()


def test_a_small_workspace_gives_the_same_bytes(hot, tmp_path):
    case = CASES["pieces"]
    rd = case.build()
    whole, cut = planned(case), planned(case)
    hot.debug_plot(rd, whole, tile=pc.TILE)
    assert hot.plot_stats()["batches"] == 1
    hot.debug_plot(rd, cut, tile=pc.TILE, workspace_bytes=250_000)
    assert hot.plot_stats()["batches"] >= 3
    assert cut.compare(whole) == 0
    assert same(write_all(cut, case.calls, tmp_path / "cut", 5.0), write_all(whole, case.calls, tmp_path / "whole", 5.0))


@pytest.mark.parametrize("storage", [1, 4])
def test_expand_kernel(hot, storage):
    rng = np.random.default_rng(0x706C30)
    n = 70_001
    for regions in ([], [0, 99], [0, 99, 1000, 1499, 33000, 41234, 69990, 70000], [5, 5, 7, 7, 9, 300]):
        keep = np.ones(n, dtype=bool)
        for s, e in np.array(regions, dtype=np.int64).reshape(-1, 2):
            keep[s:e + 1] = False
        rdc = rng.integers(1, 250 if storage == 1 else 1 << 30, size=int(keep.sum())).astype(np.int32)
        want = np.zeros(n, dtype=np.int32)
        want[keep] = rdc
        assert np.array_equal(hot.debug_plot_expand(rdc, regions, n, storage=storage), want), regions
    from rsicnv_amd import api
    with pytest.raises(api.RsiError):
        hot.debug_plot_expand(rdc[:-1], [5, 5, 7, 7, 9, 300], n, storage=storage)   # the lengths do not add up


# ---------------------------------------------------------------------------------------------------------------------
# a run's own depth
# ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def chrom(hotlib):
    """About 2 Mb, two N runs inside, a planted deletion and a planted duplication."""
    from rsicnv_amd import synth
    plan = synth.make_plan(n=2_000_003, seed=0x706C40, model=0, n_events=4, gaps=2, min_len=20000, max_len=60000, end_n=0, gap_len=30000)
    fasta, depth = synth.generate_host(hotlib, plan)
    return plan, fasta, depth


@pytest.mark.parametrize("cap", [4.0, -1.0])
def test_run_figures_equal_the_host_road(hot, chrom, cap, tmp_path):
    """cap 4: the compacted depth is bytes; no cap: int32."""
    from rsicnv_amd import api
    plan, fasta, depth = chrom
    n = plan["n"]
    res = hot.run(api.make_params(m=pc.M, cap=cap), depth, fasta)
    calls = [(c["start"], c["end"], c["type"]) for c in res.calls("calls")]
    assert len(calls) >= 2
    calls += [(a - 500, b + 700, 0) for a, b in plan["nruns"]] + [(1, 5000, 1), (n - 4000, n - 1, 0), (n - 10, n + 10, 1)]
    dev, host = planned(n, calls=calls), planned(n, calls=calls)
    hot.plot_run(res, dev)
    st = hot.plot_stats()
    rdc, pairs = hot.fetch("rd_concat"), res.noncode
    keep = np.ones(n, dtype=bool)
    for s, e in pairs.reshape(-1, 2):
        keep[s:e + 1] = False
    full = np.zeros(n, dtype=np.int32)
    full[keep] = rdc
    host.fill_host(full)
    assert dev.compare(host) == 0 and dev.chrom_median() == pc.chrom_median(full)
    assert same(write_all(dev, calls, tmp_path / "dev", 5.0), write_all(host, calls, tmp_path / "host", 5.0))
    assert st["batches"] == 1 and st["calls"] == len(calls) - 1 and st["bytes_down"] < 13 * dev.queries() + 4096 and st["bytes_up"] < 9 * dev.queries() + 65536
    # a hook that overwrites the run's depth: the context says so instead of plotting something else
    hot.debug_geno(np.arange(10, dtype=np.int32), 4, [0], [5], [0], [0], [5], [9])
    with pytest.raises(api.RsiError):
        hot.plot_run(res, dev)


def same_folders(a, b):
    """Both folders (ph/plots... and pd/plots...) hold the same files; everything but the images gnuplot draws is the same byte
    for byte, but for the folder's own name, which a script carries in its file names."""
    fa, fb = sorted(os.listdir(a)), sorted(os.listdir(b))
    assert fa == fb and fa
    for f in fa:
        if not f.endswith((".ps", ".png")):
            assert same(open(os.path.join(a, f)).read(), open(os.path.join(b, f)).read().replace("pd/plots", "ph/plots")), f
    return fa


def rsi(tmp, args, expect=0):
    r = subprocess.run([EXE, "rsi", *args], cwd=str(tmp), capture_output=True, text=True, timeout=300)
    assert r.returncode == expect, r.stderr[-2500:]
    return r


@pytest.mark.parametrize("cap", ["4", "-1"])
def test_cli_plots_device(hotlib, chrom, tmp_path, cap):
    from rsicnv_amd import synth
    plan, fasta, depth = chrom
    fa, rd_path = synth.write_case_files(hotlib, fasta, depth, str(tmp_path))
    common = ["-d", rd_path, "-c", "chrS", "-f", fa, "-cap", cap, "-plotfiles"]
    rsi(tmp_path, common + ["-o", "host.txt", "-p", "ph/plots", "-plots", "host"])
    rsi(tmp_path, common + ["-o", "dev.txt", "-p", "pd/plots", "-plots", "device"])
    files = same_folders(str(tmp_path / "ph" / "plots"), str(tmp_path / "pd" / "plots"))
    rows = open(str(tmp_path / "host.txt")).read()
    assert same(rows, open(str(tmp_path / "dev.txt")).read()) and len(rows.splitlines()) >= 3
    if shutil.which("gnuplot") is None:
        assert len(files) == 2 * (len([r for r in rows.splitlines() if r.startswith("chrS")]))
    log_h, log_d = open(str(tmp_path / "host.txt.log")).read(), open(str(tmp_path / "dev.txt.log")).read()
    assert log_d.count("#plots: chrS: ") == 1 and "#plots:" not in log_h and log_d.count("plotting: ") == log_h.count("plotting: ") >= 1
    r = rsi(tmp_path, common + ["-o", "no.txt", "-plots", "gpu"], expect=1)
    assert "-plots" in r.stderr and not os.path.exists(str(tmp_path / "no.txt"))


def test_cli_plots_device_with_samples(hotlib, tmp_path):
    from conftest import make_case
    specs = [("chrA", 200_003, 0x706C50), ("chrB", 150_001, 0x706C60)]
    seqs, cols = [], []
    for name, n, seed in specs:
        ds = []
        for s in range(3):
            plan, fa, d = make_case(hotlib, dict(n=n, seed=seed + s, model=0, mean=30.0 + 6 * s, n_events=3, gaps=1, max_len=20000, end_n=3000, gap_len=6000))
            ds.append(d)
            if s == 0:
                seqs.append((name, fa))
        cols.append((name, n, np.stack(ds)))
    fa_path = str(tmp_path / "ref.fa")
    write_fasta(fa_path, seqs)
    (tmp_path / "cohort.depth").write_text("#CHROM\tPOS\tS1\tS2\tS3\n" + "".join("".join(f"{name}\t{p + 1}\t{d[0, p]}\t{d[1, p]}\t{d[2, p]}\n" for p in range(n))
                                                                                 for name, n, d in cols))
    common = ["-d", str(tmp_path / "cohort.depth"), "-f", fa_path, "-samples", "all", "-plotfiles"]
    rsi(tmp_path, common + ["-o", "host.txt", "-p", "ph/plots"])
    rsi(tmp_path, common + ["-o", "dev.txt", "-p", "pd/plots", "-plots", "device"])
    total = 0
    for k in (1, 2, 3):
        total += len(same_folders(str(tmp_path / "ph" / "plots" / str(k)), str(tmp_path / "pd" / "plots" / str(k))))
        assert same(open(str(tmp_path / f"host.txt.{k}")).read(), open(str(tmp_path / f"dev.txt.{k}")).read())
        assert "#plots: chr" in open(str(tmp_path / f"dev.txt.{k}.log")).read()
    assert total >= 6


# ---------------------------------------------------------------------------------------------------------------------
# rsicnv view
# ---------------------------------------------------------------------------------------------------------------------

def view(tmp, args, expect=0):
    r = subprocess.run([EXE, "view", *args], cwd=str(tmp), capture_output=True, text=True, timeout=300)
    assert r.returncode == expect, r.stderr[-2500:]
    return r


def test_view_on_a_depth_file_and_on_its_bam(hot, hotlib, tmp_path):
    from conftest import make_case
    n = 150_001
    plan, fasta, depth = make_case(hotlib, dict(n=n, seed=0x706C70, model=0, mean=20.0, n_events=3, gaps=1, max_len=12000, end_n=3000, gap_len=5000))
    fa_path = str(tmp_path / "ref.fa")
    write_fasta(fa_path, [("chrS", fasta), ("chrT", fasta[:9000])])
    bam = str(tmp_path / "small.bam")
    bu.write_bam(bam, [("chrS", n), ("chrT", 9000)], bu.paired_reads_following_depth(depth, n))
    hot.load_depth_bam(bam, "chrS")
    rd = hot.fetch("depth_in")
    assert rd.size == n and int(rd[n - 1]) == 0 and int(rd.max()) > 5
    dump = str(tmp_path / "chrS.depth")
    open(dump, "w").write("".join(f"{p + 1}\t{v}\n" for p, v in enumerate(rd.tolist())))
    lines = [(a + 1, b, "DEL" if k % 2 == 0 else "dup_x") for k, (a, b, _) in enumerate(plan["events"])]
    lines += [(70_000, 70_000, "DEL"), (500, 90, "gain"), (n - 400, n - 1, "loss"), (n - 400, n, "DEL"), (n + 1, n + 50, "DUP"), (30_000, 75_000, "other")]
    names = ["chrS" if k % 2 == 0 else "S" for k in range(len(lines))]                  # with and without chr
    cnv = tmp_path / "list.txt"
    cnv.write_text("#a comment\n" + "".join(f"{c}\t{s}\t{e}\t{t}\tx\n" for c, (s, e, t) in zip(names, lines)) + "chrQ\t100\t2000\tDEL\n")
    view(tmp_path, ["-d", dump, "-c", "chrS", "-f", fa_path, "-v", str(cnv), "-p", "vd/plots", "-plotfiles"])
    view(tmp_path, ["-b", bam, "-v", str(cnv), "-p", "vb/plots", "-plotfiles"])
    fd, fb = str(tmp_path / "vd" / "plots"), str(tmp_path / "vb" / "plots")
    files = [f for f in sorted(os.listdir(fd)) if f != "view.log"]
    assert files == [f for f in sorted(os.listdir(fb)) if f != "view.log"]
    refused = {6, 7}                                                                   # END = n: size error; beyond the array
    want_names = sorted(f"rsi_chrS_{s}_{e}_{t}.{x}" for k, (s, e, t) in enumerate(lines) if k not in refused for x in ("dat", "gp"))
    if shutil.which("gnuplot") is None:
        assert files == want_names
    for f in files:
        if f.endswith((".dat", ".gp")):
            assert same(open(os.path.join(fd, f)).read(), open(os.path.join(fb, f)).read().replace("vb/plots", "vd/plots")), f
    # ... and both are the host writer's on the fetched depth
    kinds = {"DEL": 0, "dup_x": 1, "gain": 1, "loss": 0, "DUP": 1, "other": 2}
    host = planned(n, calls=[])
    for s, e, t in lines:
        host.add(s, e, kinds[t])
    host.fill_host(rd)
    assert [host.refusal(k) != 0 for k in range(len(lines))] == [k in refused for k in range(len(lines))]
    with inside(tmp_path / "hw"):
        os.makedirs("vd/plots")
        for k, (s, e, t) in enumerate(lines):
            if k in refused:
                continue
            base = f"vd/plots/rsi_chrS_{s}_{e}_{t}"
            assert host.write(k, f"chrS:{s}-{e} {abs(e - s) + 1} {t}", base + ".dat", base + ".gp", base + ".ps")
            if shutil.which("gnuplot") is None:
                for x in (".dat", ".gp"):
                    assert same(open(base + x).read(), open(os.path.join(fd, os.path.basename(base) + x)).read()), (k, x)
    for folder in (fd, fb):
        log = open(os.path.join(folder, "view.log")).read()
        assert log.count("#view: chrQ is not in the input") == 1 and log.count("size error") == 1 and log.count("beyond the array") == 1
        assert log.count("#plots: chrS: ") == 1 and f"{len(lines)} lines, {len(lines) - 2} figures" in log
    # refusals leave no file
    for args, word in ((["-d", dump, "-f", fa_path, "-v", str(cnv)], "-c"), (["-d", dump, "-c", "chrS", "-f", fa_path, "-v", str(cnv), "-samples", "all"], "-samples"),
                       (["-b", bam, "-v", str(cnv), "-gpus", "2"], "-gpus"), (["-b", bam], "-v")):
        r = view(tmp_path, args + ["-p", "never/plots", "-plotfiles"], expect=1)
        assert word in r.stderr and not os.path.exists(str(tmp_path / "never"))
    if shutil.which("gnuplot") is None:
        r = view(tmp_path, ["-b", bam, "-v", str(cnv), "-p", "never/plots"])
        assert "gnuplot not found" in r.stderr and not os.path.exists(str(tmp_path / "never"))
    u = subprocess.run([EXE], capture_output=True, text=True, timeout=60)
    assert "rsicnv view" in u.stderr and "-plots device|host" in u.stderr


def test_unarmed_and_abi(hotlib, chrom):
    """A plain run allocates and launches nothing for the plots; the header, the bindings and the library agree on the names."""
    import re
    from rsicnv_amd import api
    plan, fasta, depth = chrom
    h = api.RsiHot(0)
    try:
        with pytest.raises(api.RsiError):
            h.plot_depth(0, 100, planned(100, calls=[(10, 20, 0)]))
        h.run(api.make_params(m=pc.M), depth[:400_000], fasta[:400_000])
        st = h.plot_stats()
        assert st["launches"] == 0 and st["bytes"] == 0 and st["batches"] == 0
    finally:
        h.close()
    hdr = open(os.path.join(ROOT, "include", "rsi_hot.h")).read()
    for sym in ("rsi_hot_plot_depth", "rsi_hot_plot_run", "rsi_hot_last_plot_stats", "rsi_hot_debug_plot", "rsi_hot_debug_plot_expand", "rsi_plot_batch_new",
                "rsi_plot_batch_write", "rsi_plot_batch_compare"):
        assert re.search(r"\b" + sym + r"\(", hdr) and sym in api.EXPORTS and hasattr(hotlib, sym)
    body = re.search(r"typedef struct rsi_plot_stats \{(.*?)\} rsi_plot_stats;", hdr, re.S).group(1)
    names = [nm.strip() for _, group in re.findall(r"(int64_t|double)\s+([^;]+);", body) for nm in group.split(",")]
    assert names == [f[0] for f in api.RsiPlotStats._fields_]
