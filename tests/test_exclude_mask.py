"""Excluded regions (rsi_hot_set_exclude, `rsicnv rsi -x`): a run with mask M on sequence F must give what a run without a
mask gives on F', F with M's bases replaced by 'N'.  The kernel alone through rsi_hot_debug_classify against numpy, the whole
path against the oracle and against the library itself on F', the command line against the reference binary and against its
own runs on the masked FASTA file."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from conftest import calls_equal, make_case, small_cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "rsicnv_amd", "bin", "rsicnv")


@pytest.fixture(scope="module")
def hot():
    from rsicnv_amd import api
    h = api.RsiHot(0)
    yield h
    h.close()


def masked(fasta, mask):
    """F': every base of the mask's intervals (0-based half-open, any order, clipped to the sequence) becomes N."""
    out = np.array(fasta, dtype=np.uint8, copy=True)
    for s, e in mask:
        s, e = max(int(s), 0), min(int(e), out.size)
        if e > s:
            out[s:e] = ord("N")
    return out


# ---- the kernel alone ---------------------------------------------------------------------------------------------------

def planes(seq):
    """The two planes as K1 writes them: n // 64 + 1 little-endian words, bit j of word w for base 64 w + j, zero beyond n."""
    nwords = seq.size // 64 + 1
    def pack(bits):
        padded = np.zeros(nwords * 64, dtype=np.uint8)
        padded[:seq.size] = bits
        return np.packbits(padded, bitorder="little").view("<u8").astype(np.uint64)
    return pack((seq == ord("G")) | (seq == ord("C"))), pack(seq == ord("N"))


def random_sequence(n, seed):
    rng = np.random.default_rng(seed)
    seq = rng.choice(np.frombuffer(b"ACGTNacgtn", dtype=np.uint8), size=n, p=[.2, .2, .2, .2, .05, .04, .04, .04, .02, .01])
    if n > 600:   # N runs across word boundaries, for the masks laid over them
        seq[100:300] = ord("N")
        seq[500:520] = ord("N")
    return seq


def kernel_masks(n):
    return {
        "first_base": [(0, 1)],
        "last_base": [(n - 1, n)],
        "across_a_word_boundary": [(63, 65)],
        "one_whole_word": [(64, 128)],
        "long": [(10, 4000)],
        "two_in_one_word": [(3, 9), (20, 41)],
        "two_in_one_word_and_a_third_reaching_in": [(130, 135), (150, 160), (190, 700)],
        "touching_pairs": [(5, 64), (64, 70), (1000, 1024), (1024, 1100), (1100, 1101)],
        "overlapping_pairs": [(5, 70), (60, 140), (1000, 2000), (1500, 1600), (1990, 2100)],
        "reversed_and_empty": [(50, 40), (77, 77), (90, 95), (200, 100)],
        "only_reversed_and_empty": [(50, 40), (77, 77)],
        "beyond_n": [(n, n + 10), (n + 100, n + 200), (3, 5)],
        "partly_beyond_n": [(n - 3, n + 70), (max(n - 200, 0), n + 1)],
        "negative_start": [(-5, 3), (-9, -2)],
        "unsorted": [(3000, 3100), (10, 20), (640, 1280), (100, 130), (2000, 2001)],
        "every_second_base": [(i, i + 1) for i in range(0, 5003, 2)],
        "over_existing_n": [(100, 300), (510, 515), (90, 101)],
        "whole_sequence": [(0, n)],
        "tile_edges": [(4094, 4097), (65535, 65537), (65400, 65600)],
    }


KERNEL_N = [1, 63, 64, 65, 4096, 5003]


@functools.lru_cache(maxsize=None)
def kernel_sequence(n):
    seq = random_sequence(n, 0xE0 + n)
    seq.setflags(write=False)
    return seq


@pytest.mark.parametrize("n", KERNEL_N)
def test_no_intervals_is_the_unmasked_classification(hot, n):
    seq = kernel_sequence(n)
    gc, nb = hot.debug_classify(seq)
    exp_gc, exp_nb = planes(seq)
    assert np.array_equal(gc, exp_gc) and np.array_equal(nb, exp_nb)
    gc0, nb0 = hot.debug_classify(seq, exclude=[])
    assert np.array_equal(gc0, exp_gc) and np.array_equal(nb0, exp_nb)


@pytest.mark.parametrize("n", KERNEL_N)
@pytest.mark.parametrize("mask", sorted(kernel_masks(100)))
def test_kernel_planes_equal_numpy(hot, n, mask):
    seq = kernel_sequence(n)
    m = kernel_masks(n)[mask]
    gc, nb = hot.debug_classify(seq, exclude=m)
    exp_gc, exp_nb = planes(masked(seq, m))
    bad = np.flatnonzero((gc != exp_gc) | (nb != exp_nb))
    assert bad.size == 0, f"n={n} {mask}: {bad.size} words differ, first {bad[:4]}: nbits {nb[bad[:4]]} expected {exp_nb[bad[:4]]}"
    assert gc.size == n // 64 + 1 and nb.size == n // 64 + 1


def test_kernel_is_idempotent_and_takes_an_array(hot):
    seq = kernel_sequence(5003)
    m = np.array(kernel_masks(5003)["unsorted"], dtype=np.int32)
    first = hot.debug_classify(seq, exclude=m)
    second = hot.debug_classify(seq, exclude=np.concatenate([m, m]))   # every interval twice
    assert np.array_equal(first[0], second[0]) and np.array_equal(first[1], second[1])


def test_long_interval_is_spread_over_the_grid(hot):
    n = 2_000_003
    seq = random_sequence(n, 0xE1)
    sparse = [(65_530, 65_540), (131_071, 131_073), (196_608, 196_700), (262_100, 262_144), (327_680, 327_681)]   # at the edges of 65 536-base tiles
    for m in ([(1000, 1_900_000)], [(1000, 1_900_000), (1_900_001, 1_900_002), (1_950_000, n + 5), (3, 4)], sparse):
        gc, nb = hot.debug_classify(seq, exclude=m)
        exp_gc, exp_nb = planes(masked(seq, m))
        bad = np.flatnonzero((gc != exp_gc) | (nb != exp_nb))
        assert bad.size == 0, f"{bad.size} words differ, first {bad[:4]}"


def test_bad_arguments(hot):
    from rsicnv_amd import api
    s = np.array([1, 5], dtype=np.int64)
    e = np.array([3, 9], dtype=np.int64)
    L = hot.lib
    assert L.rsi_hot_set_exclude(hot.ctx, s.ctypes.data, e.ctypes.data, -1) == -2
    assert L.rsi_hot_set_exclude(hot.ctx, None, e.ctypes.data, 2) == -2
    assert L.rsi_hot_set_exclude(hot.ctx, s.ctypes.data, None, 2) == -2
    assert L.rsi_hot_set_exclude(hot.ctx, None, None, 0) == 0
    with pytest.raises(api.RsiError):
        hot.debug_classify(np.zeros(0, dtype=np.uint8))


# ---- the whole path -----------------------------------------------------------------------------------------------------

FLAG_SETS = {   # flag set -> (the conftest.small_cases plan it runs on, flags)
    "default": ("poisson_tail7", dict()),
    "nogc": ("poisson_nogc", dict(gcadjust=0)),
    "med_m51": ("gampois_med_m51_cap4", dict(m=51, trans=1)),
}
MASKS = ["wide", "many200", "many600"]


@functools.lru_cache(maxsize=None)
def chromosome(flags):
    from rsicnv_amd import api
    plan_kw = next(c[1] for c in small_cases() if c[0] == FLAG_SETS[flags][0])
    plan, fasta, depth = make_case(api.load_library(), plan_kw)
    fasta.setflags(write=False)
    depth.setflags(write=False)
    return plan, fasta, depth


def path_mask(plan, which):
    n = plan["n"]
    if which == "wide":   # a planted event, an existing N gap, both chromosome ends (the last one reaching beyond n)
        ev = plan["events"][1]
        gap = next(r for r in plan["nruns"] if r[0] > 0 and r[1] < n)
        return [(ev[0] - 2000, ev[1] + 3000), (gap[0] - 3000, gap[0] + 1000), (0, 9000), (n - 7000, n + 500)]
    k = 200 if which == "many200" else 600   # 20 bases every 600: none merges at a padding of 50; more than 128 regions / 512 runs
    return [(20_000 + 600 * i, 20_020 + 600 * i) for i in range(k)]


@functools.lru_cache(maxsize=None)
def oracle_on_masked(flags, which):
    """The oracle on (depth, F'), once per (flag set, mask): what the comparisons below need, copied out of it."""
    import oracle
    plan, fasta, depth = chromosome(flags)
    O = oracle.Oracle()
    O.run(oracle.make_params(**FLAG_SETS[flags][1]), depth, masked(fasta, path_mask(plan, which)))
    return dict(noncode=O.i32("noncode").copy(), rd_concat=O.i32("rd_concat").copy(), binmedint=O.i32("binmedint").copy(),
                chrom=O.f64("chrom").copy(), calls=O.calls("calls"), calls_raw=O.calls("calls_raw"), blocks=O.calls("blocks"))


@pytest.mark.parametrize("which", MASKS)
@pytest.mark.parametrize("flags", sorted(FLAG_SETS))
def test_masked_run_equals_oracle_and_library_on_masked_fasta(hot, flags, which):
    from rsicnv_amd import api
    plan, fasta, depth = chromosome(flags)
    mask = path_mask(plan, which)
    p = api.make_params(**FLAG_SETS[flags][1])
    ref = oracle_on_masked(flags, which)
    res = hot.run(p, depth, fasta, exclude=mask)
    st = res.stats
    rdc, binmed = hot.fetch("rd_concat"), hot.fetch("binmedint")
    # against the oracle on F'
    assert np.array_equal(res.noncode, ref["noncode"])
    assert st["n_compact"] == ref["rd_concat"].size and st["nbins"] == ref["binmedint"].size
    if FLAG_SETS[flags][1].get("cap", 4.0) > 1:
        assert st["cap_median"] == ref["chrom"][2]
    assert np.array_equal(binmed, ref["binmedint"])
    assert np.array_equal(rdc, ref["rd_concat"])
    for key in ("blocks", "calls_raw", "calls"):
        ok, why = calls_equal(res.calls(key), ref[key])
        assert ok, f"{flags} {which} {key}: {why}"
    assert st["RDmedian"] == ref["chrom"][0] and st["RDsd"] == ref["chrom"][1]
    if which == "wide":
        assert len(res.calls("calls_raw")) >= 1, "the case should still call an implanted event"
        assert st["n_noncode"] <= 8
    else:
        assert st["n_noncode"] > (128 if which == "many200" else 512)
    # against the library on F', unmasked: the same planes, the same path
    own = hot.run(p, depth, masked(fasta, mask))
    for key in ("segs", "blocks", "calls_raw", "calls"):
        ok, why = calls_equal(res.calls(key), own.calls(key), rtol=0)
        assert ok, f"{flags} {which} {key}: {why}"
    assert st["RDmedian"] == own.stats["RDmedian"] and st["RDsd"] == own.stats["RDsd"]
    assert np.array_equal(res.noncode, own.noncode)
    assert np.array_equal(rdc, hot.fetch("rd_concat")) and np.array_equal(binmed, hot.fetch("binmedint"))


def same_result(a, b):
    ok, why = calls_equal(a.calls("calls"), b.calls("calls"), rtol=0)
    assert ok, why
    ok, why = calls_equal(a.calls("calls_raw"), b.calls("calls_raw"), rtol=0)
    assert ok, why
    assert np.array_equal(a.noncode, b.noncode)
    for k in ("n_compact", "nbins", "n_noncode", "cap_median", "RDmedian", "RDsd"):
        assert a.stats[k] == b.stats[k], k


@pytest.mark.parametrize("which", ["wide", "many200"])
def test_device_and_text_entry_points(hot, tmp_path, which):
    import torch
    from rsicnv_amd import api
    plan, fasta, depth = chromosome("default")
    mask = path_mask(plan, which)
    fm = masked(fasta, mask)
    p = api.make_params()
    d_rd = torch.from_numpy(np.array(depth)).cuda()
    d_fa, d_fm = torch.from_numpy(np.array(fasta)).cuda(), torch.from_numpy(fm).cuda()
    torch.cuda.synchronize()
    a = hot.run_device(p, d_rd.data_ptr(), d_fa.data_ptr(), depth.size, exclude=np.array(mask))
    b = hot.run_device(p, d_rd.data_ptr(), d_fm.data_ptr(), depth.size)
    same_result(a, b)
    assert np.array_equal(d_fa.cpu().numpy(), fasta), "the caller's sequence in HBM is not modified"
    same_result(a, hot.run(p, depth, fm))
    path = str(tmp_path / "depth.txt")
    d32 = np.ascontiguousarray(depth, dtype=np.int32)
    hot.lib.rsi_synth_write_depth_text.argtypes = [C.c_char_p, C.c_void_p, C.c_int64]
    assert hot.lib.rsi_synth_write_depth_text(path.encode(), d32.ctypes.data, d32.size) == 0
    same_result(hot.run_text(p, path, fasta, exclude=mask), hot.run_text(p, path, fm))


def test_the_mask_is_spent_by_one_run(hot):
    from rsicnv_amd import api
    plan, fasta, depth = chromosome("default")
    mask = path_mask(plan, "wide")
    p = api.make_params()
    plain = hot.run(p, depth, fasta)
    with_mask = hot.run(p, depth, fasta, exclude=mask)
    assert with_mask.stats["n_compact"] < plain.stats["n_compact"]
    same_result(hot.run(p, depth, fasta), plain)           # not armed again: unmasked
    # a run that fails spends the mask too (gccontent.cpp:66-71: too short for the GC adjustment)
    hot.set_exclude(mask)
    with pytest.raises(api.RsiError) as e:
        hot.run(p, depth[:4000], fasta[:4000])
    assert e.value.code == -4
    same_result(hot.run(p, depth, fasta), plain)
    # armed, then disarmed
    hot.set_exclude(mask)
    hot.set_exclude(None)
    same_result(hot.run(p, depth, fasta), plain)
    # armed through set_exclude alone
    hot.set_exclude(mask)
    same_result(hot.run(p, depth, fasta), with_mask)


def test_region_limit_is_the_masked_fastas(hot):
    from rsicnv_amd import api
    # no N inside the chromosome: every interval is a region of its own
    _, fasta, depth = make_case(hot.lib, dict(n=600_000, seed=0xE45, model=0, n_events=4, gaps=0, max_len=15000, end_n=5000))
    mask = [(6000 + 140 * i, 6010 + 140 * i) for i in range(4100)]   # 130 bases apart: none merges at a padding of 50
    isn = np.concatenate([[0], (masked(fasta, mask) == ord("N")).astype(np.int8), [0]])
    starts, ends = np.flatnonzero(np.diff(isn) == 1), np.flatnonzero(np.diff(isn) == -1)
    assert starts.size == 4102 and (starts[1:] - ends[:-1] > 101).all()   # the regions the padding of 50 leaves apart
    p = api.make_params()
    with pytest.raises(api.RsiError) as e_mask:
        hot.run(p, depth, fasta, exclude=mask)
    with pytest.raises(api.RsiError) as e_own:
        hot.run(p, depth, masked(fasta, mask))
    assert e_mask.value.code == e_own.value.code == -5
    assert str(e_mask.value) == str(e_own.value)
    hot.run(p, depth, fasta)   # and the context goes on, unmasked


def test_unmasked_runs_launch_nothing_new(hot):
    from rsicnv_amd import api
    plan, fasta, depth = chromosome("default")
    p = api.make_params()
    hot.set_timing(True)
    try:
        hot.run(p, depth, fasta)
        plain = [k for k, _ in hot.kernel_times()]
        hot.run(p, depth, fasta, exclude=path_mask(plan, "wide"))
        with_mask = [k for k, _ in hot.kernel_times()]
        hot.run(p, depth, fasta, exclude=[(5, 5), (depth.size + 3, depth.size + 9)])   # nothing left after clipping
        empty = [k for k, _ in hot.kernel_times()]
    finally:
        hot.set_timing(False)
    assert "exclude_mask" not in plain and "fasta_classify" in plain
    assert with_mask.count("exclude_mask") == 1
    assert with_mask.index("exclude_mask") == with_mask.index("fasta_classify") + 1
    assert "exclude_mask" not in empty


# ---- the command line ---------------------------------------------------------------------------------------------------

def write_bed(path, chrom_masks, extra_lines=()):
    with open(path, "w") as f:
        f.write("track name=exclude\n# regions left out of calling\n\n")
        for chrom, mask in chrom_masks:
            for s, e in mask:
                f.write(f"{chrom}\t{max(s, 0)}\t{e}\tx\n")
        for l in extra_lines:
            f.write(l + "\n")


def cli(args, timeout=600, **kw):
    return subprocess.run([EXE, "rsi"] + args, capture_output=True, text=True, timeout=timeout, **kw)


@pytest.mark.parametrize("extra", [[], ["-NOGC"]], ids=["nb", "nogc"])
def test_cli_single_chromosome_equals_reference_on_masked_fasta(tmp_path, extra):
    import oracle
    from rsicnv_amd import api
    from test_hot_extra import _write_case
    if not os.path.exists(oracle.REF_BIN):
        pytest.skip("oracle/_ref/rsicnv_ref not built")
    plan, fasta, depth = make_case(api.load_library(), dict(n=400_007, seed=0xC11, model=1, n_events=5, gaps=1, max_len=20000, end_n=5000, gap_len=8000))
    mask = path_mask(plan, "wide")
    (tmp_path / "masked").mkdir()
    fa, rd = _write_case(str(tmp_path), fasta, depth)
    fa_masked, _ = _write_case(str(tmp_path / "masked"), masked(fasta, mask), depth[:10])
    bed = str(tmp_path / "mask.bed")
    write_bed(bed, [("chrS", mask[::-1])], extra_lines=["chrOther\t5\t50000"])
    ours, theirs = str(tmp_path / "ours.txt"), str(tmp_path / "ref.txt")
    r = cli(["-f", fa, "-d", rd, "-c", "chrS", "-x", bed, "-o", ours, "-np"] + extra)
    assert r.returncode == 0 and os.path.exists(ours), r.stderr[-2000:]
    subprocess.run([oracle.REF_BIN, "rsi", "-f", fa_masked, "-d", rd, "-c", "chrS", "-o", theirs, "-np"] + extra, check=True,
                   capture_output=True, timeout=600, cwd=str(tmp_path))
    a, b = open(ours, "rb").read(), open(theirs, "rb").read()
    assert a == b, f"output files differ:\n{a.decode()}\n---\n{b.decode()}"
    assert a.count(b"\n") >= 4
    sweep = lambda path: [l for l in open(path + ".log").read().splitlines() if l.startswith(("DEL-\t", "DUP+\t"))]
    la, lb = sweep(ours), sweep(theirs)
    assert la == lb and len(la) >= 4 * 20
    nmask = len(api.read_exclude_bed(bed, "chrS", fasta.size))
    nbases = int((masked(np.zeros(fasta.size, dtype=np.uint8), mask) == ord("N")).sum())
    assert f"#exclude: {bed}, {nmask} intervals, {nbases} bases on chrS\n" in open(ours + ".log").read()
    # without -x the log has no such line
    plain = str(tmp_path / "plain.txt")
    assert cli(["-f", fa, "-d", rd, "-c", "chrS", "-o", plain, "-np"] + extra).returncode == 0
    assert "#exclude" not in open(plain + ".log").read() and open(plain, "rb").read() != a


# lines that name the run itself (its command, files and times), not what it computed
RUN_LINES = ("#command:", "#reffile:", "#exclude:", "#output:", "timing:", "output written to", "#depth file:")


def log_of(path):
    return [l for l in open(path + ".log").read().splitlines() if not l.startswith(RUN_LINES)]


@pytest.fixture(scope="module")
def genome_files(tmp_path_factory):
    """Two chromosomes as a whole-genome depth file, a two-sample cohort file and a bedGraph; the FASTA, and the FASTA with the
    mask's bases of chrP as N; a BED file that names chrP (without its prefix), and a chromosome that is in neither."""
    from rsicnv_amd import api
    from test_genome_text import write_fasta
    lib = api.load_library()
    lib.rsi_synth_append_genome_text.argtypes = [C.c_char_p, C.c_char_p, C.c_void_p, C.c_int64]
    tmp = str(tmp_path_factory.mktemp("exclude_cli"))
    specs = [("chrP", dict(n=400_007, seed=0xC21, model=1, n_events=5, gaps=1, max_len=20000, end_n=5000, gap_len=8000)),
             ("chrQ", dict(n=300_001, seed=0xC23, model=1, n_events=4, gaps=0, max_len=15000, end_n=4000))]
    text, cohort, bg = (os.path.join(tmp, f) for f in ("g.depth", "cohort.depth", "g.bedgraph"))
    seqs, seqs_masked, mask = [], [], None
    for name, kw in specs:
        plan, fasta, d = make_case(lib, kw)
        d = np.ascontiguousarray(d, dtype=np.int32)
        if name == "chrP":
            mask = path_mask(plan, "wide")
        seqs.append((name, fasta))
        seqs_masked.append((name, masked(fasta, mask) if name == "chrP" else fasta))
        two = np.ascontiguousarray(np.stack([d, (d * 3) // 2]), dtype=np.int32)
        assert lib.rsi_synth_append_genome_text(text.encode(), name.encode(), d.ctypes.data, d.size) == 0
        assert lib.rsi_synth_append_genome_samples(cohort.encode(), name.encode(), two.ctypes.data, 2, d.size, 0) == 0
        assert lib.rsi_synth_append_genome_bedgraph(bg.encode(), name.encode(), d.ctypes.data, d.size, 0) == 0
    fa, fa_masked = os.path.join(tmp, "ref.fa"), os.path.join(tmp, "ref_masked.fa")
    write_fasta(fa, seqs)
    write_fasta(fa_masked, seqs_masked)
    bed = os.path.join(tmp, "mask.bed")
    write_bed(bed, [("P", mask)], extra_lines=["chrZ\t100\t90000", "chrZ 5 6"])
    return tmp, fa, fa_masked, bed, text, cohort, bg


@pytest.mark.parametrize("mode", ["genome", "samples", "bedgraph"])
def test_cli_genome_modes_equal_runs_on_the_masked_fasta(genome_files, mode):
    tmp, fa, fa_masked, bed, text, cohort, bg = genome_files
    depth_file, args = {"genome": (text, []), "samples": (cohort, ["-samples", "all"]), "bedgraph": (bg, [])}[mode]
    ours, own = os.path.join(tmp, f"{mode}_x.txt"), os.path.join(tmp, f"{mode}_masked.txt")
    r = cli(["-f", fa, "-d", depth_file, "-x", bed, "-o", ours, "-np"] + args)
    assert r.returncode == 0, r.stderr[-3000:]
    r = cli(["-f", fa_masked, "-d", depth_file, "-o", own, "-np"] + args)
    assert r.returncode == 0, r.stderr[-3000:]
    for suffix in ([".1", ".2"] if mode == "samples" else [""]):
        a, b = open(ours + suffix, "rb").read(), open(own + suffix, "rb").read()
        assert a == b and a.count(b"\n") >= 4, f"{mode}{suffix}:\n{a.decode()}\n---\n{b.decode()}"
        assert log_of(ours + suffix) == log_of(own + suffix)
        log = open(ours + suffix + ".log").read()
        assert f"#exclude: {bed}, 4 intervals, " in log and " bases on chrP\n" in log
        assert f"#exclude: {bed}, 0 intervals, 0 bases on chrQ\n" in log and "chrZ" not in log
        assert "#exclude" not in open(own + suffix + ".log").read()


def test_cli_bam_modes_equal_runs_on_the_masked_fasta(tmp_path):
    import bam_util as bu
    from test_genome_text import write_fasta
    bam, refs, _ = bu.build_golden_bam(str(tmp_path))
    rng = np.random.default_rng(0xBA)
    seqs = [(name, rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=n)) for name, n in refs]
    mask = [(30_000, 41_000), (100_000, 100_700), (199_000, 200_003)]
    fa, fa_masked, bed = str(tmp_path / "ref.fa"), str(tmp_path / "ref_masked.fa"), str(tmp_path / "mask.bed")
    write_fasta(fa, seqs)
    write_fasta(fa_masked, [(name, masked(s, mask) if name == "chrS" else s) for name, s in seqs])
    write_bed(bed, [("chrS", mask)])
    for tag, args in (("all", []), ("one", ["-c", "chrS"]), ("pool", ["-gpus", "1", "-workers", "2"])):
        ours, own = str(tmp_path / f"{tag}_x.txt"), str(tmp_path / f"{tag}_masked.txt")
        r = cli(["-b", bam, "-f", fa, "-x", bed, "-o", ours, "-np"] + args)
        assert r.returncode == 0, r.stderr[-3000:]
        r = cli(["-b", bam, "-f", fa_masked, "-o", own, "-np"] + args)
        assert r.returncode == 0, r.stderr[-3000:]
        a, b = open(ours, "rb").read(), open(own, "rb").read()
        assert a == b and a.count(b"\n") >= 2, f"{tag}:\n{a.decode()}\n---\n{b.decode()}"
        assert log_of(ours) == log_of(own)
        log = open(ours + ".log").read()
        assert f"#exclude: {bed}, 3 intervals, {11_000 + 700 + 1003} bases on chrS\n" in log
        # the mask's regions are among the chromosome's removed ones
        assert "chrS\t29950\t41049\n" in log and "chrS\t29950\t41049\n" in open(own + ".log").read()


def test_cli_broken_bed_leaves_no_output(genome_files, tmp_path):
    tmp, fa, fa_masked, bed, text, cohort, bg = genome_files
    broken = str(tmp_path / "broken.bed")
    with open(broken, "w") as f:
        f.write("chrP\t100\t200\nchrZ\t300\n")   # the bad line names a chromosome that is not processed: an error all the same
    for args in (["-d", text], ["-d", text, "-c", "chrP"], ["-d", cohort, "-samples", "all"]):
        out = str(tmp_path / "out.txt")
        r = cli(["-f", fa, "-x", broken, "-o", out, "-np"] + args)
        assert r.returncode == 1, r.stderr[-2000:]
        assert "line 2" in r.stderr and "broken.bed" in r.stderr
        assert not [f for f in os.listdir(str(tmp_path)) if f.startswith("out.txt") and not f.endswith(".log")]


def test_exclude_in_the_usage():
    u = subprocess.run([EXE], capture_output=True, text=True)
    assert "-x   FILE" in u.stderr and "4096" in u.stderr
