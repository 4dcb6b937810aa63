"""The depth-text readers' integer extraction against the reference's own: load_data_from_text's `iss >> pos >> d` with
libstdc++ (rsicnv_amd/csrc/text_rules.h).

CPU: the restatement in tests/text_rules.py equals the reference's stored answers on a corpus of awkward lines (and the
compiled reference itself when oracle/_ref/libref.so is built); text_rules.h, built as host C++ under ASan + UBSan, equals
std::istringstream on the corpus and on a million random lines, and so does the restatement.
GPU: every reader -- the single-chromosome text reader (plain, gzip, BGZF), the genome reader, the cohort reader and the
bedGraph reader -- equals the restatement on files of about a megabase with the quirk lines on 4097-byte chunk boundaries,
on the device path and, with one repeated position, on the host fallback."""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import bgzf_util as bz
import text_rules as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "text_rules.npz")
HARNESS = os.path.join(ROOT, "tests", "sanitize_text", "text_harness")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
STATS = ("lines", "stored", "beyond", "fallback")
N_GOLDEN = 3001


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the stored reference answers
# ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize("case", list(tr.CASES))
def test_restatement_equals_reference_answers(golden, case):
    b = tr.case_bytes(case, N_GOLDEN)
    assert str(golden[f"sha_{case}"]) == tr.text_hash(b), "the corpus changed: rerun tools/make_golden_text_rules.py"
    rd, _ = tr.load_text(b.decode("latin-1"), N_GOLDEN)
    ref = golden[f"rd_{case}"]
    assert ref.dtype == np.int32 and ref.size == N_GOLDEN
    bad = np.nonzero(rd != ref)[0]
    assert bad.size == 0, (case, bad[:10].tolist(), rd[bad[:5]].tolist(), ref[bad[:5]].tolist())


def test_reference_answers_hold_the_clamps(golden):
    """The answers that distinguish the reference's extraction from a wrapping one are in the stored data."""
    a = N_GOLDEN // 3
    d = golden["rd_d_bounds"]
    assert d[a - 1:a - 1 + 37 * 11:37].tolist() == [2147483647, 2147483647, 2147483647, 2147483647, -2147483648,
                                                    -2147483648, -2147483648, 17, 2147483647, 2147483647, 2147483647]
    for case in ("pos_2e31", "pos_int_max", "pos_2e64p1", "pos_1e22"):   # the read ends at the overflowing line
        r = golden[f"rd_{case}"]
        assert np.all(r[a - 1:] == 0) and np.count_nonzero(r[:a - 1]) > 0.9 * (a - 1), case
    assert golden["rd_pos_2e64p1"][0] == 7919 % 97                        # a wrapped position would have stored 5 there
    assert np.count_nonzero(golden["rd_pos_neg"][a:]) > 0.9 * (N_GOLDEN - a - 2)   # -inf positions are skipped, the read goes on


@pytest.mark.skipif(not os.path.exists(os.path.join(ROOT, "oracle", "_ref", "libref.so")), reason="oracle/_ref/libref.so not built")
def test_live_reference_matches_golden_answers(golden, tmp_path):
    import importlib.util
    import sys
    sys.path.insert(0, ROOT)
    import oracle
    spec = importlib.util.spec_from_file_location("make_golden_text_rules", os.path.join(ROOT, "tools", "make_golden_text_rules.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    ref = oracle.Ref()
    if not ref.has_load_text():
        pytest.skip("oracle/_ref/libref.so was built before ref_load_text existed (no reference sources to rebuild it)")
    got = mk.reference_answers(ref, str(tmp_path))
    for case in tr.CASES:
        assert str(got[f"sha_{case}"]) == str(golden[f"sha_{case}"]), case
        assert np.array_equal(got[f"rd_{case}"], golden[f"rd_{case}"]), case


# ---------------------------------------------------------------------------------------------------------------------
# CPU: text_rules.h under ASan + UBSan against std::istringstream, and the restatement against the same runs
# ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    tmp = tmp_path_factory.mktemp("probe")
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", str(tmp / "probe")], input=b"int main(){return 0;}",
                           capture_output=True)
    if probe.returncode != 0:
        pytest.skip("g++ cannot link the sanitizer runtimes here")
    r = subprocess.run(["make", "-f", "tests/sanitize_text/Makefile"], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return HARNESS


def _clean(r):
    return "Sanitizer" not in r.stderr and "runtime error" not in r.stderr


def _python_values(line):
    ints, _ = tr.chain(line, 9)
    ok, a, q = tr.extract(line, 0, 64)
    b = d = 0
    if ok:
        ok, b, q = tr.extract(line, q, 64)
        if ok:
            _, d, _ = tr.extract(line, q)
    return ints + [a, b, d]


def _check(harness, lines_path, vals_path, sample=None):
    r = subprocess.run([harness, "check", str(lines_path), str(vals_path)], capture_output=True, text=True, env=ENV, timeout=550)
    assert r.returncode == 0 and "check ok" in r.stdout and _clean(r), r.stdout[-2000:] + r.stderr[-3000:]
    lines = open(lines_path, "rb").read().decode("latin-1").split("\n")[:-1]
    vals = np.loadtxt(vals_path, dtype=np.int64, delimiter="\t", ndmin=2)
    assert vals.shape == (len(lines), 12)
    idx = range(len(lines)) if sample is None else sample
    for i in idx:
        assert _python_values(lines[i]) == vals[i].tolist(), (i, repr(lines[i]), vals[i].tolist())
    return r.stdout, vals


@pytest.mark.timeout(300)
def test_extraction_equals_istringstream_on_the_corpus(harness, tmp_path):
    lines = []
    for case in tr.CASES:
        lines += tr.case_text(case, N_GOLDEN).split("\n")
        lines += [t.replace("{P}", "77") for t in tr.CASES[case]]
    p = tmp_path / "corpus.txt"
    p.write_bytes(("\n".join(lines) + "\n").encode("latin-1"))
    _check(harness, p, tmp_path / "corpus.vals")


@pytest.mark.timeout(900)
def test_extraction_equals_istringstream_on_random_lines(harness, tmp_path):
    """A million random lines: signs, blanks, digit runs of 1-25 characters, boundary values and junk, read as int chains of
    up to 9 (pos and 8 cohort columns) and as bedGraph's long long, long long, int."""
    p = tmp_path / "random.txt"
    r = subprocess.run([harness, "gen", "20261016", "1000000", str(p)], capture_output=True, text=True, env=ENV, timeout=300)
    assert r.returncode == 0 and _clean(r), r.stderr[-2000:]
    out, vals = _check(harness, p, tmp_path / "random.vals", sample=range(0, 1000000, 5))
    # the input reaches every kind of answer: clamps of both signs and widths, failed and later columns
    for v in (2147483647, -2147483648, 9223372036854775807, -9223372036854775808, 0):
        assert (vals == v).any(), v
    assert (vals[:, 8] != 0).sum() > 1000 and (vals[:, 11] != 0).sum() > 1000


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the restatement's own rules
# ---------------------------------------------------------------------------------------------------------------------

def test_restatement_rules():
    assert tr.per_base("5\t3000000000") == (5, 2147483647) and tr.per_base("5\t-3000000000") == (5, -2147483648)
    assert tr.per_base("18446744073709551617\t5") == (2147483647, 0) and tr.per_base("-9223372036854775809\t5") == (-2147483648, 0)
    assert tr.per_base("5abc 3") == (5, 0) and tr.per_base("5.7\t3") == (5, 0) and tr.per_base("+5 +3") == (5, 3)
    assert tr.columns("7 1 99999999999 4", 3) == (7, [1, 2147483647, 0])
    assert tr.columns("7 99999999999 1 4", 3) == (7, [2147483647, 0, 0])
    assert tr.bed_fields("0\t3\t3000000000") == (0, 3, 2147483647)
    assert tr.bed_fields("0\t9223372036854775808\t1") is None and tr.bed_fields("-9223372036854775809 3 1") is None
    items = tr.items_of(["1 5", "3 6", "2 7", "9 9"])
    rd, st = tr.restate(items, 5)
    assert rd[0].tolist() == [5, 7, 6, 0, 0] and st == dict(lines=4, stored=3, beyond=1, fallback=1)
    rd, st = tr.restate(tr.items_of(["1 5", "4 6", "5 7", "9 9"]), 5)
    assert rd[0].tolist() == [5, 0, 0, 6, 0] and st == dict(lines=4, stored=2, beyond=2, fallback=0)


# ---------------------------------------------------------------------------------------------------------------------
# GPU: the readers against the restatement
# ---------------------------------------------------------------------------------------------------------------------

NOT_STOPPING = tr.CASES["d_bounds"] + tr.CASES["pos_neg"] + tr.CASES["tokens"] + tr.CASES["blanks"]
STOPPERS = ["pos_2e31", "pos_int_max", "pos_2e64p1", "pos_1e22"]
N_BIG = 1_000_003
HEAD = "# text_rules: quirk lines on chunk boundaries\n"


@functools.lru_cache(maxsize=1)
def _per_base_variants(n):
    """{tag: (text, depth, stats)} of single-chromosome files: all quirks (device path), each stopper halfway, a stopper as the last line
    (device path, one more beyond), all quirks with one repeated position (host fallback)."""
    rows = tr.per_base_rows(n)
    out = {"quirks": HEAD + "\n".join(tr.embed(rows, NOT_STOPPING, offset=len(HEAD))) + "\n"}
    for case in STOPPERS:
        out[case] = HEAD + "\n".join(tr.embed(rows, tr.CASES[case], offset=len(HEAD), first=n // 2)) + "\n"
    out["stop_last"] = HEAD + "\n".join(t for t, _ in rows) + "\n18446744073709551617\t5\n"
    lines = tr.embed(rows, NOT_STOPPING, offset=len(HEAD))
    lines.insert(len(lines) * 2 // 3, lines[len(lines) // 3])
    out["quirks_repeat"] = HEAD + "\n".join(lines) + "\n"
    return {tag: (text, *tr.load_text(text, n)) for tag, text in out.items()}


@pytest.fixture(scope="module")
def hot():
    from rsicnv_amd import api
    h = api.RsiHot(0)
    yield h
    h.close()


def _check_stats(st, exp, tag):
    for k in STATS:
        assert st[k] == exp[k], (tag, k, st[k], exp[k])


@pytest.mark.gpu
@pytest.mark.timeout(900)
@pytest.mark.parametrize("form", ["text", "gzip", "bgzf"])
def test_text_rules_single_chromosome_reader(hot, tmp_path, form):
    for tag, (text, exp, est) in _per_base_variants(N_BIG).items():
        raw = text.encode("latin-1")
        data = raw if form == "text" else (bz.gzip_members(raw, parts=2) if form == "gzip" else bz.bgzf(raw))
        p = tmp_path / f"{tag}.depth"
        p.write_bytes(data)
        st = hot.load_depth_text(str(p), N_BIG)
        got = hot.fetch("depth_in")
        bad = np.nonzero(got != exp)[0]
        assert bad.size == 0, (form, tag, bad[:8].tolist(), got[bad[:4]].tolist(), exp[bad[:4]].tolist())
        _check_stats(st, est, (form, tag))
        assert est["fallback"] == (1 if tag in STOPPERS or tag == "quirks_repeat" else 0), (tag, est)


def _genome_text(n, k=None, repeat_in=None):
    """Three chromosomes: chrA with every non-stopping quirk, chrB with the 2^64+1 position halfway, chrC with the
    d bounds (and, for repeat_in, one repeated position in that chromosome)."""
    parts, off = [HEAD], len(HEAD)
    plan = [("chrA", NOT_STOPPING, n // 8), ("chrB", tr.CASES["pos_2e64p1"], n // 2), ("chrC", tr.CASES["d_bounds"], n // 8)]
    for name, tmpl, first in plan:
        lines = tr.embed(tr.per_base_rows(n, k=k), tmpl, prefix=f"{name}\t", offset=off, first=first)
        if name == repeat_in:
            lines.insert(len(lines) * 2 // 3, lines[len(lines) // 3])
        s = "\n".join(lines) + "\n"
        parts.append(s)
        off += len(s)
    return "".join(parts)


def _genome_names(n):
    return ["chrA", "chrB", "chrC"], [n, n + 10, n - 7]


@pytest.mark.gpu
@pytest.mark.timeout(900)
@pytest.mark.parametrize("chunk", [0, 4097])
def test_text_rules_genome_reader(tmp_path, chunk):
    from rsicnv_amd import api
    n = 300_007
    names, lens = _genome_names(n)
    for repeat_in in (None, "chrC"):
        text = _genome_text(n, repeat_in=repeat_in)
        p = tmp_path / "genome.depth"
        p.write_bytes(text.encode("latin-1"))
        exp = tr.load_named(text, dict(zip(names, lens)))
        seen = []
        with api.GenomeText(str(p), names, lens, chunk_bytes=chunk, max_resident=2) as g:
            for name, ptr, m, st in g:
                seen.append(name)
                got = g.depth(st["slot"])
                rd, est = exp[name]
                bad = np.nonzero(got != rd[0])[0]
                assert bad.size == 0, (chunk, repeat_in, name, bad[:8].tolist(), got[bad[:4]].tolist(), rd[0][bad[:4]].tolist())
                _check_stats(st, est, (chunk, repeat_in, name))
                assert est["fallback"] == (1 if name == "chrB" or name == repeat_in else 0)
        assert seen == names


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_text_rules_cohort_reader(tmp_path):
    """Overflows in column k itself give the clamp; in a column before k (or in pos) they leave column k at 0."""
    from rsicnv_amd import api
    n, K = 200_003, 4
    names, lens = _genome_names(n)
    col_quirks = ["{P}\t1\t3000000000\t7\t8", "{P}\t99999999999\t2\t3\t4", "{P}\t1\t2\t3\t-99999999999999999999",
                  "{P}\t1\t2\t3x\t4", "{P}\t-2147483649\t5\t6\t7", "{P} +-1 2 3 4", "{P}\t1\t2\t3"]
    samples = [4, 2, 1, 3]
    for repeat_in in (None, "chrA"):
        parts, off = [HEAD], len(HEAD)
        for name, tmpl, first in (("chrA", col_quirks + NOT_STOPPING, n // 8), ("chrB", tr.CASES["pos_2e64p1"], n // 2),
                                  ("chrC", col_quirks, n // 4)):
            lines = tr.embed(tr.per_base_rows(n, k=K), tmpl, prefix=f"{name}\t", offset=off, first=first)
            if name == repeat_in:
                lines.insert(len(lines) * 2 // 3, lines[len(lines) // 3])
            s = "\n".join(lines) + "\n"
            parts.append(s)
            off += len(s)
        text = "".join(parts)
        p = tmp_path / "cohort.depth"
        p.write_bytes(text.encode("latin-1"))
        exp = tr.load_named(text, dict(zip(names, lens)), form="samples", k=K)
        with api.GenomeText(str(p), names, lens, samples=samples, chunk_bytes=4097, max_resident=2) as g:
            for name, ptr, m, st in g:
                rd, est = exp[name]
                for j, k in enumerate(samples):
                    got = g.sample_depth(st["slot"], j)
                    bad = np.nonzero(got != rd[k - 1])[0]
                    assert bad.size == 0, (repeat_in, name, k, bad[:8].tolist(), got[bad[:4]].tolist(), rd[k - 1][bad[:4]].tolist())
                _check_stats(st, est, (repeat_in, name))
                assert est["fallback"] == (1 if name == "chrB" or name == repeat_in else 0)
        if repeat_in is None:   # the quirks landed: clamps in column 2 and 4, zeros behind a failed column
            a = exp["chrA"][0]
            assert (a[1] == 2147483647).any() and (a[3] == -2147483648).any() and (a[0] == 2147483647).any()


BED_QUIRKS = ["{S}\t{E}\t3000000000", "{S}\t{E}\t-2147483649", "{S}\t{E}\t99999999999999999999", "{S}\t99999999999999999999\t5",
              "99999999999999999999\t{E}\t5", "-9223372036854775809\t{E}\t5", "{S}\t-9223372036854775809\t5", "{S}\t{E}\t12abc",
              "{S}.5\t{E}\t6", "{S}\t{E}\t+-3", " {S} \v{E}\f\f13", "{S}\t{E}", "{S}\t{E}\t000000000000000000042"]


@pytest.mark.gpu
@pytest.mark.timeout(900)
@pytest.mark.parametrize("zero_runs", [True, False], ids=["bga", "bg"])
def test_text_rules_bedgraph_reader(tmp_path, zero_runs):
    """d, start and end overflows; an end of 2^63 - 1 (a valid long long) ends the read at n; -bga and -bg forms."""
    from rsicnv_amd import api
    n = 300_007
    names, lens = _genome_names(n)
    for repeat_in in (None, "chrC"):
        parts, off = [HEAD, "track type=bedGraph\n"], len(HEAD) + 20
        for i, (name, tmpl, first) in enumerate((("chrA", BED_QUIRKS, 1000), ("chrB", ["{S}\t9223372036854775807\t5"], 30000),
                                                 ("chrC", BED_QUIRKS[:6], 20000))):
            lines = tr.embed(tr.bed_rows(n + (0, 10, -7)[i], 11 + i, zero_runs), tmpl, prefix=f"{name}\t", offset=off, first=first)
            if name == repeat_in:
                lines.insert(len(lines) * 2 // 3, lines[len(lines) // 3])
            s = "\n".join(lines) + "\n"
            parts.append(s)
            off += len(s)
        text = "".join(parts)
        p = tmp_path / "depth.bedgraph"
        p.write_bytes(text.encode("latin-1"))
        exp = tr.load_named(text, dict(zip(names, lens)), form="bedgraph")
        for chunk in (0, 4097):
            with api.GenomeText(str(p), names, lens, bedgraph=True, chunk_bytes=chunk, max_resident=2) as g:
                for name, ptr, m, st in g:
                    got = g.depth(st["slot"])
                    rd, est = exp[name]
                    bad = np.nonzero(got != rd[0])[0]
                    assert bad.size == 0, (chunk, repeat_in, name, bad[:8].tolist(), got[bad[:4]].tolist(), rd[0][bad[:4]].tolist())
                    _check_stats(st, est, (chunk, repeat_in, name))
                    assert est["fallback"] == (1 if name == "chrB" or name == repeat_in else 0)
        if repeat_in is None:
            assert (exp["chrA"][0][0] == 2147483647).any() and (exp["chrA"][0][0] == -2147483648).any()


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_text_rules_cli_matches_reference_binary(hotlib, tmp_path):
    """`rsicnv rsi -d FILE -c chrS` on a file with a 2^64 + 1 position halfway: the reference stops reading there."""
    import oracle
    from conftest import make_case
    from test_hot_extra import _write_case
    if not os.path.exists(oracle.REF_BIN):
        pytest.skip("oracle/_ref/rsicnv_ref not built")
    _, fasta, depth = make_case(hotlib, dict(n=400_007, seed=0xC13, model=1, n_events=5, gaps=1, max_len=20000, end_n=5000, gap_len=8000))
    fa, rd = _write_case(str(tmp_path), fasta, depth)
    lines = open(rd).read().split("\n")
    lines.insert(len(lines) // 2, "18446744073709551617\t5")
    open(rd, "w").write("\n".join(lines))
    ours, theirs = str(tmp_path / "ours.txt"), str(tmp_path / "ref.txt")
    exe = os.path.join(ROOT, "rsicnv_amd", "bin", "rsicnv")
    subprocess.run([exe, "rsi", "-f", fa, "-d", rd, "-c", "chrS", "-o", ours, "-np"], check=True, capture_output=True, timeout=300)
    subprocess.run([oracle.REF_BIN, "rsi", "-f", fa, "-d", rd, "-c", "chrS", "-o", theirs, "-np"], check=True,
                   capture_output=True, timeout=600, cwd=str(tmp_path))
    a, b = open(ours, "rb").read(), open(theirs, "rb").read()
    assert a == b, f"output files differ:\n{a.decode()}\n---\n{b.decode()}"
    assert a.count(b"\n") >= 2
