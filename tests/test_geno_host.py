"""CPU: `rsicnv geno` stated three times agrees -- the compiled reference's _median and _interquartilerange of every
range of every case that it can be asked (tests/golden/geno_edges.npz), the Python restatement of geno_cases.py, and
rsicnv_amd/csrc/geno_host.h in a stand-alone program under ASan + UBSan (tests/geno_harness.cpp): the mapping through the removed
regions, the flanks, the tile tables, the ranks and the formatted field."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import geno_cases as gc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
CASES = gc.cases()


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "geno_edges.npz"))


def test_restatement_equals_the_reference(golden):
    """med and uqt - lqt of every stored range; the cases without golden values are exactly the wide-span ones."""
    stored = {k[:-4] for k in golden.files if k.endswith(".med")}
    assert set(CASES) - stored == set(gc.WIDE_SPAN) and stored <= set(CASES)
    assert {name for name, c in CASES.items() if gc.is_wide(c)} == set(gc.WIDE_SPAN)
    checked = 0
    for name in sorted(stored):
        vals = gc.golden_ranges(CASES[name])
        med, iqr = golden[name + ".med"], golden[name + ".iqr"]
        assert len(vals) == med.size == iqr.size == 2 * len(CASES[name].jobs), name
        for k, v in enumerate(vals):
            if v is None:
                assert np.isnan(med[k]) and np.isnan(iqr[k]), (name, k)
                continue
            q = gc.quantiles(v)
            assert (q[1], q[2] - q[0]) == (med[k], iqr[k]), (name, k, q, med[k], iqr[k], sorted(v.tolist())[:12])
            checked += 1
    assert checked > 6000


def test_cases_are_what_they_say():
    assert [gc.ranks(n) for n in (1, 2, 3, 4, 5, 7, 8)] == [[0, 0, 0], [0, 0, 0], [0, 0, 1], [0, 1, 2], [0, 1, 2], [0, 2, 4], [1, 3, 5]]
    assert gc.quantiles([9]) == [9, 9, 9] and gc.quantiles([7, 3]) == [3, 3, 3] and gc.quantiles([5, 1, 3]) == [1, 1, 3]
    lens = {j[1] - j[0] for j in CASES["short_lengths"].jobs}
    assert lens == {1, 2, 3, 4, 5, 7, 8}
    t = CASES["ties_on_ranks"]
    q = [gc.quantiles(t.depth[j[0]:j[1]]) for j in t.jobs[:7]]
    assert q[0] == [5, 9, 9] and q[1] == [9, 9, 9] and q[2] == [5, 5, 9] and q[3] == [5, 9, 9] and q[4] == [5, 5, 5] and q[5] == [5, 5, 9]
    assert {j[1] - j[0] for j in CASES["tile_seams"].jobs} >= {gc.TILE - 1, gc.TILE, gc.TILE + 1}
    assert CASES["short_lengths"].depth.max() == 255 and any(255 in CASES["short_lengths"].depth[j[0]:j[1]] for j in CASES["short_lengths"].jobs)
    assert len(CASES["no_jobs"].jobs) == 0 and len(CASES["one_job"].jobs) == 1 and len(CASES["batch_3000"].jobs) == 3000
    e = CASES["empty_flanks"].jobs
    assert e[0][2] == e[0][3] and e[1][4] == e[1][5] and e[2][2] == e[2][3] and e[2][4] == e[2][5] and e[3][0] == e[3][1]
    w = CASES["span_0_and_2p30"].depth
    assert w.min() == 0 and w.max() == (1 << 31) - 1 and {0, 65535, 65536} <= set(CASES["around_65536"].depth.tolist())
    b = CASES["band_at_2p30"].depth
    assert b.min() > (1 << 30) - 1000 and b.max() < (1 << 30) + 1000
    for name, start, end, expect in gc.MAP_CASES:
        assert gc.map_line(start, end, gc.MAP_N, gc.MAP_PAIRS) == expect, name
    # the mapping is the inverse of re-inserting the regions: every kept base maps to its index among the kept ones
    kept = [x for x in range(gc.MAP_N) if not any(s <= x <= e for s, e in gc.MAP_PAIRS)]
    for i in (0, 99, 100, 199, 200, 849):
        assert gc.map_line(kept[i] + 1, kept[i] + 1, gc.MAP_N, gc.MAP_PAIRS) == (i, i + 1)
    assert gc.line_job(10, 20, 101, 850) == (10, 20, 0, 10, 20, 121) and gc.line_job(400, 800, 101, 850) == (400, 800, 0, 400, 800, 850)
    assert gc.line_job(0, 850, 5, 850) == (0, 850, 0, 0, 850, 850) and gc.line_job(100, 100, 7, 850) == (100, 100, 93, 100, 100, 107)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    tmp = tmp_path_factory.mktemp("geno_harness")
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", str(tmp / "probe")], input=b"int main(){return 0;}",
                           capture_output=True)
    if probe.returncode != 0:
        pytest.skip("g++ cannot link the sanitizer runtimes here")
    exe = str(tmp / "geno_harness")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                        os.path.join(ROOT, "tests", "geno_harness.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def run_jobs(exe, tmp, lines):
    job = os.path.join(str(tmp), "jobs.txt")
    open(job, "w").write("\n".join(lines) + "\n")
    r = subprocess.run([exe, job], capture_output=True, text=True, env=ENV, timeout=600)
    assert r.returncode == 0 and "error" not in r.stdout and not r.stderr, r.stdout[-1500:] + r.stderr[-3000:]
    blocks = []
    for ln in r.stdout.splitlines():
        if ln.startswith("job "):
            blocks.append([])
        else:
            blocks[-1].append(ln)
    assert len(blocks) == len(lines)
    return blocks


def test_header_mapping_and_flanks(harness, tmp_path):
    flat = " ".join(f"{s} {e}" for s, e in gc.MAP_PAIRS)
    rng = np.random.default_rng(5)
    lines_in = [(c[1], c[2]) for c in gc.MAP_CASES] + [tuple(int(v) for v in rng.integers(-20, gc.MAP_N + 40, 2)) for _ in range(400)]
    jobs = [f"M {gc.MAP_N} {len(gc.MAP_PAIRS)} {flat} {s} {e}" for s, e in lines_in]
    jobs += [f"M {gc.MAP_N} 0 {s} {e}" for s, e in lines_in[:20]]                  # no removed region at all
    got = run_jobs(harness, tmp_path, jobs)
    for (s, e), b in zip(lines_in, got):
        assert tuple(int(v) for v in b[0].split()) == gc.map_line(s, e, gc.MAP_N, gc.MAP_PAIRS), (s, e)
    for (s, e), b in zip(lines_in[:20], got[len(lines_in):]):
        assert tuple(int(v) for v in b[0].split()) == gc.map_line(s, e, gc.MAP_N, []), (s, e)
    spans = [(0, 0), (0, 1), (0, 850), (849, 850), (100, 100), (10, 20), (400, 800), (840, 845), (3, 9)]
    ms = (1, 5, 101, 2000)
    got = run_jobs(harness, tmp_path, [f"L {a} {b} {m} 850" for a, b in spans for m in ms])
    want = [gc.line_job(a, b, m, 850) for a, b in spans for m in ms]
    assert [tuple(int(v) for v in b[0].split()) for b in got] == want


def test_header_tiles_ranks_and_field(harness, tmp_path):
    names = [n for n in CASES if n not in ("batch_3000", "batch_wide_3000")]
    jobs = []
    for name in names:
        c = CASES[name]
        for tile in (gc.TILE, 16384, 1):
            if tile == 1 and c.depth.size > 700:
                continue
            jobs.append((name, tile))
    text = [f"T {tile} {CASES[n].depth.size} {len(CASES[n].jobs)} " + " ".join(" ".join(str(v) for v in j) for j in CASES[n].jobs) for n, tile in jobs]
    text += ["T 256 100 1 0 101 0 0 101 101", "T 256 100 1 10 5 0 0 5 5", "T 0 100 1 0 10 0 0 10 10", "T 256 100 1 -1 10 0 0 10 10"]
    got = run_jobs(harness, tmp_path, text)
    for (name, tile), b in zip(jobs, got):
        assert b[0] == "ok", (name, tile)
        tiles = [tuple(int(v) for v in ln.split()) for ln in b[1:]]
        assert tiles == gc.tiles_of(CASES[name].jobs, tile), (name, tile)
        assert all(0 < t[2] <= tile for t in tiles)
    assert [b[0] for b in got[len(jobs):]] == ["bad"] * 4
    ns = list(range(1, 40)) + [255, 256, 257, (1 << 31) - 5000]
    got = run_jobs(harness, tmp_path, [f"R {n}" for n in ns])
    assert [[int(v) - 1 for v in b[0].split()] for b in got] == [gc.ranks(n) for n in ns]
    recs = [(dict(n_body=10, n_flank=20, body_q=[1, 15, 30], flank_q=[2, 31, 40]), 30.0, 2.0),
            (dict(n_body=0, n_flank=20, body_q=[0, 0, 0], flank_q=[2, 31, 40]), 30.5, 2.0),
            (dict(n_body=7, n_flank=0, body_q=[0, 0, 0], flank_q=[0, 0, 0]), 29.0, 2.0),
            (dict(n_body=1234567, n_flank=5, body_q=[1, 45, 30], flank_q=[2, 1000000, 40]), 30.0, 1.0),
            (dict(n_body=3, n_flank=3, body_q=[1, 120, 30], flank_q=[2, 3, 40]), 30.0, 3.0),
            (dict(n_body=3, n_flank=3, body_q=[1, 12, 30], flank_q=[2, 3, 40]), 0.0, 2.0)]
    got = run_jobs(harness, tmp_path, [f"F {r['n_body']} {r['n_flank']} {r['body_q'][1]} {r['flank_q'][1]} {cm} {pl}" for r, cm, pl in recs])
    assert [b[0] for b in got] == [gc.field(r, cm, pl) for r, cm, pl in recs]
    assert got[0][0] == "CN=1.00;RATIO=0.500;MED=15;FLANK=31;CHR=30;N=10" and got[1][0] == "CN=NA;RATIO=NA;MED=NA;FLANK=31;CHR=30.5;N=0"
    assert got[2][0] == "CN=0.00;RATIO=0.000;MED=0;FLANK=NA;CHR=29;N=7" and got[3][0].endswith("FLANK=1e+06;CHR=30;N=1234567")
