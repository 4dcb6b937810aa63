"""CPU: rsicnv_amd/csrc/depth_host.h in a stand-alone program under ASan + UBSan (tests/depth_harness.cpp) equals
the Python restatement of depth_cases.py: the rounding rule, the window table, clipping and written coordinates, the slice plan,
the BED reader with its refusals, and the summary and distribution files."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import depth_cases as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


def test_restatement_is_what_it_says():
    assert [dc.fixed2(*a) for a in ((1, 200), (1, 8), (199, 200), (0, 5), (5, 0), (-3, 2), (7, 2), (1, 3), (2, 3))] == \
        ["0.01", "0.13", "1.00", "0.00", "0.00", "0.00", "3.50", "0.33", "0.67"]
    assert dc.fixed2(dc.I32MAX * 5, 5) == f"{dc.I32MAX}.00" and dc.fixed2((1 << 62) + 1, 3) == "1537228672809129301.67"
    for d, W, mean in dc.TIES:
        assert dc.fixed2(int(d.astype(np.int64).sum()), W) == mean
    # half up, against exact rational arithmetic
    from fractions import Fraction
    rng = np.random.default_rng(3)
    for S, L in zip(rng.integers(0, 1 << 40, 500), rng.integers(1, 1 << 20, 500)):
        q = dc.hundredths(S, L)
        assert Fraction(2 * q - 1, 200) <= Fraction(int(S), int(L)) < Fraction(2 * q + 1, 200)
    assert dc.windows(10, 3) == [(0, 3), (3, 6), (6, 9), (9, 10)] and dc.windows(10, 11) == [(0, 10)] and dc.windows(0, 5) == []
    assert dc.written(-5, 7, 100) == (0, 7) and dc.written(120, 130, 100) == (120, 130) and dc.written(5, 5, 100) == (5, 5)
    d = np.array([0, 1, 1, 70000, 3], dtype=np.int32)
    assert dc.summary(d) == dict(n=5, sum=70005, over=1, negative=0, min=0, max=70000)
    assert dc.dist(d)[65535] == 1 and dc.dist(d)[1] == 2 and dc.dist(d).sum() == 5
    assert dc.dist_lines("c", dc.dist(np.array([0, 2, 2, 1])), 4, 2) == "c\t2\t0.50\nc\t1\t0.75\nc\t0\t1.00\n"
    assert dc.summary_text([("a", np.array([1, 2, 3])), ("b", np.array([], dtype=np.int32))]) == \
        "chrom\tlength\tbases\tmean\tmin\tmax\na\t3\t6\t2.00\t1\t3\nb\t0\t0\t0.00\t0\t0\ntotal\t3\t6\t2.00\t1\t3\n"
    sizes = {v.size for v in dc.value_cases().values()}
    assert sizes == {3 * dc.SPAN + 17}
    r = dc.region_cases(3017)
    assert len(r["batch_3000"]) == 3000 and r["none"] == [] and any(e > 3017 for _, e in r["batch_3000"]) and any(s < 0 for s, _ in r["batch_3000"])


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    tmp = tmp_path_factory.mktemp("depth_harness")
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", str(tmp / "probe")], input=b"int main(){return 0;}",
                           capture_output=True)
    if probe.returncode != 0:
        pytest.skip("g++ cannot link the sanitizer runtimes here")
    exe = str(tmp / "depth_harness")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(ROOT, "tests", "depth_harness.cpp"), "-o", exe], capture_output=True, text=True)
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


def test_rounding_windows_and_clipping(harness, tmp_path):
    rng = np.random.default_rng(7)
    pairs = [(1, 200), (1, 8), (199, 200), (1197, 400), (0, 5), (5, 0), (-3, 2), (3, -2), (dc.I32MAX * 5, 5), ((1 << 62) + 1, 3), ((1 << 62), 1),
             ((1 << 54) - 1, (1 << 54))]
    pairs += [(int(s), int(l)) for s, l in zip(rng.integers(0, 1 << 45, 400), rng.integers(1, 1 << 31, 400))]
    pairs += [(int(l * k + l // 2), int(l)) for l, k in zip(rng.integers(2, 5000, 200), rng.integers(0, 90, 200))]       # halves of a hundredth's step
    pairs += [(int((200 * k + 199) * l // 200), int(l)) for l, k in zip(rng.integers(200, 5000, 100), rng.integers(0, 90, 100))]   # just below a carry
    got = run_jobs(harness, tmp_path, [f"H {s} {l}" for s, l in pairs])
    assert [b[0] for b in got] == [dc.fixed2(s, l) for s, l in pairs]
    nw = [(0, 5), (1, 1), (10, 3), (10, 10), (10, 11), (1000, 1), (1001, 500), (50000, 500), (7, 1 << 40)]
    got = run_jobs(harness, tmp_path, [f"W {n} {w}" for n, w in nw])
    for (n, w), b in zip(nw, got):
        want = [(k * w, min(n, (k + 1) * w)) for k in range(-(-n // w))]
        assert int(b[0]) == len(want) and [tuple(int(v) for v in ln.split()) for ln in b[1:]] == want
    cl = [(-5, 7, 100), (95, 130, 100), (-3, 103, 100), (120, 130, 100), (-9, -2, 100), (-9, 0, 100), (100, 105, 100), (5, 5, 100), (9, 3, 100), (0, 100, 100),
          (0, 10, 0), (-(1 << 62), 1 << 62, 50)]
    got = run_jobs(harness, tmp_path, [f"C {s} {e} {n}" for s, e, n in cl])
    for (s, e, n), b in zip(cl, got):
        a, bb = dc.clip(s, e, n)
        assert b[0] == f"{a} {bb} {1 if bb > a else 0}" and b[1] == "%d %d" % dc.written(s, e, n)


def test_plan_bounds(harness, tmp_path):
    jobs = [(1, 0, 0), (1, 1, 0), (5, 100, 0), (5, 100, 7), (255, 10 ** 9, 0), (4, 10 ** 9, 10 ** 9), (4, 3, 50), (4, -1, 0)]
    got = run_jobs(harness, tmp_path, [f"P {a} {b} {c}" for a, b, c in jobs])
    for (name_len, count, want_slice), b in zip(jobs, got):
        if count < 0:
            assert b[0] == "bad"
            continue
        s, max_line, cap = (int(v) for v in b[0].split())
        assert max_line == name_len + 4 + 40 + 23 and cap == s * max_line and cap <= 32 << 20 and 1 <= s <= max(count, 1) and s <= 512 << 10
        if want_slice and want_slice <= count and want_slice * max_line <= 32 << 20:
            assert s == min(want_slice, 512 << 10)


def test_bed_reader(harness, tmp_path):
    good = tmp_path / "good.bed"
    good.write_text("# a comment\ntrack name=x\nbrowser position chr1\n\nchr1\t10\t20\tname\t0\t+\n1 5 5\nchrX\t0\t7\r\n  chr1   30   40  \nchr1\t10\t20\n")
    bad = {"few.bed": ("chr1\t5\n", "line 1: fewer than three fields"), "neg.bed": ("chr1\t1\t2\nchr1\t-1\t5\n", "line 2: start and end must be non-negative integers"),
           "word.bed": ("\n\nchr1\tx\t5\n", "line 3: start and end must be non-negative integers"), "rev.bed": ("chr1\t9\t3\n", "line 1: end < start"),
           "long.bed": ("chr1\t1\t1234567890123456789\n", "line 1: start and end must be non-negative integers")}
    for name, (text, _) in bad.items():
        (tmp_path / name).write_text(text)
    got = run_jobs(harness, tmp_path, [f"B {good}"] + [f"B {tmp_path / name}" for name in bad] + [f"B {tmp_path / 'missing.bed'}"])
    assert got[0] == ["ok", "chr1 10 20", "1 5 5", "chrX 0 7", "chr1 30 40", "chr1 10 20"]
    for (name, (_, msg)), b in zip(bad.items(), got[1:]):
        assert b == [f"bad {tmp_path / name}: {msg}"]
    assert got[-1] == ["ok"]                       # (the caller opens the file and says when it cannot)


def test_summary_and_dist_files(harness, tmp_path):
    vals = dc.value_cases()
    chroms = [("chr1", vals["poisson_30"]), ("chr2", vals["around_65535"]), ("empty", np.zeros(0, dtype=np.int32)), ("chrX", vals["int32_max_beside_0"]),
              ("z", vals["all_zero"][:9])]
    rows = " ".join(f"{nm} {d.size} {int(d.astype(np.int64).sum())} {int(d.min()) if d.size else 0} {int(d.max()) if d.size else 0}" for nm, d in chroms)
    jobs = [f"S {len(chroms)} {rows}", "S 0"]
    for nm, d in chroms:
        b = dc.dist(d)
        nz = np.flatnonzero(b)
        jobs.append(f"D {nm} {d.size} {int(d.max()) if d.size else 0} {nz.size} " + " ".join(f"{k} {b[k]}" for k in nz))
    got = run_jobs(harness, tmp_path, jobs)
    assert "\n".join(got[0]) + "\n" == dc.summary_text(chroms)
    assert got[1] == ["chrom\tlength\tbases\tmean\tmin\tmax", "total\t0\t0\t0.00\t0\t0"]
    per = "".join("\n".join(b) + "\n" if b else "" for b in got[2:])
    assert per + dc.dist_lines("total", sum(dc.dist(d) for _, d in chroms), sum(d.size for _, d in chroms), dc.I32MAX) == dc.dist_text(chroms)
    assert len(got[3]) == 65536 and got[3][0] == "chr2\t65535\t" + dc.fixed2(int((vals["around_65535"] >= 65535).sum()), vals["around_65535"].size)
