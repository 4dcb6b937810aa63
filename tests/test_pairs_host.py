"""CPU: the read-pair annotation's three statements agree on every case of pairs_cases -- the Python restatement of pairrd.cpp,
the host functions (bam_host.cpp: bam_pair_sample, bam_annotate_calls, pinned to the reference binary by test_bam_depth) on a
BAM written from the case, and bam_pairs_core.h's logic run serially -- with both C++ sides in one stand-alone program under
ASan + UBSan (tests/pairs_harness.cpp).  The two count cases have no file: core and restatement only."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import pairs_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    tmp = tmp_path_factory.mktemp("pairs_harness")
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", str(tmp / "probe")], input=b"int main(){return 0;}",
                           capture_output=True)
    if probe.returncode != 0:
        pytest.skip("g++ cannot link the sanitizer runtimes here")
    exe = str(tmp / "pairs_harness")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                        os.path.join(ROOT, "tests", "pairs_harness.cpp"), os.path.join(ROOT, "rsicnv_amd", "csrc", "bam_host.cpp"), "-lz", "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def write_table(path, table):
    with open(path, "wb") as f:
        for a in table:
            f.write((np.asarray(a, dtype=np.int64) & 0xffffffff).astype(np.uint32).tobytes())


def run_jobs(exe, tmp, lines):
    job = os.path.join(tmp, "jobs.txt")
    open(job, "w").write("\n".join(lines) + "\n")
    r = subprocess.run([exe, job], capture_output=True, text=True, env=ENV, timeout=600)
    assert r.returncode == 0 and "error" not in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]
    blocks = []
    for ln in r.stdout.splitlines():
        if ln.startswith("job "):
            blocks.append([])
        else:
            blocks[-1].append(ln.split())
    assert len(blocks) == len(lines)
    return blocks


@pytest.fixture(scope="module")
def sample_runs(harness, tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("sample"))
    cases = dict(pc.sample_cases(), **pc.count_cases())
    lines = []
    for name, (reads, table, tid_len) in cases.items():
        tab = os.path.join(tmp, name + ".tab")
        write_table(tab, table)
        bam = "-"
        if reads is not None:
            bam = os.path.join(tmp, name + ".bam")
            pc.write_case_bam(bam, reads, tid_len)
            lines.append(f"X {bam} {pc.TID}")
        lines.append(f"S {bam} {pc.TID} {tid_len} {tab} {len(table[0])}")
    blocks = iter(run_jobs(harness, tmp, lines))
    out = {}
    for name, (reads, table, tid_len) in cases.items():
        out[name] = (next(blocks) if reads is not None else None, next(blocks))
    return cases, out


@pytest.mark.parametrize("name", list(pc.sample_cases()) + list(pc.count_cases()))
def test_sample(sample_runs, name):
    cases, out = sample_runs
    reads, table, tid_len = cases[name]
    extracted, sample = out[name]
    want = pc.sample_expected(table, tid_len)
    isize = pc.isize_expected(want)
    core = [r for r in sample if r[:2] == ["s", "core"]][0]
    assert [int(v) for v in core[2:6]] == want
    assert (int(core[6]), int(core[7])) == isize
    if reads is not None:
        host = [r for r in sample if r[:2] == ["s", "host"]][0]
        assert (int(host[2]), int(host[3])) == isize
        got = np.array([[int(v) for v in r[1:6]] for r in extracted], dtype=np.int64).reshape(-1, 5)
        assert np.array_equal(got.T, np.array(table)) and not any(int(r[6]) for r in extracted)


def test_sample_cases_are_what_they_say():
    c = dict(pc.sample_cases(), **pc.count_cases())
    stop = {k: pc.sample_expected(t, n) for k, (_, t, n) in c.items()}
    kept = {k: pc.sample_expected(t, 1 << 40)[3] for k, (_, t, n) in c.items()}
    assert pc.isize_expected(stop["two_pairs"]) == (-1, -1) and pc.isize_expected(stop["three_pairs"])[0] > 0
    assert stop["all_before"] == [0, 0, 0, -1] and stop["n0"][3] == -1 and stop["n1"][3] == 0
    assert stop["straddle_by_rend"][:2] == [6, 311 + sum(280 + (k * 7) % 50 for k in range(5))]
    assert stop["span_1000000"][3] == 1001 and stop["span_1000001"][3] == 1001                # the read behind the exact span / the one past it
    assert stop["count_1000000"][3] == 999_999 and stop["count_1000001"][3] == 1_000_000
    assert stop["stop_by_pos"][3] == 10 and stop["stop_by_rend"][3] == 10 and stop["no_cigar_at_the_end"][3] == 11
    assert stop["stop_last_of_tile"][3] == pc.TILE - 1 and stop["stop_first_of_tile"][3] == pc.TILE
    assert stop["square_wraps"][2] == 2 * 605_032_704 + 30 * 10_000 != sum(i * i for i in pc.WRAPPING)
    for k in ("gap_1000", "gap_1001", "passed_over_on_a_boundary", "passed_over_on_a_seam"):
        assert stop[k][3] == kept[k]


@pytest.fixture(scope="module")
def annotate_runs(harness, tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("annotate"))
    cases = pc.annotate_cases()
    lines = []
    for name, (reads, table, calls, mean, sd) in cases.items():
        tab, bam = os.path.join(tmp, name + ".tab"), os.path.join(tmp, name + ".bam")
        write_table(tab, table)
        pc.write_case_bam(bam, reads, 5_000_000)
        flat = " ".join(f"{s} {e} {t}" for s, e, t in calls)
        lines.append(f"A {bam} {pc.TID} {tab} {len(table[0])} {mean} {sd} {len(calls)} {flat}")
    return cases, dict(zip(cases, run_jobs(harness, tmp, lines)))


@pytest.mark.parametrize("name", list(pc.annotate_cases()))
def test_annotate(annotate_runs, name):
    cases, out = annotate_runs
    _, table, calls, mean, sd = cases[name]
    want = pc.annotate_expected(table, calls, mean, sd)
    core = [tuple(int(v) for v in r[2:5]) for r in out[name] if r[:2] == ["a", "core"]]
    host = [(int(r[2]), float.fromhex(r[3])) for r in out[name] if r[:2] == ["a", "host"]]
    assert core == want
    assert host == [(rp, pc.q0_of(qa, qq)) for rp, qa, qq in want]


def test_annotate_cases_reach_every_exit():
    seen = set()
    some_rp = some_q0 = 0
    for _, table, calls, mean, sd in pc.annotate_cases().values():
        for rp, qa, qq in pc.annotate_expected(table, calls, mean, sd, exits=seen):
            some_rp += rp; some_q0 += qq
    assert seen == set(pc.EXITS), set(pc.EXITS) - seen
    assert some_rp > 0 and some_q0 > 0
