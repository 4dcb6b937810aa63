"""CPU: the record finder's per-offset logic (rsicnv_amd/csrc/bam_walk_core.h: plausibility, hop, segment walk, stitch) as
plain C++ under ASan + UBSan (tests/sanitize/bam_walk_harness.cpp, a program of its own), segment by segment over inflated BAM
bytes, against a serial walk in Python (bam_walk_cases.serial_walk).  The result must be the serial chain's on every input:
the guess only decides how many segments are walked twice."""
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import bam_util as bu
import bam_walk_cases as bw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
REFLEN = [n for _, n in bw.REFS]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    tmp = tmp_path_factory.mktemp("bam_walk")
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", str(tmp / "probe")], input=b"int main(){return 0;}",
                           capture_output=True)
    if probe.returncode != 0:
        pytest.skip("g++ cannot link the sanitizer runtimes here")
    exe = str(tmp / "bam_walk_harness")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(ROOT, "tests", "sanitize", "bam_walk_harness.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def run(harness, tmp, jobs, seg=bw.SEG):
    """jobs: (bytes, start, tid).  Returns per job (recs, report dict)."""
    args = [harness, str(seg), str(len(REFLEN))] + [str(n) for n in REFLEN]
    for i, (data, start, tid) in enumerate(jobs):
        p = os.path.join(str(tmp), f"s{i}.bin")
        with open(p, "wb") as f:
            f.write(data)
        args += [p, str(start), str(tid)]
    r = subprocess.run(args, capture_output=True, text=True, env=ENV)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 2 * len(jobs)
    out = []
    for i in range(len(jobs)):
        rep = lines[2 * i].split()
        assert rep[0] == "report" and lines[2 * i + 1].startswith("recs")
        keys = ("listed", "seen", "end", "flags", "guessed", "rewalked", "passed")
        out.append(([int(x) for x in lines[2 * i + 1].split()[1:]], dict(zip(keys, map(int, rep[1:])))))
    return out


def check(got, data, start, tid, seg=bw.SEG):
    recs, rep = got
    want, seen, end, flags = bw.serial_walk(data, start, tid)
    assert recs == want
    assert (rep["listed"], rep["seen"], rep["end"], rep["flags"]) == (len(want), seen, end, flags)
    nseg = (len(data) + seg - 1) // seg
    assert rep["guessed"] + rep["rewalked"] + rep["passed"] <= nseg
    if not flags:
        assert rep["guessed"] + rep["rewalked"] + rep["passed"] == nseg
    return rep


def test_segment_constant_is_the_kernels():
    src = open(os.path.join(ROOT, "rsicnv_amd", "csrc", "kernels.h")).read()
    assert int(re.search(r"#define RSI_BAM_SEGMENT (\d+)", src).group(1)) == bw.SEG


@pytest.fixture(scope="module")
def golden(tmp_path_factory):
    _, refs, recs = bu.build_golden_bam(str(tmp_path_factory.mktemp("golden")))
    assert refs == bw.REFS
    return recs


def test_golden_stream_whole_and_from_index_starts(harness, tmp_path, golden):
    data = b"".join(golden)
    offs = np.concatenate([[0], np.cumsum([len(r) for r in golden])])
    first_s = next(i for i, r in enumerate(golden) if struct.unpack_from("<i", r, 4)[0] == 1)
    # a .bai gives the start of a chromosome's first read, or of a read in front of it: the first chrS read, a few reads
    # before it, and a spread of chrA reads
    starts = [(0, 0), (0, 1), (int(offs[first_s]), 1), (int(offs[first_s - 3]), 1)] + [(int(offs[i]), 0) for i in range(1, first_s, 997)]
    got = run(harness, tmp_path, [(data, s, t) for s, t in starts])
    for g, (s, t) in zip(got, starts):
        rep = check(g, data, s, t)
    whole = got[0][1]
    assert whole["flags"] == bw.BEYOND and whole["guessed"] > 10 * whole["rewalked"]     # ordinary reads: the guesses hold


@pytest.fixture(scope="module")
def streams():
    return {k: (b"".join(recs), tid) for k, (refs, recs, tid) in bw.cases().items()}


def test_list_a(harness, tmp_path, streams):
    names = list(streams)
    got = run(harness, tmp_path, [(streams[k][0], 0, streams[k][1]) for k in names])
    reps = {}
    for k, g in zip(names, got):
        reps[k] = check(g, streams[k][0], 0, streams[k][1])
    for k in ("straddle1", "straddle2", "straddle3"):
        data = streams[k][0]
        split = int(k[-1])
        assert bw.serial_walk(data, bw.SEG - split, 0)[0][0] == bw.SEG - split       # a record does start there
        assert reps[k]["flags"] == 0 and reps[k]["passed"] == 0
    assert bw.SEG in bw.serial_walk(streams["ends_on_seam"][0], 0, 0)[0]
    assert reps["long_record"]["passed"] >= 2 and reps["long_record"]["flags"] == 0
    assert reps["decoys"]["rewalked"] >= 1 and reps["decoys"]["flags"] == 0          # the verify path ran
    assert reps["beyond"]["flags"] == bw.BEYOND and reps["beyond"]["end"] == bw.SEG + 5000
    assert reps["unplaced"]["flags"] == bw.BEYOND and reps["unplaced"]["listed"] == 60
    assert reps["bad_chain"]["flags"] == bw.BAD and reps["bad_chain"]["listed"] == 200
    assert reps["bad_body"]["flags"] == 0 and reps["bad_body"]["listed"] == 410
    assert reps["cut"]["flags"] == bw.OPEN and reps["cut"]["end"] == len(streams["cut"][0]) - 57
    assert reps["empty"] == dict(listed=0, seen=0, end=0, flags=0, guessed=0, rewalked=0, passed=0)


def test_decoys_are_the_lowest_plausible_offsets(harness, tmp_path, streams):
    """With one segment per seam the decoy segment's guess is the decoy itself: the walk from the true entry differs from it."""
    data, tid = streams["decoys"]
    (recs, rep), = run(harness, tmp_path, [(data, 0, tid)])
    assert bw.SEG not in recs and 2 * bw.SEG not in recs and rep["rewalked"] >= 2    # both decoys sit on a seam; neither is a record


def test_other_segment_sizes(harness, tmp_path, streams):
    for seg in (64, 1000, 40000):
        names = [k for k in streams]
        got = run(harness, tmp_path, [(streams[k][0], 0, streams[k][1]) for k in names], seg=seg)
        for k, g in zip(names, got):
            check(g, streams[k][0], 0, streams[k][1], seg=seg)


def test_random_truncations_and_byte_flips(harness, tmp_path, golden):
    data = b"".join(golden[:400])
    rec_at = np.concatenate([[0], np.cumsum([len(r) for r in golden[:400]])[:-1]])
    rng = np.random.default_rng(20240)
    jobs = []
    for i in range(500):
        d = bytearray(data)
        for _ in range(int(rng.integers(1, 6))):
            at = int(rng.integers(0, len(d)))
            # the length and reference-id fields are where a flip changes the chain: aim half of the flips at them
            if rng.integers(0, 2):
                at = int(rec_at[rng.integers(0, len(rec_at))]) + int(rng.integers(0, 8))
            d[at] = int(rng.integers(0, 256))
        if i % 2:
            d = d[:int(rng.integers(0, len(d) + 1))]
        jobs.append((bytes(d), 0, 0))
    flagged = 0
    for a in range(0, len(jobs), 100):
        for g, (d, s, t) in zip(run(harness, tmp_path, jobs[a:a + 100]), jobs[a:a + 100]):
            flagged += check(g, d, s, t)["flags"] != 0
    assert flagged > 100            # the mutations do break chains
