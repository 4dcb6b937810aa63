"""CPU: `rsicnv pin` and `rsicnv stat` stated three times agree on every case of pin_cases -- what the reference binary made of the
case's BAM (tests/golden/pin_edges.npz), the Python restatement of pairrd.cpp, and bam_pin_core.h's serial forms with pin_host.h's
host functions in one stand-alone program under ASan + UBSan (tests/pin_harness.cpp) -- and the CNV-list reader takes the line
forms read_cnvlist takes."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import pairs_cases as pc
import pin_cases as pn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
CASES = pn.cases()
NAMES = [n for n, _ in pc.refs(pn.TID_LEN)]


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "pin_edges.npz"))


@pytest.fixture(scope="module")
def restated():
    return {name: pn.expected(case) for name, case in CASES.items()}


def printed(v):
    return "%g" % v                                          # an ostream's default format of a double


def test_restatement_equals_the_reference(golden, restated):
    moved = stayed = some_rp = 0
    for name, (sample, pins, stats) in restated.items():
        assert [list(p[:2]) for p in pins] == golden[name + ".pin"].tolist(), name
        assert [f"RP={rp};Q0={printed(q0)}" for rp, q0 in stats] == golden[name + ".stat"].tolist(), name
        want = [pn.CHROM, str(sample["l_qseq"])] + [printed(sample[k]) for k in ("rd", "rd_sd", "drd", "drd_sd")]
        assert want == golden[name + ".sample"].tolist(), name
        calls = [(s, e) for _, _, tid, s, e, _ in pn.read_cnvlist(CASES[name].cnv, NAMES) if tid >= 0]
        moved += sum(a != s for (a, _, _, _), (s, _) in zip(pins, calls)) + sum(b != e for (_, b, _, _), (_, e) in zip(pins, calls))
        stayed += sum(a == s for (a, _, _, _), (s, _) in zip(pins, calls))
        some_rp += sum(rp > 0 for rp, _ in stats)
    assert moved >= 10 and stayed >= 5 and some_rp >= 5, "vacuous: no breakpoint moved, none stayed, or no RP above 0"


def test_cases_are_what_they_say(restated):
    r = {k: v[1] for k, v in restated.items()}
    s = {k: v[0] for k, v in restated.items()}
    assert r["types"][0] == (2_000_041, 2_010_021, 3, 3) and r["types"][1][2:] == (0, 0)      # the issue's example; a 501-base call
    assert r["types"][7] == (4_000_010, 4_000_809, 0, 0) and r["types"][8][2:] == (3, 3)      # lengths 799 and 800
    assert r["types"][9] == (2_010_000, 2_000_000, 0, 0)                                      # START above END: nothing near either
    assert r["types"][10][0] == 60                                                            # START below r_len: a window from below 0
    assert r["ties"][0] == (2_000_041, 2_010_031, 2, 2)          # two equal maxima: the first; one clip does not move, two do
    assert r["ties"][1] == (6_000_000, 6_010_000, 0, 0)          # no depth, no clip: the best score is 0 and is not taken
    assert r["filters"][0] == (2_000_041, 2_010_000, 2, 0)       # of six clipped reads only mtid 0 and mtid -1 count
    assert r["negative_drd"][0][2:] == (0, 0) and r["lq101"][0][2:] == (0, 0)
    assert s["lq99"]["l_qseq"] == 99 and s["lq101"]["l_qseq"] == 101 and s["lq_mean_half"]["l_qseq"] == 101
    assert s["first_before_10mb"]["pos_start"] < 10_000_000 and s["restart"]["pos_start"] == 10_012_006
    stale = pn.sample_restated([x for x in CASES["restart"].reads if x.pos >= 10_012_000])
    assert stale["rd"] != s["restart"]["rd"], "the first stretch's counts must still be in the second one's array"
    assert s["flat_sample"]["drd_sd"] < 0.15 and s["chromosome_end"]["pos_start"] > 10_090_000
    lim = {k: pn.sample_restated(reads, n) for k, (reads, _, n) in pn.limit_cases().items()}
    assert lim["no_sample"]["count"] == 0 and lim["grows"]["grows"]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    tmp = tmp_path_factory.mktemp("pin_harness")
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", str(tmp / "probe")], input=b"int main(){return 0;}",
                           capture_output=True)
    if probe.returncode != 0:
        pytest.skip("g++ cannot link the sanitizer runtimes here")
    exe = str(tmp / "pin_harness")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                        os.path.join(ROOT, "tests", "pin_harness.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


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
            blocks[-1].append(ln)
    assert len(blocks) == len(lines)
    return blocks


def write_words(path, arrays):
    with open(path, "wb") as f:
        for a in arrays:
            f.write((np.asarray(a, dtype=np.int64) & 0xffffffff).astype(np.uint32).tobytes())


@pytest.fixture(scope="module")
def core_runs(harness, tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("pin_core"))
    lines = []
    for name, case in CASES.items():
        table, cigs = pn.tables_of(case.reads)
        write_words(os.path.join(tmp, name + ".tab"), table)
        write_words(os.path.join(tmp, name + ".cig"), cigs)
        calls = [(s, e, t) for _, _, tid, s, e, t in pn.read_cnvlist(case.cnv, NAMES) if tid >= 0]
        lines.append(f"P {tmp}/{name}.tab {len(table[0])} {tmp}/{name}.cig {len(cigs[2])} {pn.TID_LEN} {case.m} {len(calls)} " +
                     " ".join(f"{s} {e} {t}" for s, e, t in calls))
    for name, (reads, _, tid_len) in pn.limit_cases().items():
        table, cigs = pn.tables_of(reads)
        write_words(os.path.join(tmp, name + ".tab"), table)
        write_words(os.path.join(tmp, name + ".cig"), cigs)
        lines.append(f"P {tmp}/{name}.tab {len(table[0])} {tmp}/{name}.cig {len(cigs[2])} {tid_len} 101 0")
    return dict(zip(list(CASES) + list(pn.limit_cases()), run_jobs(harness, tmp, lines)))


@pytest.mark.parametrize("name", list(CASES))
def test_core_equals_the_restatement(core_runs, restated, name):
    sample, pins, _ = restated[name]
    s = core_runs[name][0].split()
    assert s[0] == "s" and [int(v) for v in s[1:4]] == [sample["count"], sample["pos_start"], sample["pos_end"]] and int(s[5]) == sample["l_qseq"]
    got = [float.fromhex(v) for v in s[6:10]]
    want = [sample[k] for k in ("rd", "rd_sd", "drd", "drd_sd")]
    assert got == want                                       # the doubles bit for bit
    assert [tuple(int(v) for v in ln.split()[1:]) for ln in core_runs[name][1:]] == pins


def test_core_flags_the_limits(core_runs):
    assert core_runs["no_sample"][0].split()[1] == "0"
    assert int(core_runs["grows"][0].split()[4]) & 1


def test_cnv_list_reader(harness, tmp_path):
    text = "\n".join(["#CHROM\tSTART\tEND\tTYPE", "", "abcd", "chrP 1", "chrP\t100\t900\tDEL", "  chrP   5x   7e3  my_LOSS_call   extra  fields ",
                      "chrP\t-5\t+12\tdupdel", "chrP\t1\t2\tadd-del", "chrP\t1\t2\tGAIN", "chrP\t1\t2\tinv", "chrp\t1\t2\tDEL", "chr2\t9999\t20000\tDup\tq",
                      "chrP\t2000000\t1990000\tDEL"])
    cnv = str(tmp_path / "list.txt")
    open(cnv, "w").write(text + "\n")
    block = run_jobs(harness, str(tmp_path), [f"L {cnv} " + " ".join(NAMES), f"L {cnv}.missing chrP"])
    want = pn.read_cnvlist(text, NAMES)
    assert [w[2:] for w in want] == [(1, 100, 900, 0), (1, 5, 7, 0), (1, -5, 12, 1), (1, 1, 2, 1), (1, 1, 2, 1), (1, 1, 2, 2), (-1, 1, 2, 0), (2, 9999, 20000, 1),
                                     (1, 2000000, 1990000, 0)]
    windows = pn.stat_windows([(s, e, t) for _, _, _, s, e, t in want])
    got = [ln.split(" ", 1)[1] for ln in block[0]]
    for k, (line, cell, tid, start, end, type_) in enumerate(want):
        assert got[3 * k] == f"{tid} {start} {end} {type_} {len(cell)} {windows[k][2]} {windows[k][3]}"
        assert got[3 * k + 1] == line + "\tRP=3;Q0=0.333333"
        assert got[3 * k + 2] == "\t".join([cell[0], str(start + 1), str(end - 1)] + cell[3:]) + "\tSC=2;0"
    assert len(got) == 3 * len(want) and block[1] == ["none"]
    assert windows[0][2:] == (1, 1900) and windows[7][2:] == (9999 - 5000, 25000) and windows[8][2:] == (1985000, 2005000)   # DIS: 1000, then carried
