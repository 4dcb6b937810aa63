"""GPU: `rsicnv pin` and `rsicnv stat` on the device.  The two debug hooks on every case of pin_cases against the
Python restatement (integers, and the sample's doubles bit for bit); the kept CIGARs of a mixed BAM, in both read modes, against
the written records; the command line's rows against what the reference binary made of the same files
(tests/golden/pin_edges.npz); the windows of stat taken as given; the stated limits; and an unarmed context, which has no tables."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import bam_util as bu
import pairs_cases as pc
import pin_cases as pn

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "rsicnv_amd", "bin", "rsicnv")
SMALL = 65536
CASES = pn.cases()
NAMES = [n for n, _ in pc.refs(pn.TID_LEN)]


@pytest.fixture(scope="module")
def hot(hotlib):
    from rsicnv_amd import api
    h = api.RsiHot(0)
    yield h
    h.close()


@pytest.fixture(scope="module")
def restated():
    return {name: pn.expected(case) for name, case in CASES.items()}


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "pin_edges.npz"))


def calls_of(case):
    return [(s, e, t) for _, _, tid, s, e, t in pn.read_cnvlist(case.cnv, NAMES) if tid >= 0]


@pytest.mark.parametrize("name", list(CASES))
def test_sample_hook(hot, restated, name):
    sample = restated[name][0]
    table, cigs = pn.tables_of(CASES[name].reads)
    n = len(sample["rd_array"])
    st, rd, drd = hot.debug_pin_sample(table, cigs, pn.TID_LEN, rd_cap=n)
    assert (st["sample_reads"], st["pos_start"], st["pos_end"], st["l_qseq"]) == (sample["count"], sample["pos_start"], sample["pos_end"], sample["l_qseq"])
    assert np.array_equal(rd, sample["rd_array"]) and np.array_equal(drd, sample["drd_array"]) and rd.max() > 0 and np.abs(drd).max() > 0
    assert [st[k] for k in ("rd", "rd_sd", "drd", "drd_sd")] == [sample[k] for k in ("rd", "rd_sd", "drd", "drd_sd")]       # bit for bit


@pytest.mark.parametrize("name", list(CASES))
def test_calls_hook(hot, restated, name):
    sample, pins, _ = restated[name]
    case = CASES[name]
    table, cigs = pn.tables_of(case.reads)
    calls = calls_of(case)
    got = hot.debug_pin_calls(table, cigs, pn.TID_LEN, case.m, sample["l_qseq"], sample["drd_sd"], *zip(*calls))
    assert list(zip(*(g.tolist() for g in got))) == pins


def test_hooks_are_not_vacuous(restated):
    pins = [(p, c) for name in CASES for p, c in zip(restated[name][1], calls_of(CASES[name]))]
    assert sum(p[0] != c[0] for p, c in pins) >= 5 and sum(p[1] != c[1] for p, c in pins) >= 5, "vacuous: no breakpoint moved"
    assert sum(p[0] == c[0] and abs(c[1] - c[0]) >= 800 and c[2] != pn.UNKNOWN for p, c in pins) >= 3, "vacuous: every breakpoint looked at moved"


@pytest.mark.parametrize("name", list(pn.limit_cases()))
def test_limits(hot, name):
    from rsicnv_amd import api
    reads, words, tid_len = pn.limit_cases()[name]
    table, cigs = pn.tables_of(reads)
    with pytest.raises(api.RsiError) as e:
        hot.debug_pin_sample(table, cigs, tid_len)
    assert api.STATUS_NAMES[e.value.code] == "RSI_ERR_UNSUPPORTED" and words in str(e.value)


def test_window_beyond_the_lds_is_refused(hot):
    from rsicnv_amd import api
    table, cigs = pn.tables_of(CASES["types"].reads)
    ok = hot.debug_pin_calls(table, cigs, pn.TID_LEN, 2559, 100, 0.2, [2_000_000], [2_010_000], [0])
    assert ok[2][0] == 3 and ok[0][0] == 2_000_041                     # the largest window that fits finds the same base
    with pytest.raises(api.RsiError) as e:
        hot.debug_pin_calls(table, cigs, pn.TID_LEN, 2561, 100, 0.2, [2_000_000], [2_010_000], [0])
    assert api.STATUS_NAMES[e.value.code] == "RSI_ERR_UNSUPPORTED" and "LDS" in str(e.value)


def test_cigar_table(hot, tmp_path):
    """test_pairs_device.test_table's recipe: about 3000 records of chrS with mixed CIGARs (none, one, several operations), BGZF blocks
    cut at 4093 bytes so that records straddle every seam of the 64 KiB chunks.  The order in the pool is free: every read's words
    are read through its own offset."""
    rng = np.random.default_rng(0x7AB1E)
    refs = [("chrA", 50_000), ("chrS", 37_001), ("chrT", 9_000)]
    recs = []
    for t, (_, n) in enumerate(refs):
        for r in bu.synth_reads(n, coverage=8.0, seed=0x51 + t):
            b = bytearray(r)
            b[4:8] = struct.pack("<i", t)
            b[24:36] = struct.pack("<iii", int(rng.choice([-1, 0, 1, 1, 1, 2])), int(rng.integers(-1, n)), int(rng.integers(-70000, 70000)))
            recs.append(bytes(b))
    bam = str(tmp_path / "mixed.bam")
    bu.write_bam(bam, refs, recs, block=4093, straddle=True)
    lq, cigs = pn.cigars_from_bytes(recs, 1)
    assert 2500 < len(lq) < 3500 and {0, 1, 2, 3} <= {len(c) for c in cigs}
    for mode in ("host", "device"):
        hot.set_bam_read(mode, chunk_bytes=SMALL)
        hot.set_bam_pin(True)
        try:
            hot.load_depth_bam(bam, "chrS")
            got_lq, coff, pool = hot.fetch("pin_lq"), hot.fetch("pin_coff").view(np.uint32), hot.fetch("pin_pool").view(np.uint32)
            st, ps = hot.pin_stats(), hot.pairs_stats()
        finally:
            hot.set_bam_read("host")
            hot.set_bam_pin(False)
            hot.set_bam_pairs(False)
        assert got_lq.tolist() == lq, mode
        assert [pool[o + 1:o + 1 + pool[o]].tolist() for o in coff.tolist()] == cigs, mode
        words = 1 + sum(len(c) + 1 for c in cigs)
        assert st["records"] == ps["records"] == len(lq) and st["pool_words"] == len(pool) == words and st["table_bytes"] == 8 * len(lq) + 4 * words
        spans = sorted((o, o + 1 + int(pool[o])) for o in coff.tolist())             # the reads' words tile the pool behind its first word
        assert spans[0][0] == 1 and spans[-1][1] == words and all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
    assert hot.bam_read_stats()["mode"] == "device" and hot.bam_read_stats()["chunks"] >= 2


def run_cli(tmp, function, tag, bam, cnv, m, extra=()):
    out = os.path.join(tmp, f"{tag}.{function}.txt")
    r = subprocess.run([EXE, function, "-b", bam, "-v", cnv, "-o", out, "-m", str(m), *extra], cwd=tmp, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return open(out).read().splitlines(), open(out + ".log").read()


@pytest.mark.parametrize("k,name", list(enumerate(CASES)))
def test_command_line_rows(hotlib, golden, tmp_path, k, name):
    """`rsicnv pin` and `rsicnv stat` on the case's BAM (no .bai), the read mode alternating from case to case: START and END of every
    row, and the RP=..;Q0=.. column as printed, are what the reference binary wrote; the other fields are the line's own."""
    tmp, case = str(tmp_path), CASES[name]
    bam, cnv = os.path.join(tmp, "case.bam"), os.path.join(tmp, "case.cnv")
    pn.write_case_bam(bam, case.reads)
    open(cnv, "w").write(case.cnv + "\n")
    extra = ["-bamread", "device"] if k % 2 else []
    lines = pn.read_cnvlist(case.cnv, NAMES)
    known = [ln for ln in lines if ln[2] >= 0]
    pin_rows, pin_log = run_cli(tmp, "pin", name, bam, cnv, case.m, extra)
    stat_rows, stat_log = run_cli(tmp, "stat", name, bam, cnv, case.m, extra)
    assert len(pin_rows) == len(stat_rows) == len(lines)
    g_pin, g_stat, at = golden[name + ".pin"].tolist(), golden[name + ".stat"].tolist(), 0
    for (line, cell, tid, _s, _e, _t), prow, srow in zip(lines, pin_rows, stat_rows):
        if tid < 0:
            assert prow == srow == line and f"{cell[0]} is not in the BAM header" in pin_log and f"{cell[0]} is not in the BAM header" in stat_log
            continue
        f = prow.split("\t")
        assert f[0] == cell[0] and [int(f[1]), int(f[2])] == g_pin[at] and f[3:-1] == cell[3:] and re.fullmatch(r"SC=\d+;\d+", f[-1])
        assert srow == line + "\t" + g_stat[at]
        at += 1
    assert at == len(known) == len(g_pin)
    g_sample = golden[name + ".sample"].tolist()
    for key, val in zip(("sample chr ", "read length", "rd mean    ", "rd sd      ", "drd mean   ", "drd sd     "), g_sample):
        assert f"{key}: {val}\n" in pin_log
    if name == "types":
        assert any(g != [s, e] for g, (_, _, _, s, e, _) in zip(g_pin, known)) and any(g == [s, e] for g, (_, _, _, s, e, _) in zip(g_pin, known))
        assert any(not s.startswith("RP=0;") for s in g_stat), "vacuous: no breakpoint moved, none stayed, or no RP above 0"


def two_chromosome_bam(tmp):
    refs, reads, cnv = pn.stat_two_chromosomes()
    bam = os.path.join(tmp, "two.bam")
    bu.write_bam(bam, refs, pn.encode(reads, 0) + pn.encode(reads, 1), block=20000)
    return refs, reads, cnv, bam


def test_stat_windows_are_taken_as_given(hot, golden, tmp_path):
    """DIS travels from chrA's long call to chrP's short one: the device looks at the table entries of the carried window, not of
    the one a fresh DIS = 1000 gives; the rows are the reference's either way (pin_cases.stat_two_chromosomes says why)."""
    tmp = str(tmp_path)
    refs, reads, cnv, bam = two_chromosome_bam(tmp)
    lines = pn.read_cnvlist(cnv, [n for n, _ in refs])
    calls = [(s, e, t) for _, _, _, s, e, t in lines]
    carried, fresh = pn.stat_windows(calls), pn.stat_windows(calls[1:2])
    assert carried[1][2:] == (3_000_000 - 5000, 3_000_400 + 5000) and fresh[0][2:] == (3_000_000 - 1000, 3_000_400 + 1000)
    table, _ = pn.tables_of(reads)
    pos, span = table[0], int(np.max(table[1] - table[0]))
    isize = pc.isize_expected(pc.sample_expected(table, pn.TID_LEN))
    hot.set_bam_pairs(True)
    try:
        hot.load_depth_bam(bam, "chrP")
        seen = {}
        for tag, w in (("carried", carried[1]), ("fresh", fresh[0])):
            rp, q0, i1, i2 = hot.stat_calls([calls[1][0]], [calls[1][1]], [calls[1][2]], [w[2]], [w[3]])
            assert (i1, i2) == isize and [(int(rp[0]), float(q0[0]))] == pn.stat_restated(table, calls[1:2], [w], *isize)
            seen[tag] = hot.pairs_stats()["examined"]
            assert seen[tag] == int(np.searchsorted(pos, w[3], "left") - np.searchsorted(pos, w[2] - span, "left"))
        assert seen["carried"] > seen["fresh"] > 0 and rp[0] > 0
        assert hot.stat_calls([1], [2], [2], [1], [1001], 7, 8)[2:] == isize                 # a sample with pairs replaces what was carried
    finally:
        hot.set_bam_pairs(False)
    cnv_path = os.path.join(tmp, "two.cnv")
    open(cnv_path, "w").write(cnv + "\n")
    rows, log = run_cli(tmp, "stat", "two", bam, cnv_path, 101)
    assert rows == [ln[0] + "\t" + g for ln, g in zip(lines, golden["two_chromosomes.stat"].tolist())] and log.count("#stat: ") == 2
    r = subprocess.run([EXE, "stat", "-b", bam, "-v", cnv_path, "-o", os.path.join(tmp, "no.txt"), "-gpus", "2"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "-gpus" in r.stderr and not os.path.exists(os.path.join(tmp, "no.txt"))


def test_limits_from_the_command_line(hotlib, tmp_path):
    tmp = str(tmp_path)
    reads, words, _ = pn.limit_cases()["no_sample"]
    bam, cnv = os.path.join(tmp, "l.bam"), os.path.join(tmp, "l.cnv")
    pn.write_case_bam(bam, reads)
    text = pn.line(2_000_000, 2_010_000)
    open(cnv, "w").write(text + "\n")
    rows, log = run_cli(tmp, "pin", "limit", bam, cnv, 101)
    assert rows == [text] and words in log and "written unchanged" in log
    u = subprocess.run([EXE], capture_output=True, text=True, timeout=60)
    assert "rsicnv stat" in u.stderr + u.stdout and "rsicnv pin" in u.stderr + u.stdout
    p = subprocess.run([EXE, "plot", "-b", bam, "-v", cnv], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and "not part of the accelerated read-depth path" in p.stderr


def test_unarmed(hot, tmp_path):
    from rsicnv_amd import api
    bam = str(tmp_path / "u.bam")
    pn.write_case_bam(bam, CASES["ties"].reads)
    hot.load_depth_bam(bam, pn.CHROM)
    assert hot.pin_stats()["records"] == 0 and hot.pin_stats()["table_bytes"] == 0 and hot.pairs_stats()["records"] == 0
    for name in ("pin_lq", "pin_coff", "pin_pool"):
        with pytest.raises(KeyError):
            hot.fetch(name)
    with pytest.raises(api.RsiError) as e:
        hot.pin_sample()
    assert api.STATUS_NAMES[e.value.code] == "RSI_ERR_BAD_ARG" and "not armed" in str(e.value)
    hot.set_bam_pairs(True)                                              # the pair table alone does not serve pin
    try:
        hot.load_depth_bam(bam, pn.CHROM)
        with pytest.raises(api.RsiError) as e:
            hot.pin_sample()
        assert "rsi_hot_set_bam_pin" in str(e.value)
    finally:
        hot.set_bam_pairs(False)
    hot.set_bam_pin(True)
    try:
        hot.load_depth_bam(bam, pn.CHROM)
        with pytest.raises(api.RsiError) as e:
            hot.pin_calls(101, [2_000_000], [2_010_000], [0])
        assert "rsi_hot_pin_sample comes first" in str(e.value)
        st = hot.pin_sample()
        want = pn.expected(CASES["ties"])
        assert st["l_qseq"] == want[0]["l_qseq"] and st["drd_sd"] == want[0]["drd_sd"] and st["records"] == len(CASES["ties"].reads)
        got = hot.pin_calls(101, *zip(*calls_of(CASES["ties"])))
        assert list(zip(*(g.tolist() for g in got))) == want[1]
    finally:
        hot.set_bam_pin(False)
        hot.set_bam_pairs(False)
    hot.load_depth_bam(bam, pn.CHROM)                                    # the next load, unarmed, drops the tables
    assert hot.pin_stats()["records"] == 0


def test_abi(hotlib):
    from rsicnv_amd import api
    hdr = open(os.path.join(ROOT, "include", "rsi_hot.h")).read()
    for sym in ("rsi_hot_set_bam_pin", "rsi_hot_stat_calls", "rsi_hot_pin_sample", "rsi_hot_pin_calls", "rsi_hot_last_pin_stats", "rsi_hot_debug_pin_sample",
                "rsi_hot_debug_pin_calls"):
        assert re.search(r"\b" + sym + r"\(", hdr) and sym in api.EXPORTS and hasattr(hotlib, sym)
    body = re.search(r"typedef struct rsi_pin_stats \{(.*?)\} rsi_pin_stats;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    size = 0
    for decl in body.split(";"):
        t = decl.split()
        if t:
            size += {"int32_t": 4, "int64_t": 8, "double": 8}[t[0]] * (decl.count(",") + 1)
    assert C.sizeof(api.RsiPinStats) == size == 4 * 8 + 4 * 4 + 4 * 8 + 8 + 3 * 8
