"""CPU: the host side of the tabix index (rsicnv_amd/csrc/track_index_host.h: the builder that merges the device's per-slice
records, the .tbi writer, the .tbi / .csi parser) built as a stand-alone program under AddressSanitizer +
UndefinedBehaviorSanitizer (tests/sanitize_index) and run through its checks, with no sanitizer report.  What it writes is
parsed back field by field by tabix_util; what tabix_util writes, it parses."""
import gzip
import os
import shutil
import subprocess

import pytest

import tabix_util as tx
from bgzf_util import bgzf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "tests", "sanitize_index", "index_harness")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


def vo(coff, uoff):
    return coff << 16 | uoff


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    tmp = tmp_path_factory.mktemp("probe")
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", str(tmp / "probe")], input=b"int main(){return 0;}",
                           capture_output=True)
    if probe.returncode != 0:
        pytest.skip("g++ cannot link the sanitizer runtimes here")
    r = subprocess.run(["make", "-f", "tests/sanitize_index/Makefile"], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return HARNESS


def run(harness, *args):
    r = subprocess.run([harness] + [str(a) for a in args], capture_output=True, text=True, env=ENV, timeout=100)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    return r


@pytest.mark.timeout(120)
def test_builder_and_writer_under_sanitizers(harness, tmp_path):
    r = run(harness, "build", tmp_path)
    assert r.returncode == 0 and "index host ok" in r.stdout, r.stdout[-1000:] + r.stderr[-3000:]
    assert sorted(os.listdir(tmp_path)) == ["joined.tbi", "none.tbi", "one.tbi", "two.tbi"]
    head = dict(format=0x10000, col_seq=1, col_beg=2, col_end=3, meta=ord("#"), skip=0)
    one = tx.parse_index(str(tmp_path / "one.tbi"))
    assert one["kind"] == "tbi" and one["names"] == ["chrA", "chrB"] and one["header"] == head and one["trailing"] == 0
    a, b = one["refs"]
    # merged across the slices at 1000 and the calls at 1600; bins ascending; no pseudo-bin
    assert a["order"] == [585, 4681, 4682, 4687, 4690] and a["pseudo"] is None
    assert a["bins"] == {4681: [(vo(0, 0), vo(400, 7))], 4682: [(vo(400, 7), vo(700, 0))], 585: [(vo(700, 0), vo(1300, 50))],
                         4687: [(vo(1300, 50), vo(1610, 3))], 4690: [(vo(1610, 3), vo(1800, 0))]}
    # windows 7 and 8, which no line touched, take window 9's offset
    assert a["linear"] == [vo(0, 0), vo(400, 7), vo(700, 0)] + [vo(1300, 50)] * 4 + [vo(1610, 3)] * 3
    assert b["bins"] == {4683: [(vo(1800, 0), vo(1864, 0))]} and b["linear"] == [vo(1800, 0)] * 3
    two = tx.parse_index(str(tmp_path / "two.tbi"))
    assert two["names"] == ["chrC"] and two["refs"][0]["bins"] == {4681 + 32767: [(0, vo(100, 0))]} and two["refs"][0]["linear"] == [0] * 32768
    joined = tx.parse_index(str(tmp_path / "joined.tbi"))
    assert joined["names"] == ["chrA", "chrB", "chrC"] and joined["refs"][0]["bins"] == a["bins"] and joined["refs"][1]["linear"] == b["linear"]
    assert joined["refs"][2]["bins"] == {4681 + 32767: [(vo(5000, 0), vo(5100, 0))]} and joined["refs"][2]["linear"] == [vo(5000, 0)] * 32768
    none = tx.parse_index(str(tmp_path / "none.tbi"))
    assert none["names"] == [] and none["refs"] == []
    # the stream is the documented one, byte for byte: tabix_util writes the same from the parsed fields
    for name, index in (("one", one), ("joined", joined)):
        assert gzip.decompress(open(tmp_path / f"{name}.tbi", "rb").read()) == tx.tbi_bytes(index)


def fixture_index(kind, min_shift=14, depth=5, names=("chr1", "chr2", "3")):
    refs = []
    for k, _ in enumerate(names):
        base = 10_000 * (k + 1)
        leaf = ((1 << depth * 3) - 1) // 7
        bins = {leaf + k: [(vo(base, 5), vo(base + 500, 0)), (vo(base + 900, 1), vo(base + 2_000, 77))], 0: [(vo(base + 500, 0), vo(base + 900, 1))]}
        refs.append(dict(bins=bins, linear=[vo(base, 5)] * (k + 1), loffset={b: vo(base, 5) for b in bins}))
    return dict(kind=kind, min_shift=min_shift, depth=depth, names=list(names), refs=refs)


PARSE_CASES = [("tbi", 14, 5, False, None), ("tbi", 14, 5, True, 3), ("csi", 14, 5, False, None), ("csi", 14, 5, True, 0), ("csi", 12, 6, True, None),
               ("csi", 12, 6, False, 9)]


@pytest.mark.timeout(120)
@pytest.mark.parametrize("kind,min_shift,depth,pseudo,n_no_coor", PARSE_CASES)
def test_parser_reads_what_the_format_says(harness, tmp_path, kind, min_shift, depth, pseudo, n_no_coor):
    index = fixture_index(kind, min_shift, depth)
    path = tmp_path / f"f.{kind}"
    tx.write_index(str(path), index, pseudo=pseudo, n_no_coor=n_no_coor)
    again = tx.parse_index(str(path))                      # the helper reads its own file
    assert again["names"] == index["names"] and [r["bins"] for r in again["refs"]] == [r["bins"] for r in index["refs"]]
    assert (again["refs"][0]["pseudo"] is not None) == pseudo
    # names with and without chr, in both directions; the pseudo-bin's "chunks" (offsets 7 and 0) never count
    for ask, k in (("chr1", 0), ("1", 0), ("chr2", 1), ("3", 2), ("chr3", 2)):
        base = 10_000 * (k + 1)
        r = run(harness, "parse", path, ask)
        assert r.returncode == 0 and r.stdout.split() == ["ok", kind, str(min_shift), str(depth), "3", str(vo(base, 5)), str(vo(base + 2_000, 77))], r.stdout
    r = run(harness, "parse", path, "chr9")
    assert r.returncode == 0 and r.stdout.split()[-1] == "none"


@pytest.mark.timeout(300)
@pytest.mark.parametrize("kind", ["tbi", "csi"])
def test_truncated_and_garbage_files_are_errors(harness, tmp_path, kind):
    raw = (tx.csi_bytes if kind == "csi" else tx.tbi_bytes)(fixture_index(kind), pseudo=True)
    path = tmp_path / "cut"
    cuts = sorted(set(list(range(0, 60)) + list(range(60, len(raw) - 1, 7)) + [len(raw) - 1]))
    for cut in cuts:                                       # every prefix is an error, none a crash
        path.write_bytes(bgzf(raw[:cut]))
        r = run(harness, "parse", path, "chr1")
        assert r.returncode == 2 and r.stdout.startswith("error: index "), (cut, r.stdout, r.stderr[-500:])
    for k, garbage in enumerate([b"", b"not an index at all", bgzf(b"TBI\x02" + raw[4:]), bgzf(raw)[:-40], bgzf(raw + b"xyz"),
                                 bgzf(raw[:8] + b"\xff\xff\xff\x7f" + raw[12:]), bgzf(raw[:4] + b"\xff\xff\xff\x7f" + raw[8:])]):
        path.write_bytes(garbage)
        r = run(harness, "parse", path, "chr1")
        assert r.returncode == 2 and r.stdout.startswith("error: index "), (k, r.stdout, r.stderr[-500:])
    path.write_bytes(bgzf(raw))
    assert run(harness, "parse", path, "chr1").returncode == 0
    assert run(harness, "parse", tmp_path / "missing", "chr1").returncode == 2
