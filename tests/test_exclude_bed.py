"""rsi_exclude_read_bed (include/rsi_hot.h): the BED file of an exclusion mask -> the normalised intervals of one chromosome.
Host only: no device is needed."""
import gzip

import numpy as np
import pytest

from rsicnv_amd import api

N = 100_000
BED = "\n".join([
    "track name=blacklist description=\"two words\"",
    "browser position chr1:1-1000",
    "# a comment",
    "",
    "chr1\t5000\t6000\tsatellite\t0\t+",        # extra columns
    "chr1 100 200",                              # blanks; out of order
    "chr1\t150\t300",                            # overlaps the line above
    "chr1\t300\t400",                            # touches it
    "1\t7000\t7100",                             # no chr prefix
    "chr2\t1\t99999",                            # another chromosome
    "chr1 \t 9000  \t9500\textra",               # mixed separators
    "chr1\t99990\t100500",                       # end > n
    "chr1\t200000\t200100",                      # all of it beyond n
    "chr1\t401\t402",                            # one base away from [100, 400): stays apart
    "",
]) + "\n"
EXPECT = [[100, 400], [401, 402], [5000, 6000], [7000, 7100], [9000, 9500], [99990, N]]


def write(tmp_path, text, name="mask.bed"):
    p = tmp_path / name
    p.write_text(text)
    return str(p)


def test_normalised_intervals(tmp_path):
    got = api.read_exclude_bed(write(tmp_path, BED), "chr1", N)
    assert got.dtype == np.int64 and got.tolist() == EXPECT


def test_chr_prefix_in_both_directions(tmp_path):
    p = write(tmp_path, BED)
    assert api.read_exclude_bed(p, "1", N).tolist() == EXPECT          # file says chr1, the caller 1
    assert api.read_exclude_bed(p, "chr2", N).tolist() == [[1, 99999]]
    assert api.read_exclude_bed(p, "2", N).tolist() == [[1, 99999]]
    assert api.read_exclude_bed(p, "chr3", N).shape == (0, 2)          # no lines: no intervals, no error
    q = write(tmp_path, "7\t10\t20\nchr7\t15\t30\nchr17\t50\t60\n", "seven.bed")
    assert api.read_exclude_bed(q, "chr7", N).tolist() == [[10, 30]]   # file says 7 and chr7, the caller chr7
    assert api.read_exclude_bed(q, "7", N).tolist() == [[10, 30]]


def test_gzip_file_reads_the_same(tmp_path):
    p = str(tmp_path / "mask.bed.gz")
    with gzip.open(p, "wb") as f:
        f.write(BED.encode())
    assert api.read_exclude_bed(p, "chr1", N).tolist() == EXPECT


def test_small_cap_still_returns_the_count(tmp_path):
    lib = api.load_library()
    p = write(tmp_path, BED).encode()
    assert lib.rsi_exclude_read_bed(p, b"chr1", N, None, None, 0) == len(EXPECT)
    s, e = np.full(4, -1, dtype=np.int64), np.full(4, -1, dtype=np.int64)
    assert lib.rsi_exclude_read_bed(p, b"chr1", N, s.ctypes.data, e.ctypes.data, 2) == len(EXPECT)
    assert s.tolist() == [100, 401, -1, -1] and e.tolist() == [400, 402, -1, -1]


def test_no_final_newline_and_crlf(tmp_path):
    assert api.read_exclude_bed(write(tmp_path, "chr1\t5\t9\r\nchr1\t20\t30"), "chr1", N).tolist() == [[5, 9], [20, 30]]


MALFORMED = [
    ("chr1\t500", "two fields"),
    ("chr1", "one field"),
    ("chr1\tabc\t900", "non-numeric start"),
    ("chr1\t500\t9x0", "non-numeric end"),
    ("chr1\t5.0\t900", "a decimal point"),
    ("chr1\t-5\t900", "negative start"),
    ("chr1\t500\t-3", "negative end"),
    ("chr1\t500\t500", "end == start"),
    ("chr1\t500\t400", "end < start"),
    ("chr9\t500\t400", "end < start on another chromosome"),
    ("chr1\t500\t99999999999999999999", "a coordinate beyond long long"),
]


@pytest.mark.parametrize("bad,what", MALFORMED, ids=[w.replace(" ", "_") for _, w in MALFORMED])
def test_malformed_line_is_an_error_with_its_number(tmp_path, bad, what):
    text = "# header\nchr1\t10\t20\n\n" + bad + "\nchr1\t30\t40\n"   # the bad line is line 4
    p = write(tmp_path, text)
    with pytest.raises(api.RsiError) as e:
        api.read_exclude_bed(p, "chr1", N)
    assert e.value.code < 0 and "line 4" in str(e.value), (what, str(e.value))
    lib = api.load_library()
    assert lib.rsi_exclude_read_bed(p.encode(), b"chr1", N, None, None, 0) < 0
    assert b"line 4" in lib.rsi_hot_last_error(None)


def test_missing_file_and_bad_arguments(tmp_path):
    lib = api.load_library()
    assert lib.rsi_exclude_read_bed(str(tmp_path / "nope.bed").encode(), b"chr1", N, None, None, 0) < 0
    assert lib.rsi_exclude_read_bed(None, b"chr1", N, None, None, 0) < 0
    assert lib.rsi_exclude_read_bed(write(tmp_path, BED).encode(), b"chr1", -1, None, None, 0) < 0


def test_set_exclude_needs_a_context():
    lib = api.load_library()
    s = np.array([1], dtype=np.int64)
    assert lib.rsi_hot_set_exclude(None, s.ctypes.data, s.ctypes.data, 1) == -2


def test_symbols_are_exported():
    for name in ("rsi_hot_set_exclude", "rsi_exclude_read_bed", "rsi_hot_debug_classify"):
        assert name in api.EXPORTS and hasattr(api.load_library(), name)
