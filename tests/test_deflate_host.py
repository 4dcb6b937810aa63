"""CPU: the deflate coder of the device kernel k_deflate_bgzf (rsicnv_amd/csrc/deflate_core.h, one lane) and the BGZF join of the
command line's part files (track_host.h), built as stand-alone programs under AddressSanitizer + UndefinedBehaviorSanitizer
(tests/sanitize_deflate).  zlib must take every stream back as the text it was made from; the code lengths must stay within
their limit and complete; no sanitizer report."""
import os
import shutil
import subprocess
from fractions import Fraction

import pytest

import bgzf_walk as bw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "sanitize_deflate")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    tmp = tmp_path_factory.mktemp("probe")
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", str(tmp / "probe")], input=b"int main(){return 0;}",
                           capture_output=True)
    if probe.returncode != 0:
        pytest.skip("g++ cannot link the sanitizer runtimes here")
    r = subprocess.run(["make", "-f", "tests/sanitize_deflate/Makefile"], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return os.path.join(DIR, "deflate_harness")


def _clean(r):
    return "Sanitizer" not in r.stderr and "runtime error" not in r.stderr


def deflate(harness, tmp_path, text):
    src, out = tmp_path / "in.txt", tmp_path / "out.gz"
    src.write_bytes(text)
    r = subprocess.run([harness, "deflate", str(src), str(out)], capture_output=True, text=True, env=ENV, timeout=250)
    assert r.returncode == 0 and "deflate ok" in r.stdout and _clean(r), r.stdout[-1000:] + r.stderr[-3000:]
    words = r.stdout.split()
    return out.read_bytes(), int(words[words.index("members") + 1]), int(words[words.index("stored") + 1])


@pytest.mark.timeout(300)
@pytest.mark.parametrize("case", bw.length_cases() + bw.content_cases(), ids=lambda c: c[0])
def test_zlib_takes_the_stream_back(harness, tmp_path, case):
    name, text = case
    data, nmembers, _ = deflate(harness, tmp_path, text)
    ms = bw.check_file(data, text, eof=False)
    assert len(ms) == nmembers == -(-len(text) // bw.MEMBER_TEXT)
    assert all(len(m["text"]) == bw.MEMBER_TEXT for m in ms[:-1])


@pytest.mark.timeout(300)
def test_empty_text_and_random_bytes(harness, tmp_path):
    assert deflate(harness, tmp_path, b"") == (b"", 0, 0)
    rand = os.urandom(bw.MEMBER_TEXT)
    data, nmembers, stored = deflate(harness, tmp_path, rand)
    ms = bw.check_file(data, rand, eof=False)
    assert (nmembers, stored) == (1, 1) and ms[0]["btype"] == 0 and len(data) == bw.MEMBER_TEXT + 5 + 26


@pytest.mark.timeout(300)
@pytest.mark.parametrize("name,text", [("poisson", bw.poisson_text), ("ten_digit", bw.ten_digit_text)])
def test_size_condition(harness, tmp_path, name, text):
    """Smaller than zlib's Huffman-only coding of the same members: matches are found and the codes fit the text."""
    t = text()
    data, _, stored = deflate(harness, tmp_path, t)
    bw.check_file(data, t, eof=False)
    print(f"{name}: text {len(t)} file {len(data)} cap {bw.size_cap(t)} level1 {bw.zlib_bytes(t, 1)} level6 {bw.zlib_bytes(t, 6)}")
    assert stored == 0 and len(data) < bw.size_cap(t)


def test_same_text_same_bytes(harness, tmp_path):
    t = bw.poisson_text()[:150_000]
    assert deflate(harness, tmp_path, t)[0] == deflate(harness, tmp_path, t)[0]


# ---- code lengths ----

def lengths(harness, maxbits, counts):
    r = subprocess.run([harness, "lengths", str(maxbits)] + [str(c) for c in counts], capture_output=True, text=True, env=ENV, timeout=100)
    assert r.returncode == 0 and r.stdout.startswith("lengths") and _clean(r), r.stdout[-1000:] + r.stderr[-3000:]
    ls = [int(x) for x in r.stdout.split()[1:]]
    assert len(ls) == len(counts)
    return ls


def kraft(ls):
    return sum(Fraction(1, 2**l) for l in ls if l)


def fibonacci(n):
    f = [1, 1]
    while len(f) < n:
        f.append(f[-1] + f[-2])
    return f


def huffman_depth(counts):
    """Depth of the unrestricted Huffman tree (to show that a case does need the limit)."""
    import heapq
    h = [(c, 0) for c in counts if c]
    heapq.heapify(h)
    while len(h) > 1:
        a, b = heapq.heappop(h), heapq.heappop(h)
        heapq.heappush(h, (a[0] + b[0], max(a[1], b[1]) + 1))
    return h[0][1]


DEEP = {
    "fibonacci30": fibonacci(30),
    "fibonacci30_reversed_with_gaps": [c for f in reversed(fibonacci(30)) for c in (f, 0)],
    "286_ones_and_one_huge": [1] * 285 + [1 << 30],
    "doubling_286": [1 << (i // 12) for i in range(286)],
}


@pytest.mark.parametrize("name", sorted(DEEP))
def test_lengths_are_limited_and_complete(harness, name):
    counts = DEEP[name]
    ls = lengths(harness, 15, counts)
    assert max(ls) <= 15 and kraft(ls) == 1
    assert all((l == 0) == (c == 0) for l, c in zip(ls, counts))
    if name.startswith("fibonacci"):
        assert huffman_depth(counts) > 15
    # a more frequent symbol never has the longer code
    used = sorted((c, l) for c, l in zip(counts, ls) if c)
    assert all(a[1] >= b[1] for a, b in zip(used, used[1:]) if a[0] < b[0])


def test_code_length_code_stays_within_seven(harness):
    counts = fibonacci(19)
    assert huffman_depth(counts) > 7
    ls = lengths(harness, 7, counts)
    assert max(ls) == 7 and kraft(ls) == 1 and all(ls)


def test_an_unlimited_tree_is_huffmans(harness):
    counts = [5, 9, 12, 13, 16, 45, 0, 0]
    ls = lengths(harness, 15, counts)
    assert ls == [4, 4, 3, 3, 3, 1, 0, 0]


def test_one_and_two_used_symbols(harness):
    """What zlib accepts: a single code of length 1 (incomplete, allowed), two codes of length 1 (complete)."""
    assert lengths(harness, 15, [0, 0, 7, 0]) == [0, 0, 1, 0]
    assert lengths(harness, 15, [0, 3, 0, 1000000]) == [0, 1, 0, 1]
    assert lengths(harness, 15, [0, 0, 0]) == [0, 0, 0]


# ---- the compressed join ----

@pytest.mark.timeout(120)
def test_compressed_join_ends_in_one_eof_block(harness, tmp_path):
    r = subprocess.run([os.path.join(DIR, "join_harness"), str(tmp_path)], capture_output=True, text=True, env=ENV, timeout=100)
    assert r.returncode == 0 and "bgzf join ok" in r.stdout and _clean(r), r.stdout[-1000:] + r.stderr[-3000:]
    assert os.listdir(tmp_path) == []
