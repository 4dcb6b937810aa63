"""CPU: the deflate decoder of the device inflate kernel (rsicnv_amd/csrc/inflate_core.h) built as plain C++ under
AddressSanitizer + UndefinedBehaviorSanitizer (tests/sanitize_inflate).  It must inflate every case the GPU test uses exactly
as zlib does, and on thousands of damaged members return an error or the original text, with no sanitizer report."""
import os
import shutil
import subprocess

import pytest

import bgzf_util as bz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "tests", "sanitize_inflate", "inflate_harness")
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
    r = subprocess.run(["make", "-f", "tests/sanitize_inflate/Makefile"], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return HARNESS


def _clean(r):
    return "Sanitizer" not in r.stderr and "runtime error" not in r.stderr


@pytest.mark.timeout(300)
@pytest.mark.parametrize("case", bz.inflate_cases(), ids=lambda c: c[0])
def test_decoder_equals_zlib(harness, tmp_path, case):
    name, data, text = case
    src, out = tmp_path / "in.gz", tmp_path / "out.txt"
    src.write_bytes(data)
    r = subprocess.run([harness, "inflate", str(src), str(out)], capture_output=True, text=True, env=ENV, timeout=250)
    assert r.returncode == 0 and "inflate ok" in r.stdout and _clean(r), r.stdout[-1000:] + r.stderr[-3000:]
    assert out.read_bytes() == text


@pytest.mark.timeout(600)
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_damaged_members_error_or_intact(harness, tmp_path, seed):
    """Bit flips, truncation, wrong ISIZE, random byte runs and random payloads behind a fixed / dynamic block header."""
    text = bz.depth_text(20_000, seed)
    data = (bz.bgzf(text, block=9000) + bz.bgzf(text[:70_000], block=35_000, level=1, strategy=bz.zlib.Z_FIXED) +
            bz.bgzf(os.urandom(5000) + text[:3000], block=4000, level=0) + bz.bgzf(text[:50_000], level=9, strategy=bz.zlib.Z_RLE))
    src = tmp_path / "in.gz"
    src.write_bytes(data)
    r = subprocess.run([harness, "fuzz", str(src), str(seed), "4000"], capture_output=True, text=True, env=ENV, timeout=550)
    assert r.returncode == 0 and "fuzz ok" in r.stdout and _clean(r), r.stdout[-1000:] + r.stderr[-3000:]
    # the damage reached the decoder, not only the CRC check
    assert "invalid Huffman code" in r.stdout and "CRC32 mismatch" in r.stdout, r.stdout
