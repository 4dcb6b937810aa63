"""CPU: the host side of the per-bin track (rsicnv_amd/csrc/track_host.h: the slice plan over bins, the region table, twice the
chromosome's median as an integer) built as a stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer
(tests/sanitize_bintrack) and run through its checks, with no sanitizer report."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "tests", "sanitize_bintrack", "bintrack_harness")
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
    r = subprocess.run(["make", "-f", "tests/sanitize_bintrack/Makefile"], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return HARNESS


@pytest.mark.timeout(120)
def test_bin_track_host_side_under_sanitizers(harness):
    r = subprocess.run([harness], capture_output=True, text=True, env=ENV, timeout=100)
    assert r.returncode == 0 and "bin track host ok" in r.stdout, r.stdout[-1000:] + r.stderr[-3000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
