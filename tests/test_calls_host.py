"""CPU: the tester-less path of the three list stages (test_block_segments, merge_neighbours, call_from_segments of host_calls.cpp) on
every case of tests/calls_cases.py, in a stand-alone program under ASan + UBSan (tests/calls_harness.cpp, never loaded into Python): the
block cases through the dense and the sparse status form -- whose packed values end with the last run, so a look-up outside the runs
that read them would be an error -- and every list against the restatement (tests/calls_cases.py, pinned to the compiled reference by
tests/test_calls_cases.py): integers and grid-valued columns bit for bit, p1, cnvsd and score at 1e-6."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import calls_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
CALL = np.dtype([(k, np.int32) for k in ("start", "end", "type", "geno", "status", "length", "qscore", "pad")] +
                [(k, np.float64) for k in ("score", "p1", "cnvmed", "cnvsd", "cnviqr", "refmed", "refsd", "refiqr")])
STAGE = dict(block=0, merge=1, calls=2)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    tmp = tmp_path_factory.mktemp("calls_harness")
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", str(tmp / "probe")], input=b"int main(){return 0;}",
                           capture_output=True)
    if probe.returncode != 0:
        pytest.skip("g++ cannot link the sanitizer runtimes here")
    hip = os.environ.get("ROCM_PATH", "/opt/rocm")
    if not os.path.exists(os.path.join(hip, "include", "hip", "hip_runtime.h")):
        pytest.skip("no HIP headers")
    exe = str(tmp / "calls_harness")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                        "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", f"-I{hip}/include", os.path.join(ROOT, "tests", "calls_harness.cpp"),
                        os.path.join(ROOT, "rsicnv_amd", "csrc", "host_calls.cpp"), "-o", exe, f"-L{hip}/lib", "-lamdhip64", f"-Wl,-rpath,{hip}/lib",
                        "-lpthread"], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def records(L):
    out = np.zeros(len(L), dtype=CALL)
    for i, c in enumerate(L):
        for k in K.FIELDS:
            out[i][k] = c[k]
    return out


def jobs():
    """(case, sparse) in the order they are written."""
    return [(c, s) for c in K.all_cases() for s in ((0, 1) if c.stage == "block" else (0,))]


def write_cases(path):
    with open(path, "wb") as f:
        J = jobs()
        f.write(struct.pack("<i", len(J)))
        for c, sparse in J:
            P = c.P
            f.write(struct.pack("<9i", STAGE[c.stage], c.depth.size, len(c.cands), len(c.noncode), c.span_all, sparse, P["m"], P["maxchkbp"], P["merge"]))
            f.write(struct.pack("<6d", P["minmlen"], P["chklen"], P["buffer"], P["p"], c.RDmedian, c.RDsd))
            f.write(np.ascontiguousarray(c.depth, dtype="<i4").tobytes())
            if c.stage == "block":
                f.write(np.ascontiguousarray(c.status, dtype="<i4").tobytes())
            f.write(records(c.cands).tobytes())
            f.write(np.ascontiguousarray(c.noncode, dtype="<i4").tobytes())


def read_lists(path):
    buf = open(path, "rb").read()
    at, out = 0, []
    while at < len(buf):
        n = struct.unpack_from("<i", buf, at)[0]
        out.append(np.frombuffer(buf, dtype=CALL, count=n, offset=at + 4))
        at += 4 + n * CALL.itemsize
    return out


def check(got, want, tag):
    assert len(got) == len(want), (tag, len(got), len(want))
    for i, w in enumerate(want):
        for k in K.EXACT:
            assert got[i][k].item() == w[k], (tag, i, k, got[i][k].item(), w[k])
        for k in K.CLOSE:
            assert np.isclose(got[i][k].item(), w[k], rtol=1e-6, atol=1e-300), (tag, i, k, got[i][k].item(), w[k])


def test_host_path_of_every_case_under_the_sanitizers(harness, tmp_path):
    cases, out = str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")
    write_cases(cases)
    r = subprocess.run([harness, cases, out], capture_output=True, text=True, env=ENV, timeout=600)
    assert r.returncode == 0 and not r.stderr, r.stdout[-1500:] + r.stderr[-3000:]
    lists = read_lists(out)
    at = 0
    golden = K.load_golden()
    for c, sparse in jobs():
        want = K.restated(c, tester=False)
        for part in ((want[0],) if c.stage != "calls" else want[:3]):
            check(lists[at], part, (c.name, c.claim, sparse))
            at += 1
        if c.stage == "calls" and len(c.noncode):      # the calls' coordinates against the reference's own expand_coordinate
            back = dict(zip(*(a.tolist() for a in golden[c.name]["expand"])))
            alive = [x for x in want[-1]["tested"] if x["status"] != -9]
            got = lists[at - 2]
            assert [(int(x["start"]), int(x["end"])) for x in got] == [(back[x["start"]], back[x["end"]]) for x in alive], c.name
    assert at == len(lists)
