#!/usr/bin/env python3
"""tests/golden/plot_edges.npz: the gnuplot data (.dat) and script (.gp) files the REFERENCE's own plot_icnv (plotcnv.cpp:246-610,
inside oracle/_ref/libref.so, through ref_plot_icnv of oracle/ref_driver.cpp) writes for every plannable call of every case of
tests/plot_cases.py that qualifies: the reference's _median allocates a counter per unit of the array's span, so an array
qualifies only below a span of 10^6 -- all but the two wide-value cases do; one of the four wide walks is left out to keep the
file small.  The arrays are not stored: the cases rebuild them from their seeds.  A call the planner refuses has no entry (the
reference draws an empty frame or returns early there), nor has a call without a back piece whose walk reaches its own start: the
reference then reads its running mean one past the end, and its bounds-checked Array ends the process.  Runs only where the reference exists; the file holds data (parameters,
the reference's output text, LZMA-compressed: plot_cases.pack), never reference source.
  python tools/make_golden_plot_edges.py"""
import ctypes as C
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import oracle
    import plot_cases as pc
    R = oracle.Ref()
    L = R.lib
    L.ref_plot_icnv.argtypes = [C.POINTER(oracle.Params), C.POINTER(C.c_int32), C.c_int32, C.POINTER(oracle.Call), C.c_char_p, C.c_char_p, C.c_char_p,
                                C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(C.c_double)]
    p = oracle.make_params()
    assert (p.m, p.minmlen, p.chklen) == (pc.M, pc.MINMLEN, pc.CHKLEN)
    out = {"params": np.array([p.m, p.minmlen, p.chklen])}
    version = None
    with tempfile.TemporaryDirectory() as d:
        cwd = os.getcwd()
        os.chdir(d)
        os.makedirs("plots")
        try:
            for name, case in pc.cases().items():
                rd = case.build()
                span = int(rd.max()) - int(rd.min())
                if not case.golden:
                    print(f"{name}: left out (span {span})")
                    continue
                assert span < 10 ** 6, (name, span)
                for k, (s, e, t) in enumerate(case.calls):
                    P = pc.plan(s, e, case.n)
                    if not isinstance(P, dict) or P["past"]:   # refused; or the reference's own bounds check ends the process there
                        continue
                    c = oracle.Call()
                    c.start, c.end, c.type, c.length, c.p1 = s, e, t, abs(e - s) + 1, pc.p1_of(k)
                    base = pc.base_of(s, e, t)
                    res = (C.c_double * 2)()
                    rc = L.ref_plot_icnv(C.byref(p), rd.ctypes.data_as(C.POINTER(C.c_int32)), case.n, C.byref(c), b"chrS", pc.title_of(s, e, t).encode(), b"ps",
                                         (base + ".dat").encode(), (base + ".gp").encode(), (base + ".ps").encode(),
                                         (base + ".dat.keep").encode(), (base + ".gp.keep").encode(), res)
                    assert rc == 0, (name, k, rc)
                    assert not os.path.exists(base + ".dat"), "the reference did not get to the end of plot_icnv"
                    out[f"{name}_{k}_dat"] = pc.pack(open(base + ".dat.keep").read())
                    out[f"{name}_{k}_gp"] = pc.pack(open(base + ".gp.keep").read())
                    out[name + "_rdmed"] = np.array([res[0]])
                    assert version in (None, res[1])
                    version = res[1]
                    os.unlink(base + ".dat.keep"); os.unlink(base + ".gp.keep")
                print(f"{name}: {sum(1 for key in out if key.startswith(name + '_') and key.endswith('_dat'))} calls")
        finally:
            os.chdir(cwd)
    out["version"] = np.array([version])
    path = os.path.join(ROOT, "tests", "golden", "plot_edges.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
