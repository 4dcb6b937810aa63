"""CPU: the C-ABI library loads and exports every symbol include/*.h declares; without a GPU the
product fails loudly (no CPU fallback).  No compute calls here."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_functions(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(rsi_[a-z0-9_]+)\s*\(", txt)))


def test_every_declared_symbol_is_exported(hotlib):
    from rsicnv_amd import api
    names = declared_functions("rsi_hot.h") + declared_functions("rsi_synth.h")
    assert len(names) >= 25
    missing = [n for n in names if not hasattr(hotlib, n)]
    assert not missing, f"librsi_hot.so lacks: {missing}"
    assert set(api.EXPORTS) <= set(names)
    assert "rsi_hot_debug_per_base" in names and "rsi_hot_debug_per_base" in api.EXPORTS
    for hook in ("rsi_hot_debug_segments", "rsi_hot_debug_sharpen", "rsi_hot_debug_nb_transform", "rsi_hot_debug_filterstatus",
                 "rsi_hot_debug_candidate_tests", "rsi_hot_debug_range_sums", "rsi_hot_debug_block_stage", "rsi_hot_debug_merge",
                 "rsi_hot_debug_calls"):
        assert hook in names and hook in api.EXPORTS


def test_struct_layouts_match_header(hotlib):
    from rsicnv_amd import api
    assert C.sizeof(api.RsiParams) == 6 * 4 + 7 * 8
    assert C.sizeof(api.RsiCall) == 8 * 4 + 8 * 8
    hdr = open(os.path.join(ROOT, "include", "rsi_hot.h")).read()
    body = re.search(r"typedef struct rsi_cand_record \{(.*?)\} rsi_cand_record;", hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [(ty, re.sub(r"\[\d+\]", "", nm.strip())) for ty, names in re.findall(r"(int32_t|double)\s+([^;]+);", body) for nm in names.split(",")]
    assert [nm for _, nm in fields] == list(api.CAND_RECORD.names)          # the same fields in the same order
    assert all((ty == "int32_t") == (api.CAND_RECORD[nm].base == "int32") for ty, nm in fields)
    assert api.CAND_RECORD.itemsize == 18 * 4 + 17 * 8 and api.CAND_RECORD.fields["body_q"][1] == 18 * 4
    p = api.RsiParams()
    hotlib.rsi_default_params(C.byref(p))
    assert (p.m, p.gcadjust, p.trans, p.merge, p.maxchkbp, p.cap, p.epsilon, p.chklen, p.minmlen, p.buffer, p.p) == \
        (101, 1, 0, 1, 100000, 4.0, 1.5, 2.5, 3.01, 0.05, 0.05)      # rsi.cpp:34-98
    assert api.make_params(m=100).m == 101                             # rsi.cpp:2061-2064


def test_no_cpu_fallback(hotlib):
    """With no HIP device the context cannot be created and says why; with one it can."""
    from rsicnv_amd import api
    try:
        h = api.RsiHot(0)
    except api.RsiError as e:
        assert e.code == -1 and "no CPU fallback" in str(e)
    else:
        h.close()


def test_cli_binary_exists_and_prints_usage():
    import subprocess
    exe = os.path.join(ROOT, "rsicnv_amd", "bin", "rsicnv")
    assert os.path.exists(exe), "build with make -f rsicnv_amd/csrc/Makefile"
    r = subprocess.run([exe], capture_output=True, text=True)
    assert "rsicnv rsi <options> [-b BAMFILE | -d RDFILE -c RNAME ] -f REFFILE" in r.stderr
