"""ctypes bindings for the CPU checkers (TEST INFRASTRUCTURE ONLY).

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may import this package;
the product (rsicnv_amd/) never does.

* ``Oracle``  -- oracle/librsi_oracle.so, the CPU restatement (oracle/rsi_oracle.cpp).
* ``Ref``     -- oracle/_ref/libref.so, the real reference compiled by oracle/Makefile.ref with
                 the stage driver oracle/ref_driver.cpp.  Single global session (the reference
                 keeps its state in globals), so use one instance at a time.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
ORACLE_SO = os.path.join(_HERE, "librsi_oracle.so")
REF_SO = os.path.join(_HERE, "_ref", "libref.so")
REF_BIN = os.path.join(_HERE, "_ref", "rsicnv_ref")


class Params(C.Structure):
    """Same layout as orc_params / ref_params."""
    _fields_ = [("m", C.c_int32), ("gcadjust", C.c_int32), ("trans", C.c_int32), ("merge", C.c_int32),
                ("maxchkbp", C.c_int32), ("debug", C.c_int32), ("cap", C.c_double), ("epsilon", C.c_double),
                ("threshold", C.c_double), ("chklen", C.c_double), ("minmlen", C.c_double),
                ("buffer", C.c_double), ("p", C.c_double)]


class Call(C.Structure):
    _fields_ = [("start", C.c_int32), ("end", C.c_int32), ("type", C.c_int32), ("geno", C.c_int32),
                ("status", C.c_int32), ("length", C.c_int32), ("qscore", C.c_int32), ("pad", C.c_int32),
                ("score", C.c_double), ("p1", C.c_double), ("cnvmed", C.c_double), ("cnvsd", C.c_double),
                ("cnviqr", C.c_double), ("refmed", C.c_double), ("refsd", C.c_double), ("refiqr", C.c_double)]


class ScanScalars(C.Structure):
    _fields_ = [("tmedian1", C.c_double), ("tsigma1", C.c_double), ("tlamda1", C.c_double),
                ("tmedian2", C.c_double), ("tsigma2", C.c_double), ("tlamda2", C.c_double),
                ("target_tlamda", C.c_double), ("Lmax", C.c_int32), ("cal_max", C.c_int32),
                ("stepwise_matches_reference", C.c_int32), ("nseg", C.c_int32)]


CALL_FIELDS = [f[0] for f in Call._fields_ if f[0] != "pad"]


def calls_to_dicts(arr, n):
    return [{k: getattr(arr[i], k) for k in CALL_FIELDS} for i in range(n)]


def make_params(m=101, gcadjust=1, trans=0, merge=1, maxchkbp=100000, debug=0, cap=4.0, epsilon=1.5,
                threshold=-1.0, chklen=2.5, minmlen=3.01, buffer=0.05, p=0.05):
    """Reference defaults (rsi.cpp:34-98); trans: 0 NBN, 1 MED, 2 ALL.  m is forced odd as
    get_parameters does (rsi.cpp:2061-2064)."""
    if m % 2 != 1:
        m += 1
    return Params(m, gcadjust, trans, merge, maxchkbp, debug, cap, epsilon, threshold, chklen, minmlen, buffer, p)


def _i32(a):
    a = np.ascontiguousarray(a, dtype=np.int32)
    return a, a.ctypes.data_as(C.POINTER(C.c_int32))


def _u8(a):
    a = np.ascontiguousarray(a, dtype=np.uint8)
    return a, a.ctypes.data_as(C.POINTER(C.c_uint8))


class Oracle:
    def __init__(self):
        if not os.path.exists(ORACLE_SO):
            raise RuntimeError(f"{ORACLE_SO} missing: run `make -f oracle/Makefile` (or __graft_entry__.build())")
        L = self.lib = C.CDLL(ORACLE_SO)
        L.orc_create.restype = C.c_void_p
        L.orc_destroy.argtypes = [C.c_void_p]
        L.orc_run.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.c_int32, C.c_int32]
        L.orc_run.restype = C.c_int
        L.orc_run_per_base.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.c_int32]
        L.orc_run_per_base.restype = C.c_int
        for nm, ct in (("orc_get_i32", C.c_int32), ("orc_get_f32", C.c_float), ("orc_get_f64", C.c_double)):
            f = getattr(L, nm)
            f.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(ct), C.c_int64]
            f.restype = C.c_int64
        L.orc_get_calls.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(Call), C.c_int32]
        L.orc_get_calls.restype = C.c_int
        for nm, ct in (("orc_median_i32", C.c_int32), ("orc_median_f32", C.c_float), ("orc_median_f64", C.c_double),
                       ("orc_iqr_i32", C.c_int32), ("orc_iqr_f32", C.c_float), ("orc_exact_median_i32", C.c_int32)):
            f = getattr(L, nm)
            f.argtypes = [C.POINTER(ct), C.c_int64]
            f.restype = C.c_double
        L.orc_pnorm.argtypes = [C.c_double]
        L.orc_pnorm.restype = C.c_double
        self.h = C.c_void_p(L.orc_create())

    def __del__(self):
        try:
            self.lib.orc_destroy(self.h)
        except Exception:
            pass

    def run(self, params, depth, fasta, snapshots=True):
        d, dp = _i32(depth)
        f, fp = _u8(fasta)
        assert d.shape == f.shape
        return self.lib.orc_run(self.h, C.byref(params), dp, fp, d.size, 1 if snapshots else 0)

    def run_per_base(self, params, depth, fasta):
        """The per-base stages alone: rd_gc, rd_cap, rd_concat, noncode, binmedint and the "chrom" scalars; returns the bins."""
        d, dp = _i32(depth)
        f, fp = _u8(fasta)
        assert d.shape == f.shape
        return self.lib.orc_run_per_base(self.h, C.byref(params), dp, fp, d.size)

    def _get(self, fn, ct, dt, name):
        n = fn(self.h, name.encode(), None, 0)
        if n < 0:
            raise KeyError(name)
        out = np.zeros(n, dtype=dt)
        fn(self.h, name.encode(), out.ctypes.data_as(C.POINTER(ct)), n)
        return out

    def i32(self, name):
        return self._get(self.lib.orc_get_i32, C.c_int32, np.int32, name)

    def f32(self, name):
        return self._get(self.lib.orc_get_f32, C.c_float, np.float32, name)

    def f64(self, name):
        return self._get(self.lib.orc_get_f64, C.c_double, np.float64, name)

    def calls(self, which="calls"):
        n = self.lib.orc_get_calls(self.h, which.encode(), None, 0)
        arr = (Call * max(n, 1))()
        self.lib.orc_get_calls(self.h, which.encode(), arr, n)
        return calls_to_dicts(arr, n)

    # numeric-utility probes
    def median(self, x):
        x = np.ascontiguousarray(x)
        fn, ct = {np.dtype(np.int32): (self.lib.orc_median_i32, C.c_int32),
                  np.dtype(np.float32): (self.lib.orc_median_f32, C.c_float),
                  np.dtype(np.float64): (self.lib.orc_median_f64, C.c_double)}[x.dtype]
        return fn(x.ctypes.data_as(C.POINTER(ct)), x.size)

    def iqr(self, x):
        x = np.ascontiguousarray(x)
        fn, ct = {np.dtype(np.int32): (self.lib.orc_iqr_i32, C.c_int32),
                  np.dtype(np.float32): (self.lib.orc_iqr_f32, C.c_float)}[x.dtype]
        return fn(x.ctypes.data_as(C.POINTER(ct)), x.size)

    def exact_median(self, x):
        x = np.ascontiguousarray(x, dtype=np.int32)
        return self.lib.orc_exact_median_i32(x.ctypes.data_as(C.POINTER(C.c_int32)), x.size)

    def pnorm(self, x):
        return self.lib.orc_pnorm(x)


def ref_available():
    return os.path.exists(REF_SO)


class Ref:
    """The compiled reference behind oracle/ref_driver.cpp."""

    def __init__(self):
        if not ref_available():
            raise RuntimeError(f"{REF_SO} missing: needs /root/reference and `make -f oracle/Makefile.ref`")
        L = self.lib = C.CDLL(REF_SO)
        L.ref_load.argtypes = [C.POINTER(Params), C.POINTER(C.c_int32), C.c_char_p, C.c_int32, C.c_char_p, C.c_char_p]
        L.ref_get_rd.argtypes = [C.POINTER(C.c_int32), C.c_int32]
        if self.has_load_text():   # a libref.so built from an older ref_driver.cpp lacks it; everything else still works
            L.ref_load_text.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(C.c_int32), C.c_int32]
        L.ref_get_noncode.argtypes = [C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int32]
        L.ref_get_chrom_scalars.argtypes = [C.POINTER(C.c_double)]
        L.ref_get_bins.argtypes = [C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_float), C.c_int32]
        L.ref_scan_stepwise.argtypes = [C.c_int, C.POINTER(ScanScalars)]
        L.ref_get_status.argtypes = [C.c_int, C.POINTER(C.c_int32), C.c_int32]
        L.ref_get_segs.argtypes = [C.POINTER(Call), C.c_int32]
        L.ref_stage_blocks.argtypes = [C.POINTER(Call), C.c_int32]
        L.ref_get_calls.argtypes = [C.c_int, C.POINTER(Call), C.c_int32]
        L.ref_format_calls.argtypes = [C.c_char_p, C.c_int32]
        L.ref_run_timed.argtypes = [C.POINTER(Params), C.POINTER(C.c_int32), C.c_char_p, C.c_int32, C.POINTER(C.c_double)]
        for nm, ct in (("ref_median_i32", C.c_int32), ("ref_median_f32", C.c_float), ("ref_median_f64", C.c_double),
                       ("ref_iqr_i32", C.c_int32), ("ref_iqr_f32", C.c_float), ("ref_exact_median_i32", C.c_int32)):
            f = getattr(L, nm)
            f.argtypes = [C.POINTER(ct), C.c_int64]
            f.restype = C.c_double
        L.ref_pnorm.argtypes = [C.c_double]
        L.ref_pnorm.restype = C.c_double
        L.ref_runmean_f32.argtypes = [C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int32, C.c_int32]
        if hasattr(L, "ref_rsistatus"):   # a libref.so built from an older ref_driver.cpp lacks it
            L.ref_rsistatus.argtypes = [C.POINTER(C.c_float), C.POINTER(C.c_int32), C.c_int32, C.c_double, C.c_double, C.c_double,
                                        C.c_int32, C.POINTER(C.c_int32)]
            L.ref_rsistatus.restype = None
        if hasattr(L, "ref_get_rsi_segments"):   # likewise
            L.ref_get_rsi_segments.argtypes = [C.POINTER(C.c_float), C.POINTER(C.c_int32), C.c_int32, C.c_double, C.POINTER(C.c_int32),
                                               C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_double), C.c_int32]
            L.ref_optimize_with_derivative.argtypes = [C.POINTER(C.c_int32), C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int32,
                                                       C.c_int32]
            L.ref_optimize_with_derivative.restype = None

        if hasattr(L, "ref_filterstatus"):   # likewise
            L.ref_negative_binomial_transfer.argtypes = [C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.POINTER(C.c_float), C.c_int32]
            L.ref_filterstatus.argtypes = [C.POINTER(C.c_float), C.POINTER(C.c_int32), C.c_int32, C.c_double]
            L.ref_filterstatus.restype = None

        if hasattr(L, "ref_isitcnvwrap"):   # likewise
            ip = C.POINTER(C.c_int32)
            L.ref_isitcnvwrap.argtypes = [C.POINTER(Params), ip, C.c_int32, C.c_int32, C.c_double, ip, ip, ip, ip, C.c_int32, C.c_int32,
                                          C.POINTER(Call)]

        if hasattr(L, "ref_areblockscnv"):   # likewise
            ip, cp = C.POINTER(C.c_int32), C.POINTER(Call)
            L.ref_areblockscnv.argtypes = [C.POINTER(Params), ip, ip, C.c_int32, C.c_int32, C.c_double, cp, C.c_int32]
            L.ref_mergesegments.argtypes = [C.POINTER(Params), ip, C.c_int32, C.c_double, cp, C.c_int32, cp, C.c_int32]
            L.ref_isitcnvwrap_in_order.argtypes = [C.POINTER(Params), ip, C.c_int32, C.c_int32, C.c_double, cp, C.c_int32, C.c_int32]
            L.ref_expand_coordinate.argtypes = [ip, ip, C.c_int32, ip, C.c_int32, ip]
            L.ref_expand_coordinate.restype = None
            L.ref_sd_filters.argtypes = [C.c_int32, C.c_double, C.c_double, cp, C.c_int32, cp, C.c_int32]

    # ---- the list stages alone: lists travel as sequences of dicts with (some of) CALL_FIELDS, missing fields as cnv_st() leaves them ----
    @staticmethod
    def _list(dicts):
        arr = (Call * max(len(dicts), 1))()
        for i, d in enumerate(dicts):
            arr[i].type, arr[i].p1 = 2, 1.0          # cnv_st(): TYPE_UNKNOWN, p1 = 1
            for k, v in d.items():
                if k in CALL_FIELDS:
                    setattr(arr[i], k, v)
        return arr

    def _need(self, name):
        if not hasattr(self.lib, name):
            raise RuntimeError(f"{REF_SO} predates {name}: rebuild it with `make -f oracle/Makefile.ref`")

    def areblockscnv(self, params, medint, status, span_all, RDmedian, segs):
        """The reference's areblockscnv (rsi.cpp:415-546) on the caller's bin medians, status array and segments: the segments as judged."""
        self._need("ref_areblockscnv")
        m, mp = _i32(medint)
        s, sp = _i32(status)
        arr = self._list(segs)
        if self.lib.ref_areblockscnv(C.byref(params), mp, sp, m.size, int(span_all), float(RDmedian), arr, len(segs)) != 0:
            raise RuntimeError("the reference's Array threw")
        return calls_to_dicts(arr, len(segs))

    def mergesegments(self, params, rd, RDmedian, cands):
        """The reference's mergesegments (rsi.cpp:694-885): the list after both passes."""
        self._need("ref_mergesegments")
        d, dp = _i32(rd)
        arr, out = self._list(cands), (Call * max(len(cands), 1))()
        n = self.lib.ref_mergesegments(C.byref(params), dp, d.size, float(RDmedian), arr, len(cands), out, len(cands))
        if n < 0:
            raise RuntimeError("the reference's Array threw")
        return calls_to_dicts(out, n)

    def isitcnvwrap_in_order(self, params, rd, span_all, RDmedian, cands, k=None):
        """isitcnvwrap for the indices 0 .. k - 1 in order on one list (the final-test loop's stateful part): the list afterwards."""
        self._need("ref_isitcnvwrap_in_order")
        d, dp = _i32(rd)
        arr = self._list(cands)
        k = len(cands) if k is None else k
        if self.lib.ref_isitcnvwrap_in_order(C.byref(params), dp, d.size, int(span_all), float(RDmedian), arr, len(cands), int(k)) != 0:
            raise RuntimeError("the reference's Array threw")
        return calls_to_dicts(arr, len(cands))

    def expand_coordinate(self, noncode, positions):
        """expand_coordinate (rsi.cpp:1524-1551) of every position with the caller's regions as rsi::noncodelist."""
        self._need("ref_expand_coordinate")
        nc = np.asarray(noncode, dtype=np.int32).reshape(-1, 2)
        a, ap = _i32(nc[:, 0])
        b, bp = _i32(nc[:, 1])
        p, pp = _i32(positions)
        out = np.zeros(p.size, dtype=np.int32)
        self.lib.ref_expand_coordinate(ap, bp, a.size, pp, p.size, out.ctypes.data_as(C.POINTER(C.c_int32)))
        return out

    def sd_filters(self, m, RDmedian, RDsd, cands):
        """sd_filters (rsi.cpp:1753-1792): the entries that stay."""
        self._need("ref_sd_filters")
        arr, out = self._list(cands), (Call * max(len(cands), 1))()
        n = self.lib.ref_sd_filters(int(m), float(RDmedian), float(RDsd), arr, len(cands), out, len(cands))
        return calls_to_dicts(out, n)

    def isitcnvwrap(self, params, rd, span_all, RDmedian, cands, idx):
        """The reference's isitcnvwrap + isitcnv (rsi.cpp:101-287) for entry idx of the list cands (int32 [k, 4]: start, end, type,
        status) over the caller's array: the candidate as judged, a dict.  The caller keeps the walks inside the reference's arrays
        (a RuntimeError here says one left them)."""
        if not hasattr(self.lib, "ref_isitcnvwrap"):
            raise RuntimeError(f"{REF_SO} predates ref_isitcnvwrap: rebuild it with `make -f oracle/Makefile.ref`")
        d, dp = _i32(rd)
        c = np.ascontiguousarray(cands, dtype=np.int32).reshape(-1, 4)
        cols = [_i32(c[:, j]) for j in range(4)]
        out = (Call * 1)()
        rc = self.lib.ref_isitcnvwrap(C.byref(params), dp, d.size, int(span_all), float(RDmedian), cols[0][1], cols[1][1], cols[2][1], cols[3][1],
                                      c.shape[0], int(idx), out)
        if rc != 0:
            raise RuntimeError("the reference's Array threw: a walk or the running mean left its array")
        return calls_to_dicts(out, 1)[0]

    def load(self, params, depth, fasta, chrom="chrS", log=None):
        d, dp = _i32(depth)
        f = np.ascontiguousarray(fasta, dtype=np.uint8)
        self._keep = (d, f)
        return self.lib.ref_load(C.byref(params), dp, f.ctypes.data_as(C.c_char_p), d.size, chrom.encode(),
                                 (log or "").encode())

    def has_load_text(self):
        """True when this libref.so has ref_load_text (built from today's oracle/ref_driver.cpp)."""
        return hasattr(self.lib, "ref_load_text")

    def load_text(self, path, fasta_path, chrom="chrS", cap=None):
        """The reference's load_data_from_text on a depth file (GC adjustment and cap off): RD as int32.  The reference
        exits the process when the FASTA's .fai is missing, so that is checked here first."""
        if not self.has_load_text():
            raise RuntimeError(f"{REF_SO} predates ref_load_text: rebuild it with `make -f oracle/Makefile.ref`")
        if not os.path.exists(str(fasta_path) + ".fai"):
            raise FileNotFoundError(f"{fasta_path}.fai")
        cap = int(cap if cap is not None else 1 << 28)
        out = np.zeros(cap, dtype=np.int32)
        n = self.lib.ref_load_text(str(path).encode(), str(fasta_path).encode(), chrom.encode(),
                                   out.ctypes.data_as(C.POINTER(C.c_int32)), cap)
        return out[:n].copy() if n <= cap else self.rd()

    def stage_gc(self):
        return self.lib.ref_stage_gc()

    def stage_cap(self):
        return self.lib.ref_stage_cap()

    def stage_concat(self):
        return self.lib.ref_stage_concat()

    def rd(self):
        n = self.lib.ref_rd_size()
        out = np.zeros(n, dtype=np.int32)
        self.lib.ref_get_rd(out.ctypes.data_as(C.POINTER(C.c_int32)), n)
        return out

    def noncode(self):
        n = self.lib.ref_get_noncode(None, None, 0)
        b = np.zeros(max(n, 1), dtype=np.int32)
        e = np.zeros(max(n, 1), dtype=np.int32)
        self.lib.ref_get_noncode(b.ctypes.data_as(C.POINTER(C.c_int32)), e.ctypes.data_as(C.POINTER(C.c_int32)), n)
        return np.stack([b[:n], e[:n]], axis=1).reshape(-1)

    def chrom_scalars(self):
        out = (C.c_double * 2)()
        self.lib.ref_get_chrom_scalars(out)
        return out[0], out[1]

    def stage_bins(self):
        nb = self.lib.ref_stage_bins()
        med = np.zeros(nb, dtype=np.float32)
        medint = np.zeros(nb, dtype=np.int32)
        nbn = np.zeros(nb, dtype=np.float32)
        self.lib.ref_get_bins(med.ctypes.data_as(C.POINTER(C.c_float)), medint.ctypes.data_as(C.POINTER(C.c_int32)),
                              nbn.ctypes.data_as(C.POINTER(C.c_float)), nb)
        return med, medint, nbn

    def scan(self, use_med=False):
        sc = ScanScalars()
        nb = self.lib.ref_scan_stepwise(1 if use_med else 0, C.byref(sc))
        st = []
        for w in range(3):
            a = np.zeros(nb, dtype=np.int32)
            self.lib.ref_get_status(w, a.ctypes.data_as(C.POINTER(C.c_int32)), nb)
            st.append(a)
        n = self.lib.ref_get_segs(None, 0)
        arr = (Call * max(n, 1))()
        self.lib.ref_get_segs(arr, n)
        return sc, st, calls_to_dicts(arr, n)

    def blocks(self):
        arr = (Call * 65536)()
        n = self.lib.ref_stage_blocks(arr, 65536)
        return calls_to_dicts(arr, n)

    def detect(self):
        self.lib.ref_stage_detect()
        out = []
        for filt in (0, 1):
            n = self.lib.ref_get_calls(filt, None, 0)
            arr = (Call * max(n, 1))()
            self.lib.ref_get_calls(filt, arr, n)
            out.append(calls_to_dicts(arr, n))
        buf = C.create_string_buffer(1 << 20)
        k = self.lib.ref_format_calls(buf, 1 << 20)
        return out[0], out[1], buf.value.decode() if k >= 0 else None

    def run_timed(self, params, depth, fasta):
        d, dp = _i32(depth)
        f = np.ascontiguousarray(fasta, dtype=np.uint8)
        st = (C.c_double * 5)()
        nc = self.lib.ref_run_timed(C.byref(params), dp, f.ctypes.data_as(C.c_char_p), d.size, st)
        return nc, list(st)

    def median(self, x):
        x = np.ascontiguousarray(x)
        fn, ct = {np.dtype(np.int32): (self.lib.ref_median_i32, C.c_int32),
                  np.dtype(np.float32): (self.lib.ref_median_f32, C.c_float),
                  np.dtype(np.float64): (self.lib.ref_median_f64, C.c_double)}[x.dtype]
        return fn(x.ctypes.data_as(C.POINTER(ct)), x.size)

    def iqr(self, x):
        x = np.ascontiguousarray(x)
        fn, ct = {np.dtype(np.int32): (self.lib.ref_iqr_i32, C.c_int32),
                  np.dtype(np.float32): (self.lib.ref_iqr_f32, C.c_float)}[x.dtype]
        return fn(x.ctypes.data_as(C.POINTER(ct)), x.size)

    def exact_median(self, x):
        x = np.ascontiguousarray(x, dtype=np.int32)
        return self.lib.ref_exact_median_i32(x.ctypes.data_as(C.POINTER(C.c_int32)), x.size)

    def pnorm(self, x):
        return self.lib.ref_pnorm(x)

    def runmean(self, y, band):
        y = np.ascontiguousarray(y, dtype=np.float32)
        out = np.zeros_like(y)
        self.lib.ref_runmean_f32(y.ctypes.data_as(C.POINTER(C.c_float)), out.ctypes.data_as(C.POINTER(C.c_float)), y.size, band)
        return out

    def rsistatus(self, T, medint, RDmedian, tmedian, tlamda, Lmax):
        """One scan pass (the reference's rsistatus, rsi.cpp:1191-1259) over the caller's bins: the status array.  The
        reference's trimming walks are unbounded; the caller keeps them inside the arrays."""
        if not hasattr(self.lib, "ref_rsistatus"):
            raise RuntimeError(f"{REF_SO} predates ref_rsistatus: rebuild it with `make -f oracle/Makefile.ref`")
        t = np.ascontiguousarray(T, dtype=np.float32)
        mi, mp = _i32(medint)
        assert t.shape == mi.shape and t.ndim == 1
        out = np.zeros(t.size, dtype=np.int32)
        self.lib.ref_rsistatus(t.ctypes.data_as(C.POINTER(C.c_float)), mp, t.size, float(RDmedian), float(tmedian), float(tlamda),
                               int(Lmax), out.ctypes.data_as(C.POINTER(C.c_int32)))
        return out

    def get_rsi_segments(self, T, status, tmedian):
        """The reference's get_rsi_segments (rsi.cpp:1060-1117) over the caller's bins and status: (start, end, type, score), one entry
        per marked run but the last."""
        if not hasattr(self.lib, "ref_get_rsi_segments"):
            raise RuntimeError(f"{REF_SO} predates ref_get_rsi_segments: rebuild it with `make -f oracle/Makefile.ref`")
        t = np.ascontiguousarray(T, dtype=np.float32)
        st, sp = _i32(status)
        cap = t.size
        s, e, ty = (np.zeros(cap, dtype=np.int32) for _ in range(3))
        sc = np.zeros(cap, dtype=np.float64)
        ip = C.POINTER(C.c_int32)
        k = self.lib.ref_get_rsi_segments(t.ctypes.data_as(C.POINTER(C.c_float)), sp, t.size, float(tmedian), s.ctypes.data_as(ip),
                                          e.ctypes.data_as(ip), ty.ctypes.data_as(ip), sc.ctypes.data_as(C.POINTER(C.c_double)), cap)
        return s[:k].copy(), e[:k].copy(), ty[:k].copy(), sc[:k].copy()

    def negative_binomial_transfer(self, rd, m):
        """The reference's negative_binomial_transfer (rsi.cpp:1120-1188) over the caller's compacted depth: the rd.size // m bins."""
        if not hasattr(self.lib, "ref_negative_binomial_transfer"):
            raise RuntimeError(f"{REF_SO} predates ref_negative_binomial_transfer: rebuild it with `make -f oracle/Makefile.ref`")
        d, dp = _i32(rd)
        out = np.zeros(d.size // int(m), dtype=np.float32)
        k = self.lib.ref_negative_binomial_transfer(dp, d.size, int(m), out.ctypes.data_as(C.POINTER(C.c_float)), out.size)
        assert k == out.size
        return out

    def filterstatus(self, T, status, dev):
        """The reference's filterstatus (rsi.cpp:948-1047) over the caller's bins and status: the filtered status.  The caller sends an
        array with an unmarked level inside its level range: the reference indexes out of range otherwise."""
        if not hasattr(self.lib, "ref_filterstatus"):
            raise RuntimeError(f"{REF_SO} predates ref_filterstatus: rebuild it with `make -f oracle/Makefile.ref`")
        t = np.ascontiguousarray(T, dtype=np.float32)
        st = np.array(status, dtype=np.int32)
        assert st.shape == t.shape and t.ndim == 1
        self.lib.ref_filterstatus(t.ctypes.data_as(C.POINTER(C.c_float)), st.ctypes.data_as(C.POINTER(C.c_int32)), t.size, float(dev))
        return st

    def optimize_with_derivative(self, rd, start, end, type_, calls=2):
        """The reference's optimize_with_derivative (rsi.cpp:889-937), `calls` times, on one candidate: (start, end).  The caller keeps
        end >= start through every call: the reference indexes its vector out of range otherwise."""
        if not hasattr(self.lib, "ref_optimize_with_derivative"):
            raise RuntimeError(f"{REF_SO} predates ref_optimize_with_derivative: rebuild it with `make -f oracle/Makefile.ref`")
        d, dp = _i32(rd)
        s, e = C.c_int32(int(start)), C.c_int32(int(end))
        self.lib.ref_optimize_with_derivative(dp, d.size, C.byref(s), C.byref(e), int(type_), int(calls))
        return s.value, e.value
