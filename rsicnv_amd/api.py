"""ctypes binding of librsi_hot.so (include/rsi_hot.h) -- the drop-in for the reference's
per-chromosome hot path (rsi.cpp:2189-2212).

The library is the product: there is no Python or CPU fallback.  `load_library()` raises if the
shared object is missing, and `RsiHot()` raises if no HIP device can be opened.
"""
import contextlib
import ctypes as C
import os

import numpy as np

# A pool drives one HIP stream per worker.  The ROCm runtime multiplexes streams onto
# GPU_MAX_HW_QUEUES hardware queues (default 4); with a dozen streams that puts unrelated chromosomes
# in line behind each other's kernels (measured: ~10 % of the genome rate).  The variable is read when
# the HIP runtime initialises, so it has to be in the environment before the first HIP call: importing
# this module is that moment for a Python program (librsi_hot.so is loaded later, and need not exist
# for the import).  A lower value that is already there does NOT win -- boxes that start every command
# with GPU_MAX_HW_QUEUES=4 kept a pool of twenty on four queues for three rounds; RSI_HOT_HW_QUEUES
# is how a caller has its way.
POOL_HW_QUEUES, MIN_HW_QUEUES = 32, 4


def _queue_count(s):
    """One to nine decimal digits and nothing else -> the number; anything else -> -1 (parse_queue_count, process_setup.cpp)."""
    return int(s) if s is not None and 1 <= len(s) <= 9 and all(c in "0123456789" for c in s) else -1


def _process_setup(env=os.environ):
    """rsi_hot_process_setup (include/rsi_hot.h) restated: the same policy on `env`, returning what GPU_MAX_HW_QUEUES holds
    afterwards (0: no number).  GPU_MAX_HW_QUEUES below 32, missing or not a number -> 32; 32 or more -> left alone;
    RSI_HOT_HW_QUEUES=keep -> nothing changes; RSI_HOT_HW_QUEUES=N -> N clamped to 4 .. 32 is written."""
    user = env.get("RSI_HOT_HW_QUEUES")
    if user != "keep":
        want = _queue_count(user)
        if want >= 0:
            env["GPU_MAX_HW_QUEUES"] = str(min(POOL_HW_QUEUES, max(MIN_HW_QUEUES, want)))
        elif _queue_count(env.get("GPU_MAX_HW_QUEUES")) < POOL_HW_QUEUES:
            env["GPU_MAX_HW_QUEUES"] = str(POOL_HW_QUEUES)
    return max(0, _queue_count(env.get("GPU_MAX_HW_QUEUES")))


HW_QUEUES = _process_setup()

_HERE = os.path.dirname(os.path.abspath(__file__))
# RSI_HOT_LIB: another build of the same ABI (A/B measurements of library versions, tools/ab_bench.py)
LIB_PATH = os.environ.get("RSI_HOT_LIB") or os.path.join(_HERE, "librsi_hot.so")

RSI_OK = 0
STATUS_NAMES = {0: "RSI_OK", -1: "RSI_ERR_NO_DEVICE", -2: "RSI_ERR_BAD_ARG", -3: "RSI_ERR_HIP",
                -4: "RSI_ERR_TOO_SMALL", -5: "RSI_ERR_UNSUPPORTED", -6: "RSI_ERR_INTERNAL"}

# rsi_cand_record (include/rsi_hot.h): one record of rsi_hot_debug_candidate_tests
CAND_RECORD = np.dtype([(k, np.int32) for k in ("capacity", "top", "margin", "cut", "nleft", "nright", "road", "flags", "nref", "nbody", "nwin",
                                                "left_reach", "right_reach", "body_min", "body_max", "type", "status", "geno")] +
                       [("body_q", np.float64, 3), ("body_s1", np.float64), ("body_s2", np.float64), ("ref_q", np.float64, 3),
                        ("ref_s1", np.float64), ("ref_s2", np.float64)] +
                       [(k, np.float64) for k in ("p1", "cnvmed", "cnvsd", "cnviqr", "refmed", "refsd", "refiqr")])
assert CAND_RECORD.itemsize == 18 * 4 + 17 * 8

# rsi_call (include/rsi_hot.h) as a numpy record: the lists of rsi_hot_debug_block_stage / _merge / _calls
CALL_RECORD = np.dtype([(k, np.int32) for k in ("start", "end", "type", "geno", "status", "length", "qscore", "pad")] +
                       [(k, np.float64) for k in ("score", "p1", "cnvmed", "cnvsd", "cnviqr", "refmed", "refsd", "refiqr")])
assert CALL_RECORD.itemsize == 8 * 4 + 8 * 8
LIST_INFO = ("spec_hits", "single_tests", "host_fallbacks", "block_batch_hits", "waits", "sum_launches", "sum_reused", "sum_redone", "tests")

# rsi_geno_record (include/rsi_hot.h): one line of rsi_hot_geno_calls / rsi_hot_debug_geno
GENO_RECORD = np.dtype([(k, np.int32) for k in ("n_body", "n_flank", "body_min", "body_max")] +
                       [("body_sum", np.int64), ("flank_sum", np.int64), ("body_q", np.float64, 3), ("flank_q", np.float64, 3),
                        ("chrom_median", np.float64)])
assert GENO_RECORD.itemsize == 4 * 4 + 2 * 8 + 7 * 8

# rsi_depth_summary, rsi_depth_region (include/rsi_hot.h): rsi_hot_depth_summary's record, one region of rsi_hot_depth_regions
DEPTH_SUMMARY = np.dtype([(k, np.int64) for k in ("n", "sum", "over", "negative")] + [("min", np.int32), ("max", np.int32)])
DEPTH_REGION = np.dtype([("n", np.int64), ("sum", np.int64), ("min", np.int32), ("max", np.int32)])
assert DEPTH_SUMMARY.itemsize == 40 and DEPTH_REGION.itemsize == 24
DEPTH_BINS = 65536

# every symbol include/rsi_hot.h and include/rsi_synth.h declare
EXPORTS = ["rsi_default_params", "rsi_hot_create", "rsi_hot_destroy", "rsi_hot_last_error", "rsi_hot_run",
           "rsi_hot_run_device", "rsi_hot_load_depth_text", "rsi_hot_run_text", "rsi_hot_load_depth_bam", "rsi_hot_run_bam", "rsi_bam_references", "rsi_result_annotate_bam", "rsi_result_summary", "rsi_summary_format_row", "rsi_summary_format_rows", "rsi_result_pairs", "rsi_result_ncalls", "rsi_result_calls", "rsi_result_stats", "rsi_result_noncode",
           "rsi_result_format_row", "rsi_result_free", "rsi_hot_fetch_i32", "rsi_hot_fetch_f32", "rsi_hot_fetch_i64",
           "rsi_hot_kernel_times", "rsi_hot_phase_times", "rsi_hot_set_timing", "rsi_hot_process_setup", "rsi_pool_create", "rsi_pool_destroy", "rsi_pool_workers", "rsi_pool_hw_queues", "rsi_pool_worker",
           "rsi_pool_set_timing", "rsi_pool_set_timing_kernel", "rsi_hot_set_timing_kernel", "rsi_pool_set_schedule", "rsi_pool_last_error", "rsi_pool_run", "rsi_pool_run_host", "rsi_pool_submit", "rsi_pool_wait", "rsi_plot_expand", "rsi_plot_write_files", "rsi_result_log_line", "rsi_hot_debug_level_sums", "rsi_hot_debug_scan", "rsi_hot_debug_segments", "rsi_hot_debug_sharpen", "rsi_hot_debug_candidate_tests", "rsi_hot_debug_range_sums", "rsi_hot_debug_block_stage", "rsi_hot_debug_merge", "rsi_hot_debug_calls", "rsi_hot_debug_nb_transform", "rsi_hot_debug_nb_keyed", "rsi_hot_debug_filterstatus", "rsi_hot_debug_grid_median", "rsi_hot_debug_grid_mad_i32", "rsi_synth_generate_host", "rsi_synth_generate_device", "rsi_synth_write_depth_text", "rsi_synth_write_fasta", "rsi_synth_append_genome_text",
           "rsi_genome_text_open", "rsi_genome_text_next", "rsi_genome_text_release", "rsi_genome_text_copy_depth",
           "rsi_genome_text_kernel_ms", "rsi_genome_text_close", "rsi_genome_text_last_error", "rsi_hot_run_depth_device",
           "rsi_hot_last_inflate_stats", "rsi_hot_inflate_bgzf", "rsi_genome_text_inflate_stats",
           "rsi_synth_append_genome_bgzf", "rsi_genome_text_open_samples", "rsi_genome_text_samples", "rsi_genome_text_max_resident",
           "rsi_genome_text_sample_depth", "rsi_genome_text_copy_sample_depth", "rsi_synth_append_genome_samples",
           "rsi_genome_bedgraph_open", "rsi_synth_append_genome_bedgraph", "rsi_genome_bedgraph_open_indexed", "rsi_genome_text_index_range",
           "rsi_hot_set_exclude", "rsi_exclude_read_bed", "rsi_hot_debug_classify", "rsi_hot_debug_per_base",
           "rsi_hot_write_track", "rsi_hot_write_track_device", "rsi_hot_debug_track",
           "rsi_hot_write_bin_track", "rsi_hot_debug_bin_track",
           "rsi_hot_set_track_format", "rsi_hot_last_deflate_stats", "rsi_bgzf_write_eof", "rsi_hot_debug_deflate",
           "rsi_track_index_create", "rsi_track_index_free", "rsi_hot_set_track_index", "rsi_track_index_append",
           "rsi_track_index_write_tbi", "rsi_track_index_counts", "rsi_track_index_debug_tbi",
           "rsi_ref_open", "rsi_ref_close", "rsi_ref_last_error", "rsi_ref_count", "rsi_ref_sequence", "rsi_ref_find", "rsi_ref_format",
           "rsi_ref_index_path", "rsi_ref_load_device", "rsi_ref_load_host", "rsi_ref_device_alloc", "rsi_ref_device_free",
           "rsi_hot_run_text_dfasta", "rsi_hot_run_bam_dfasta",
           "rsi_hot_set_bam_read", "rsi_hot_last_bam_read_stats",
           "rsi_hot_set_bam_pairs", "rsi_result_annotate_device", "rsi_hot_last_pairs_stats", "rsi_hot_debug_pair_sample",
           "rsi_hot_debug_pair_annotate",
           "rsi_hot_set_bam_pin", "rsi_hot_stat_calls", "rsi_hot_pin_sample", "rsi_hot_pin_calls", "rsi_hot_last_pin_stats",
           "rsi_hot_debug_pin_sample", "rsi_hot_debug_pin_calls",
           "rsi_hot_geno_calls", "rsi_hot_last_geno_stats", "rsi_hot_debug_geno",
           "rsi_hot_loaded_depth", "rsi_hot_depth_summary", "rsi_hot_depth_regions", "rsi_hot_write_window_track", "rsi_hot_write_region_track",
           "rsi_hot_last_depth_stats", "rsi_hot_debug_depth_summary", "rsi_hot_debug_depth_regions", "rsi_hot_debug_region_track",
           "rsi_plot_batch_new", "rsi_plot_batch_free", "rsi_plot_batch_add", "rsi_plot_batch_add_span", "rsi_plot_batch_size",
           "rsi_plot_batch_refusal", "rsi_plot_refusal_text", "rsi_plot_batch_queries", "rsi_plot_batch_fill_host",
           "rsi_plot_batch_chrom_median", "rsi_plot_batch_compare", "rsi_plot_batch_write", "rsi_hot_plot_depth", "rsi_hot_plot_run", "rsi_hot_last_plot_stats",
           "rsi_hot_debug_plot", "rsi_hot_debug_plot_expand",
           "rsi_ref_debug_set_chunks", "rsi_ref_debug_fai_line", "rsi_ref_debug_ranges", "rsi_ref_debug_gzi", "rsi_ref_debug_cover"]


class RsiParams(C.Structure):
    _fields_ = [("m", C.c_int32), ("gcadjust", C.c_int32), ("trans", C.c_int32), ("merge", C.c_int32),
                ("maxchkbp", C.c_int32), ("debug", C.c_int32), ("cap", C.c_double), ("epsilon", C.c_double),
                ("threshold", C.c_double), ("chklen", C.c_double), ("minmlen", C.c_double),
                ("buffer", C.c_double), ("p", C.c_double)]


class RsiCall(C.Structure):
    _fields_ = [("start", C.c_int32), ("end", C.c_int32), ("type", C.c_int32), ("geno", C.c_int32),
                ("status", C.c_int32), ("length", C.c_int32), ("qscore", C.c_int32), ("pad", C.c_int32),
                ("score", C.c_double), ("p1", C.c_double), ("cnvmed", C.c_double), ("cnvsd", C.c_double),
                ("cnviqr", C.c_double), ("refmed", C.c_double), ("refsd", C.c_double), ("refiqr", C.c_double)]


class RsiChromStats(C.Structure):
    _fields_ = [("n", C.c_int64), ("n_compact", C.c_int64), ("nbins", C.c_int64), ("n_noncode", C.c_int32),
                ("Lmax", C.c_int32), ("gc_rdmean", C.c_double), ("cap_median", C.c_double), ("RDmedian", C.c_double),
                ("RDsd", C.c_double), ("nb_mad", C.c_double), ("nb_r", C.c_double), ("nb_tmin", C.c_double),
                ("tmedian1", C.c_double), ("tsigma1", C.c_double), ("tlamda1", C.c_double), ("tmedian2", C.c_double),
                ("tsigma2", C.c_double), ("tlamda2", C.c_double), ("trim_escapes", C.c_int32),
                ("inexact_sums", C.c_int32), ("t_device_ms", C.c_double), ("t_kernels_ms", C.c_double),
                ("byte_escapes", C.c_int64), ("scan_tiles", C.c_int32), ("scan_tiles_listed", C.c_int32)]


RSI_MAX_TIMED = 64
SUMMARY_HEAD, SUMMARY_CALL = 8, 8   # rsi_hot.h: RSI_SUMMARY_HEAD, RSI_SUMMARY_CALL


class RsiTextStats(C.Structure):
    _fields_ = [("bytes", C.c_int64), ("lines", C.c_int64), ("stored", C.c_int64), ("beyond", C.c_int64),
                ("fallback", C.c_int32), ("pad", C.c_int32), ("t_total_ms", C.c_double), ("t_parse_kernel_ms", C.c_double)]


class RsiInflateStats(C.Structure):
    _fields_ = [("format", C.c_int32), ("eof_block", C.c_int32), ("input_error", C.c_int32), ("pad", C.c_int32), ("compressed_bytes", C.c_int64), ("text_bytes", C.c_int64),
                ("blocks", C.c_int64), ("t_inflate_kernel_ms", C.c_double), ("t_host_inflate_ms", C.c_double)]


class RsiTrackStats(C.Structure):
    _fields_ = [("n", C.c_int64), ("lines", C.c_int64), ("bytes", C.c_int64), ("slices", C.c_int64),
                ("t_total_ms", C.c_double), ("t_kernel_ms", C.c_double), ("t_write_ms", C.c_double)]


class RsiDeflateStats(C.Structure):
    _fields_ = [("members", C.c_int64), ("stored_members", C.c_int64), ("text_bytes", C.c_int64), ("file_bytes", C.c_int64),
                ("t_kernel_ms", C.c_double)]


INFLATE_FORMATS = {0: "text", 1: "bgzf", 2: "gzip"}
TRACK_FORMATS = {"text": 0, "bgzf": 1}


class RsiRefSeq(C.Structure):
    _fields_ = [("length", C.c_int64), ("offset", C.c_int64), ("linebases", C.c_int32), ("linewidth", C.c_int32), ("name", C.c_char * 256)]


class RsiRefStats(C.Structure):
    _fields_ = [("bytes_read", C.c_int64), ("text_bytes", C.c_int64), ("members", C.c_int64), ("format", C.c_int32),
                ("index_used", C.c_int32), ("t_kernel_ms", C.c_double), ("t_wall_ms", C.c_double)]


def _inflate_dict(st):
    d = {f[0]: getattr(st, f[0]) for f in RsiInflateStats._fields_ if f[0] != "pad"}
    d["format"] = INFLATE_FORMATS.get(st.format, str(st.format))
    return d


class RsiGenomeChrom(C.Structure):
    _fields_ = [("slot", C.c_int32), ("pad", C.c_int32), ("n", C.c_int64), ("d_depth", C.c_void_p), ("stats", RsiTextStats),
                ("name", C.c_char * 256)]


class RsiBamStats(C.Structure):
    _fields_ = [("n", C.c_int64), ("bytes_compressed", C.c_int64), ("bytes_inflated", C.c_int64), ("records", C.c_int64), ("on_chrom", C.c_int64),
                ("used", C.c_int64), ("runs", C.c_int64), ("tid", C.c_int32), ("indexed", C.c_int32),
                ("t_total_ms", C.c_double), ("t_inflate_ms", C.c_double), ("t_walk_ms", C.c_double), ("t_wait_ms", C.c_double),
                ("malformed", C.c_int64)]


class RsiBamReadStats(C.Structure):
    _fields_ = [("mode", C.c_int32), ("pad", C.c_int32), ("chunks", C.c_int64), ("members", C.c_int64), ("segments", C.c_int64),
                ("guessed", C.c_int64), ("rewalked", C.c_int64), ("passed", C.c_int64),
                ("t_upload_ms", C.c_double), ("t_inflate_ms", C.c_double), ("t_find_ms", C.c_double)]


class RsiPairsStats(C.Structure):
    _fields_ = [("records", C.c_int64), ("table_bytes", C.c_int64), ("maxspan", C.c_int64), ("sample_count", C.c_int64),
                ("sample_abs", C.c_int64), ("sample_sq", C.c_int64), ("sample_stop", C.c_int64), ("isize", C.c_int32),
                ("isize_sd", C.c_int32), ("calls", C.c_int64), ("examined", C.c_int64),
                ("t_table_ms", C.c_double), ("t_sample_ms", C.c_double), ("t_annotate_ms", C.c_double)]


class RsiPinStats(C.Structure):
    _fields_ = [("records", C.c_int64), ("table_bytes", C.c_int64), ("pool_words", C.c_int64), ("sample_reads", C.c_int64),
                ("pos_start", C.c_int32), ("pos_end", C.c_int32), ("l_qseq", C.c_int32), ("r_len", C.c_int32),
                ("rd", C.c_double), ("rd_sd", C.c_double), ("drd", C.c_double), ("drd_sd", C.c_double), ("breakpoints", C.c_int64),
                ("t_table_ms", C.c_double), ("t_sample_ms", C.c_double), ("t_windows_ms", C.c_double)]


class RsiGenoStats(C.Structure):
    _fields_ = [("launches", C.c_int64), ("jobs", C.c_int64), ("tiles", C.c_int64), ("passes", C.c_int64), ("bytes", C.c_int64),
                ("ms", C.c_double)]


class RsiPlotStats(C.Structure):
    _fields_ = [(k, C.c_int64) for k in ("launches", "batches", "tiles", "calls", "queries", "bytes_up", "bytes_down", "bytes")] + \
               [("ms", C.c_double), ("expand_ms", C.c_double)]


class RsiDepthStats(C.Structure):
    _fields_ = [("launches", C.c_int64), ("workgroups", C.c_int64), ("bytes", C.c_int64), ("ms", C.c_double), ("kernel_ms", C.c_double)]


BAM_READ_MODES = {"host": 0, "device": 1}
BAM_SEGMENT = 16384          # kernels.h, RSI_BAM_SEGMENT: bytes of inflated BAM per segment of the device record finder


class RsiBatchTimes(C.Structure):
    _fields_ = [("nkernels", C.c_int32), ("nphases", C.c_int32), ("kernel_name", C.c_char_p * RSI_MAX_TIMED),
                ("kernel_ms", C.c_double * RSI_MAX_TIMED), ("kernel_launches", C.c_int64 * RSI_MAX_TIMED),
                ("kernel_bases", C.c_int64 * RSI_MAX_TIMED), ("phase_name", C.c_char_p * RSI_MAX_TIMED),
                ("phase_ms", C.c_double * RSI_MAX_TIMED)]


CALL_FIELDS = [f[0] for f in RsiCall._fields_ if f[0] != "pad"]
WHICH = {"calls": 0, "calls_raw": 1, "segs": 2, "blocks": 3}

_lib = None


def load_library():
    """dlopen librsi_hot.so; raises (never falls back) when the extension has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} is missing: build it with `make -f rsicnv_amd/csrc/Makefile` "
                           "(or __graft_entry__.build()); rsicnv_amd has no CPU fallback")
    # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64.so.7 / libhsa-runtime64;
    # if librsi_hot.so were loaded first it would pull /opt/rocm's copy and the second runtime to
    # touch the GPU would fail with "no ROCm-capable device".  Importing torch first makes our
    # DT_NEEDED libamdhip64.so.7 resolve to the copy torch already loaded.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    L.rsi_default_params.argtypes = [C.POINTER(RsiParams)]
    L.rsi_hot_create.argtypes = [C.c_int, C.POINTER(C.c_int)]
    L.rsi_hot_create.restype = C.c_void_p
    L.rsi_hot_destroy.argtypes = [C.c_void_p]
    L.rsi_hot_last_error.argtypes = [C.c_void_p]
    L.rsi_hot_last_error.restype = C.c_char_p
    L.rsi_hot_run.argtypes = [C.c_void_p, C.POINTER(RsiParams), C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_void_p)]
    L.rsi_hot_run_device.argtypes = [C.c_void_p, C.POINTER(RsiParams), C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_void_p)]
    L.rsi_hot_load_depth_text.argtypes = [C.c_void_p, C.c_char_p, C.c_int64, C.POINTER(RsiTextStats)]
    L.rsi_hot_run_text.argtypes = [C.c_void_p, C.POINTER(RsiParams), C.c_char_p, C.c_void_p, C.c_int64, C.POINTER(C.c_void_p), C.POINTER(RsiTextStats)]
    L.rsi_hot_load_depth_bam.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.POINTER(RsiBamStats)]
    L.rsi_hot_run_bam.argtypes = [C.c_void_p, C.POINTER(RsiParams), C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_void_p, C.c_int64,
                                  C.POINTER(C.c_void_p), C.POINTER(RsiBamStats)]
    L.rsi_result_ncalls.argtypes = [C.c_void_p, C.c_int]
    L.rsi_result_calls.argtypes = [C.c_void_p, C.c_int]
    L.rsi_result_calls.restype = C.POINTER(RsiCall)
    L.rsi_result_stats.argtypes = [C.c_void_p]
    L.rsi_result_stats.restype = C.POINTER(RsiChromStats)
    L.rsi_result_noncode.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.c_int]
    L.rsi_result_summary.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    L.rsi_result_summary.restype = C.c_int
    L.rsi_summary_format_row.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_char_p, C.c_int]
    L.rsi_summary_format_row.restype = C.c_int
    L.rsi_summary_format_rows.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_int]
    L.rsi_summary_format_rows.restype = C.c_int
    L.rsi_result_log_line.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_int]
    L.rsi_result_log_line.restype = C.c_int
    L.rsi_result_format_row.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_char_p, C.c_int]
    L.rsi_result_free.argtypes = [C.c_void_p]
    for nm, ct in (("rsi_hot_fetch_i32", C.c_int32), ("rsi_hot_fetch_f32", C.c_float), ("rsi_hot_fetch_i64", C.c_int64)):
        f = getattr(L, nm)
        f.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(ct), C.c_int64]
        f.restype = C.c_int64
    L.rsi_hot_kernel_times.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_float), C.c_int]
    L.rsi_hot_phase_times.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_double), C.c_int]
    L.rsi_hot_set_timing.argtypes = [C.c_void_p, C.c_int]
    L.rsi_pool_create.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_int)]
    L.rsi_pool_create.restype = C.c_void_p
    L.rsi_pool_destroy.argtypes = [C.c_void_p]
    L.rsi_pool_workers.argtypes = [C.c_void_p]
    L.rsi_pool_hw_queues.argtypes = [C.c_void_p]
    L.rsi_hot_process_setup.argtypes = []
    L.rsi_pool_worker.argtypes = [C.c_void_p, C.c_int]
    L.rsi_pool_worker.restype = C.c_void_p
    L.rsi_pool_set_timing.argtypes = [C.c_void_p, C.c_int]
    L.rsi_pool_set_timing_kernel.argtypes = [C.c_void_p, C.c_char_p]
    L.rsi_hot_set_timing_kernel.argtypes = [C.c_void_p, C.c_char_p]
    L.rsi_pool_set_schedule.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.rsi_pool_last_error.argtypes = [C.c_void_p]
    L.rsi_pool_last_error.restype = C.c_char_p
    L.rsi_pool_run.argtypes = [C.c_void_p, C.POINTER(RsiParams), C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                               C.POINTER(C.c_int64), C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.POINTER(RsiBatchTimes)]
    L.rsi_pool_run_host.argtypes = [C.c_void_p, C.POINTER(RsiParams), C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                               C.POINTER(C.c_int64), C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.POINTER(RsiBatchTimes)]
    L.rsi_pool_submit.argtypes = L.rsi_pool_run.argtypes
    L.rsi_pool_submit.restype = C.c_uint64
    L.rsi_pool_wait.argtypes = [C.c_void_p, C.c_uint64]
    L.rsi_hot_run_depth_device.argtypes = [C.c_void_p, C.POINTER(RsiParams), C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_void_p)]
    L.rsi_genome_text_open.argtypes = [C.c_int, C.c_char_p, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int64), C.c_int, C.c_size_t,
                                       C.POINTER(C.c_int)]
    L.rsi_genome_text_open.restype = C.c_void_p
    L.rsi_genome_text_next.argtypes = [C.c_void_p, C.POINTER(RsiGenomeChrom)]
    L.rsi_genome_text_release.argtypes = [C.c_void_p, C.c_int]
    L.rsi_genome_text_copy_depth.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int64]
    L.rsi_genome_text_copy_depth.restype = C.c_int64
    L.rsi_genome_text_kernel_ms.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.rsi_genome_text_close.argtypes = [C.c_void_p]
    L.rsi_genome_text_last_error.argtypes = [C.c_void_p]
    L.rsi_genome_text_last_error.restype = C.c_char_p
    L.rsi_genome_text_inflate_stats.argtypes = [C.c_void_p, C.POINTER(RsiInflateStats)]
    L.rsi_genome_text_open_samples.argtypes = [C.c_int, C.c_char_p, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int64),
                                               C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_size_t, C.POINTER(C.c_int)]
    L.rsi_genome_text_open_samples.restype = C.c_void_p
    L.rsi_genome_text_samples.argtypes = [C.c_void_p]
    L.rsi_genome_text_max_resident.argtypes = [C.c_void_p]
    L.rsi_genome_text_sample_depth.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.rsi_genome_text_sample_depth.restype = C.c_void_p
    L.rsi_genome_text_copy_sample_depth.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int64]
    L.rsi_genome_text_copy_sample_depth.restype = C.c_int64
    L.rsi_synth_append_genome_samples.argtypes = [C.c_char_p, C.c_char_p, C.c_void_p, C.c_int, C.c_int64, C.c_int]
    L.rsi_genome_bedgraph_open.argtypes = L.rsi_genome_text_open.argtypes
    L.rsi_genome_bedgraph_open.restype = C.c_void_p
    L.rsi_genome_bedgraph_open_indexed.argtypes = [C.c_int, C.c_char_p, C.c_char_p, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int64), C.c_int,
                                                   C.c_size_t, C.POINTER(C.c_int)]
    L.rsi_genome_bedgraph_open_indexed.restype = C.c_void_p
    L.rsi_genome_text_index_range.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.rsi_synth_append_genome_bedgraph.argtypes = [C.c_char_p, C.c_char_p, C.c_void_p, C.c_int64, C.c_int]
    L.rsi_hot_last_inflate_stats.argtypes = [C.c_void_p, C.POINTER(RsiInflateStats)]
    L.rsi_hot_inflate_bgzf.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.POINTER(RsiInflateStats)]
    L.rsi_hot_inflate_bgzf.restype = C.c_int64
    L.rsi_hot_set_exclude.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    L.rsi_exclude_read_bed.argtypes = [C.c_char_p, C.c_char_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int]
    L.rsi_hot_debug_classify.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.rsi_hot_debug_per_base.argtypes = [C.c_void_p, C.POINTER(RsiParams), C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int,
                                         C.POINTER(RsiChromStats)]
    L.rsi_hot_write_track.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_char_p, C.c_int, C.POINTER(RsiTrackStats)]
    L.rsi_hot_write_track_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_char_p, C.c_char_p, C.c_int, C.POINTER(RsiTrackStats)]
    L.rsi_hot_debug_track.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_char_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64,
                                      C.POINTER(RsiTrackStats)]
    L.rsi_hot_debug_track.restype = C.c_int64
    L.rsi_hot_write_bin_track.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_char_p, C.c_int, C.POINTER(RsiTrackStats)]
    L.rsi_hot_debug_bin_track.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_void_p, C.c_int, C.c_int64, C.c_int,
                                          C.c_char_p, C.c_int64, C.c_void_p, C.c_int64, C.POINTER(RsiTrackStats)]
    L.rsi_hot_debug_bin_track.restype = C.c_int64
    L.rsi_hot_set_track_format.argtypes = [C.c_void_p, C.c_int]
    L.rsi_hot_last_deflate_stats.argtypes = [C.c_void_p, C.POINTER(RsiDeflateStats)]
    L.rsi_hot_set_bam_read.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    L.rsi_hot_last_bam_read_stats.argtypes = [C.c_void_p, C.POINTER(RsiBamReadStats)]
    L.rsi_hot_set_bam_pairs.argtypes = [C.c_void_p, C.c_int]
    L.rsi_result_annotate_device.argtypes = [C.c_void_p, C.c_void_p]
    L.rsi_result_annotate_bam.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p]
    L.rsi_result_pairs.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_double)]
    L.rsi_hot_last_pairs_stats.argtypes = [C.c_void_p, C.POINTER(RsiPairsStats)]
    L.rsi_hot_debug_pair_sample.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 5 + [C.c_int64, C.c_void_p]
    L.rsi_hot_debug_pair_annotate.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 5 + [C.c_int] + [C.c_void_p] * 3 + [C.c_int, C.c_int] + [C.c_void_p] * 3
    L.rsi_hot_set_bam_pin.argtypes = [C.c_void_p, C.c_int]
    L.rsi_hot_stat_calls.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 5 + [C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_void_p, C.c_void_p]
    L.rsi_hot_pin_sample.argtypes = [C.c_void_p, C.POINTER(RsiPinStats)]
    L.rsi_hot_pin_calls.argtypes = [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 7
    L.rsi_hot_last_pin_stats.argtypes = [C.c_void_p, C.POINTER(RsiPinStats)]
    L.rsi_hot_debug_pin_sample.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 8 + [C.c_int64, C.c_int64, C.POINTER(RsiPinStats), C.c_void_p, C.c_void_p,
                                           C.c_int64]
    L.rsi_hot_debug_pin_calls.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 8 + [C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_double, C.c_int] + \
                                         [C.c_void_p] * 7
    L.rsi_hot_geno_calls.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.rsi_hot_last_geno_stats.argtypes = [C.c_void_p, C.POINTER(RsiGenoStats)]
    L.rsi_hot_debug_geno.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int] + [C.c_void_p] * 6 + [C.c_int, C.c_int, C.c_void_p]
    L.rsi_plot_batch_new.argtypes = [C.c_int64, C.c_int, C.c_double, C.c_double]
    L.rsi_plot_batch_new.restype = C.c_void_p
    L.rsi_plot_batch_free.argtypes = [C.c_void_p]
    L.rsi_plot_batch_free.restype = None
    L.rsi_plot_batch_add.argtypes = [C.c_void_p, C.POINTER(RsiCall)]
    L.rsi_plot_batch_add_span.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    L.rsi_plot_batch_size.argtypes = [C.c_void_p]
    L.rsi_plot_batch_refusal.argtypes = [C.c_void_p, C.c_int]
    L.rsi_plot_refusal_text.argtypes = [C.c_int]
    L.rsi_plot_refusal_text.restype = C.c_char_p
    L.rsi_plot_batch_queries.argtypes = [C.c_void_p]
    L.rsi_plot_batch_queries.restype = C.c_int64
    L.rsi_plot_batch_fill_host.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    L.rsi_plot_batch_chrom_median.argtypes = [C.c_void_p]
    L.rsi_plot_batch_chrom_median.restype = C.c_double
    L.rsi_plot_batch_compare.argtypes = [C.c_void_p, C.c_void_p]
    L.rsi_plot_batch_write.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_char_p, C.c_double, C.c_char_p, C.c_char_p, C.c_char_p]
    L.rsi_hot_plot_depth.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    L.rsi_hot_plot_run.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.rsi_hot_last_plot_stats.argtypes = [C.c_void_p, C.POINTER(RsiPlotStats)]
    L.rsi_hot_debug_plot.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_void_p]
    L.rsi_hot_debug_plot_expand.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int64]
    L.rsi_hot_loaded_depth.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]
    L.rsi_hot_depth_summary.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int]
    L.rsi_hot_depth_regions.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.rsi_hot_write_window_track.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_char_p, C.c_int64, C.c_char_p, C.c_int, C.POINTER(RsiTrackStats)]
    L.rsi_hot_write_region_track.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_char_p, C.c_int, C.c_void_p, C.c_void_p, C.c_char_p, C.c_int,
                                             C.POINTER(RsiTrackStats)]
    L.rsi_hot_last_depth_stats.argtypes = [C.c_void_p, C.POINTER(RsiDepthStats)]
    L.rsi_hot_debug_depth_summary.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int]
    L.rsi_hot_debug_depth_regions.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.rsi_hot_debug_region_track.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_char_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                             C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.POINTER(RsiTrackStats)]
    L.rsi_hot_debug_region_track.restype = C.c_int64
    L.rsi_bgzf_write_eof.argtypes = [C.c_char_p]
    L.rsi_track_index_create.argtypes = []
    L.rsi_track_index_create.restype = C.c_void_p
    L.rsi_track_index_free.argtypes = [C.c_void_p]
    L.rsi_track_index_free.restype = None
    L.rsi_hot_set_track_index.argtypes = [C.c_void_p, C.c_void_p]
    L.rsi_track_index_append.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    L.rsi_track_index_write_tbi.argtypes = [C.c_void_p, C.c_char_p]
    L.rsi_track_index_counts.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.rsi_track_index_debug_tbi.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    L.rsi_track_index_debug_tbi.restype = C.c_int64
    L.rsi_hot_debug_deflate.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.POINTER(RsiDeflateStats)]
    L.rsi_hot_debug_deflate.restype = C.c_int64
    L.rsi_ref_open.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(C.c_void_p)]
    L.rsi_ref_close.argtypes = [C.c_void_p]
    L.rsi_ref_close.restype = None
    L.rsi_ref_last_error.argtypes = [C.c_void_p]
    L.rsi_ref_last_error.restype = C.c_char_p
    L.rsi_ref_count.argtypes = [C.c_void_p]
    L.rsi_ref_sequence.argtypes = [C.c_void_p, C.c_int, C.POINTER(RsiRefSeq)]
    L.rsi_ref_find.argtypes = [C.c_void_p, C.c_char_p]
    L.rsi_ref_format.argtypes = [C.c_void_p]
    L.rsi_ref_index_path.argtypes = [C.c_void_p]
    L.rsi_ref_index_path.restype = C.c_char_p
    L.rsi_ref_load_device.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.POINTER(RsiRefStats)]
    L.rsi_ref_load_host.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int64]
    L.rsi_ref_device_alloc.argtypes = [C.c_int, C.c_int64]
    L.rsi_ref_device_alloc.restype = C.c_void_p
    L.rsi_ref_device_free.argtypes = [C.c_int, C.c_void_p]
    L.rsi_ref_device_free.restype = None
    L.rsi_hot_run_text_dfasta.argtypes = [C.c_void_p, C.POINTER(RsiParams), C.c_char_p, C.c_void_p, C.c_int64, C.POINTER(C.c_void_p), C.POINTER(RsiTextStats)]
    L.rsi_hot_run_bam_dfasta.argtypes = [C.c_void_p, C.POINTER(RsiParams), C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_void_p, C.c_int64,
                                         C.POINTER(C.c_void_p), C.POINTER(RsiBamStats)]
    L.rsi_ref_debug_set_chunks.argtypes = [C.c_void_p, C.c_int64, C.c_int64]
    L.rsi_ref_debug_fai_line.argtypes = [C.c_char_p, C.POINTER(RsiRefSeq)]
    L.rsi_ref_debug_ranges.argtypes = [C.POINTER(RsiRefSeq), C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_void_p]
    L.rsi_ref_debug_gzi.argtypes = [C.c_char_p, C.c_int64, C.c_void_p, C.c_int64]
    L.rsi_ref_debug_gzi.restype = C.c_int64
    L.rsi_ref_debug_cover.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p]
    _lib = L
    return L


def make_params(m=101, gcadjust=1, trans=0, merge=1, maxchkbp=100000, debug=0, cap=4.0, epsilon=1.5,
                threshold=-1.0, chklen=2.5, minmlen=3.01, buffer=0.05, p=0.05):
    """rsi:: defaults (rsi.cpp:34-98); m is forced odd as get_parameters does (rsi.cpp:2061-2064).
    trans: 0 NBN (-NB), 1 MED (-MED), 2 ALL (-ALL)."""
    if m % 2 != 1:
        m += 1
    return RsiParams(m, gcadjust, trans, merge, maxchkbp, debug, cap, epsilon, threshold, chklen, minmlen, buffer, p)


def _interval_arrays(exclude):
    """An (k, 2) array or a list of (start, end) pairs -> two contiguous int64 arrays."""
    iv = np.asarray(exclude, dtype=np.int64).reshape(-1, 2)
    return np.ascontiguousarray(iv[:, 0]), np.ascontiguousarray(iv[:, 1])


def read_exclude_bed(path, chrom, n):
    """The intervals a BED file (plain or gzip) holds for `chrom` of length n, sorted, merged and clipped to n: an (k, 2) int64
    array of 0-based half-open (start, end) pairs (rsi_exclude_read_bed; host only).  A malformed line raises RsiError."""
    lib = load_library()
    k = lib.rsi_exclude_read_bed(os.fsencode(path), chrom.encode(), int(n), None, None, 0)
    if k < 0:
        raise RsiError(k, lib.rsi_hot_last_error(None).decode())
    s = np.zeros(max(k, 1), dtype=np.int64)
    e = np.zeros(max(k, 1), dtype=np.int64)
    k2 = lib.rsi_exclude_read_bed(os.fsencode(path), chrom.encode(), int(n), s.ctypes.data, e.ctypes.data, k)
    if k2 < 0:
        raise RsiError(k2, lib.rsi_hot_last_error(None).decode())
    k = min(k, k2)
    return np.stack([s[:k], e[:k]], axis=1)


def bgzf_write_eof(path):
    """Ends a BGZF track: appends the 28-byte end-of-file block to `path` (rsi_bgzf_write_eof; host only) -- once, after the
    last chromosome appended to it."""
    lib = load_library()
    k = lib.rsi_bgzf_write_eof(os.fsencode(path))
    if k < 0:
        raise RsiError(k, lib.rsi_hot_last_error(None).decode())


class RsiError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"{STATUS_NAMES.get(code, code)}: {msg}")
        self.code = code


class TrackIndex:
    """The tabix index of BGZF tracks (rsi_track_index; host memory only): set on a context with RsiHot.set_track_index, filled by
    that context's BGZF track calls chromosome by chromosome, written as FILE.tbi."""

    def __init__(self):
        self.lib = load_library()
        self.handle = self.lib.rsi_track_index_create()
        if not self.handle:
            raise MemoryError("rsi_track_index_create")

    def close(self):
        if getattr(self, "handle", None):
            self.lib.rsi_track_index_free(self.handle)
            self.handle = None

    __del__ = close

    def _check(self, k):
        if k < 0:
            raise RsiError(k, self.lib.rsi_hot_last_error(None).decode())

    def append(self, src, shift):
        """src's chromosomes behind this index's, their compressed offsets moved by `shift` bytes (rsi_track_index_append)."""
        self._check(self.lib.rsi_track_index_append(self.handle, src.handle, int(shift)))

    def write_tbi(self, path):
        self._check(self.lib.rsi_track_index_write_tbi(self.handle, os.fsencode(path)))

    def counts(self):
        """{"nref", "chunks", "windows"} (rsi_track_index_counts)."""
        r, c, w = C.c_int64(), C.c_int64(), C.c_int64()
        self._check(self.lib.rsi_track_index_counts(self.handle, C.byref(r), C.byref(c), C.byref(w)))
        return {"nref": r.value, "chunks": c.value, "windows": w.value}

    def tbi_bytes(self):
        """The .tbi stream before compression (test hook, rsi_track_index_debug_tbi)."""
        k = self.lib.rsi_track_index_debug_tbi(self.handle, None, 0)
        self._check(int(k))
        out = np.zeros(max(k, 1), dtype=np.uint8)
        k2 = self.lib.rsi_track_index_debug_tbi(self.handle, out.ctypes.data, k)
        self._check(int(k2))
        return out[:k].tobytes()


class RsiRef:
    """An indexed FASTA file, plain text or BGZF, read on the device (rsi_ref).  Opening parses the .fai (and
    later the .gzi) and touches no GPU.  fai / gzi: their paths (None: PATH.fai, PATH.gzi when it is there); gzi="none": the
    BGZF members are walked instead."""

    def __init__(self, path, fai=None, gzi=None, device=0):
        self.lib = load_library()
        self.device = int(device)
        h = C.c_void_p()
        rc = self.lib.rsi_ref_open(os.fsencode(path), None if fai is None else os.fsencode(fai), None if gzi is None else os.fsencode(gzi), C.byref(h))
        if rc != 0:
            raise RsiError(rc, self.lib.rsi_ref_last_error(None).decode())
        self.handle = h

    def close(self):
        if getattr(self, "handle", None):
            self.lib.rsi_ref_close(self.handle)
            self.handle = None

    __del__ = close

    def _check(self, rc):
        if rc < 0:
            raise RsiError(rc, self.lib.rsi_ref_last_error(self.handle).decode())

    @property
    def count(self):
        return self.lib.rsi_ref_count(self.handle)

    @property
    def format(self):
        """0 text, 1 BGZF"""
        return self.lib.rsi_ref_format(self.handle)

    def find(self, rname):
        """Index of the first sequence named rname or "chr" + rname (read_fasta's rule), -1 when there is none."""
        return self.lib.rsi_ref_find(self.handle, rname.encode())

    def sequence(self, i):
        """{"name", "length", "offset", "linebases", "linewidth"} of sequence i."""
        s = RsiRefSeq()
        if self.lib.rsi_ref_sequence(self.handle, int(i), C.byref(s)) != 0:
            raise IndexError(i)
        return {"name": s.name.decode(), "length": s.length, "offset": s.offset, "linebases": s.linebases, "linewidth": s.linewidth}

    def debug_set_chunks(self, text_chunk_bases=0, bgzf_span_bytes=0):
        """Test hook (rsi_ref_debug_set_chunks): the bases per transfer of a text load and the text per inflate launch of a BGZF
        load; 0: the default."""
        self._check(self.lib.rsi_ref_debug_set_chunks(self.handle, int(text_chunk_bases), int(bgzf_span_bytes)))

    def load_device(self, i, d_out, cap, stream=None):
        """Sequence i unfolded into device memory at address d_out (16-byte aligned, cap >= length + 64); returns the load's figures."""
        st = RsiRefStats()
        self._check(self.lib.rsi_ref_load_device(self.handle, self.device, int(i), d_out, int(cap), stream, C.byref(st)))
        return {f: getattr(st, f) for f, _ in RsiRefStats._fields_}

    def load_host(self, i):
        """Sequence i, unfolded on the device, as bytes."""
        n = self.sequence(i)["length"]
        out = np.zeros(max(n, 1), dtype=np.uint8)
        self._check(self.lib.rsi_ref_load_host(self.handle, self.device, int(i), out.ctypes.data, n))
        return out[:n].tobytes()


class Result:
    """One chromosome's results.  The C object is kept and read on demand (list by list), so that a caller
    that only wants the final calls does not pay for converting thousands of intermediate segments."""

    def __init__(self, lib, handle):
        self._lib = lib
        self._h = handle
        self._lists = {}
        self._rows = None
        self._noncode = None
        self._stats = None

    def __del__(self):
        try:
            if self._h:
                self._lib.rsi_result_free(self._h)
                self._h = None
        except Exception:
            pass

    @property
    def stats(self):
        if self._stats is None:
            st = self._lib.rsi_result_stats(self._h).contents
            self._stats = {f[0]: getattr(st, f[0]) for f in RsiChromStats._fields_}
        return self._stats

    def calls(self, which="calls"):
        if which not in self._lists:
            w = WHICH[which]
            k = self._lib.rsi_result_ncalls(self._h, w)
            arr = self._lib.rsi_result_calls(self._h, w)
            self._lists[which] = [{f: getattr(arr[i], f) for f in CALL_FIELDS} for i in range(k)]
        return self._lists[which]

    def summary_into(self, row, chrom_id, max_calls):
        """Write the fixed-layout summary block (rsi_result_summary: [chrom id, median, SD, number of calls, stored, 0, 0, 0]
        then 8 doubles per stored call) into a float64 numpy row; returns the number of doubles written."""
        assert row.dtype == np.float64 and row.flags["C_CONTIGUOUS"] and row.size >= SUMMARY_HEAD + SUMMARY_CALL * max_calls
        return self._lib.rsi_result_summary(self._h, int(chrom_id), row.ctypes.data, int(max_calls))

    def annotate_bam(self, bam, chrom):
        """RP / Q0 of the final calls from the BAM file and its .bai, on the host (rsi_result_annotate_bam)."""
        rc = self._lib.rsi_result_annotate_bam(self._h, os.fsencode(bam), chrom.encode())
        if rc != RSI_OK:
            raise RsiError(rc, self._lib.rsi_hot_last_error(None).decode())
        self._rows = None

    def pairs(self):
        """(rp, q0) of every final call (rsi_result_pairs): -1 / -1.0 before an annotation."""
        out = []
        rp, q0 = C.c_int32(0), C.c_double(0.0)
        for i in range(self._lib.rsi_result_ncalls(self._h, WHICH["calls"])):
            self._lib.rsi_result_pairs(self._h, i, C.byref(rp), C.byref(q0))
            out.append((rp.value, q0.value))
        return out

    def log_lines(self):
        """The per-L "DEL-" / "DUP+" lines of the scan passes (rsi.cpp:1221-1224, 1251-1254)."""
        out, i, buf = [], 0, C.create_string_buffer(256)
        while True:
            i = self._lib.rsi_result_log_line(self._h, i, buf, 256)
            if i <= 0:
                return out
            out.append(buf.value.decode())

    @property
    def lists(self):
        return {name: self.calls(name) for name in WHICH}

    @property
    def noncode(self):
        if self._noncode is None:
            k = self._lib.rsi_result_noncode(self._h, None, 0)
            pairs = (C.c_int32 * max(2 * k, 2))()
            self._lib.rsi_result_noncode(self._h, pairs, k)
            self._noncode = np.array(pairs[:2 * k], dtype=np.int32)
        return self._noncode

    @property
    def rows(self):
        if self._rows is None:
            buf = C.create_string_buffer(1024)
            self._rows = []
            for i in range(self._lib.rsi_result_ncalls(self._h, WHICH["calls"])):
                self._lib.rsi_result_format_row(self._h, i, b"%CHROM%", buf, 1024)
                self._rows.append(buf.value.decode())
        return self._rows

    def format_rows(self, chrom):
        return [r.replace("%CHROM%", chrom) for r in self.rows]


class RsiHot:
    """One context = one GPU + one stream (rsi_hot_create)."""

    def __init__(self, device=0):
        self.lib = load_library()
        st = C.c_int(0)
        self.ctx = self.lib.rsi_hot_create(device, C.byref(st))
        if not self.ctx:
            raise RsiError(st.value, self.lib.rsi_hot_last_error(None).decode())

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.rsi_hot_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != RSI_OK:
            raise RsiError(rc, self.lib.rsi_hot_last_error(self.ctx).decode())

    def set_timing(self, on=True):
        self.lib.rsi_hot_set_timing(self.ctx, int(on))

    def debug_level_sums(self, T, status, Lmax):
        """filterstatus' per-level float sums of host arrays on the device (test hook): (sums, counts), index = level + Lmax."""
        t = np.ascontiguousarray(T, dtype=np.float32)
        s = np.ascontiguousarray(status, dtype=np.int32)
        assert t.size == s.size
        sums = np.zeros(2 * Lmax + 1, dtype=np.float32)
        counts = np.zeros(2 * Lmax + 1, dtype=np.int32)
        self.lib.rsi_hot_debug_level_sums.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p]
        self._check(self.lib.rsi_hot_debug_level_sums(self.ctx, t.ctypes.data, s.ctypes.data, t.size, int(Lmax), sums.ctypes.data, counts.ctypes.data))
        return sums, counts

    def debug_scan(self, T, medint, RDmedian, tmedian, tlamda, Lmax):
        """One scan pass (rsistatus) over host arrays on the device (test hook): (status, info)."""
        t = np.ascontiguousarray(T, dtype=np.float32)
        mi = np.ascontiguousarray(medint, dtype=np.int32)
        assert t.size == mi.size
        st = np.zeros(t.size, dtype=np.int32)
        info = np.zeros(4, dtype=np.int32)
        self.lib.rsi_hot_debug_scan.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_double, C.c_double, C.c_double, C.c_int,
                                                C.c_void_p, C.c_void_p]
        self._check(self.lib.rsi_hot_debug_scan(self.ctx, t.ctypes.data, mi.ctypes.data, t.size, float(RDmedian), float(tmedian), float(tlamda),
                                                int(Lmax), st.ctypes.data, info.ctypes.data))
        return st, info

    def debug_segments(self, T, status, runs, tmedian, tlamda=0.0, pairs_per_item=0):
        """get_rsi_segments over host arrays on the device (test hook): runs = (start, end) pairs.  Returns (start, end, type, score, info);
        info = runs, work items, lists inline, status through the mailbox, runs beyond the LDS staging, segments, pairs per item, 0."""
        t = np.ascontiguousarray(T, dtype=np.float32)
        st = np.ascontiguousarray(status, dtype=np.int32)
        assert st.size == t.size
        rl = np.ascontiguousarray(runs, dtype=np.int32).reshape(-1, 2)
        k = rl.shape[0]
        s, e, ty = (np.zeros(max(k, 1), dtype=np.int32) for _ in range(3))
        sc = np.zeros(max(k, 1), dtype=np.float64)
        info = np.zeros(8, dtype=np.int32)
        self.lib.rsi_hot_debug_segments.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_double, C.c_double,
                                                    C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        self._check(self.lib.rsi_hot_debug_segments(self.ctx, t.ctypes.data, st.ctypes.data, t.size, rl.ctypes.data, k, float(tmedian), float(tlamda),
                                                    int(pairs_per_item), s.ctypes.data, e.ctypes.data, ty.ctypes.data, sc.ctypes.data, info.ctypes.data))
        n = int(info[5])
        return s[:n], e[:n], ty[:n], sc[:n], info

    def debug_sharpen(self, depth, storage, start, end, type_):
        """optimize_with_derivative, both calls, for a list of candidates over a host array on the device (test hook): storage 1 keeps the
        array as bytes, 4 as int32.  Returns (start, end, info); info = workspace jobs before, after, job list in the mailbox, waits."""
        d = np.ascontiguousarray(depth, dtype=np.int32)
        s = np.array(start, dtype=np.int32).reshape(-1)
        e = np.array(end, dtype=np.int32).reshape(-1)
        ty = np.ascontiguousarray(type_, dtype=np.int32).reshape(-1)
        assert s.size == e.size == ty.size
        info = np.zeros(4, dtype=np.int32)
        self.lib.rsi_hot_debug_sharpen.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        self._check(self.lib.rsi_hot_debug_sharpen(self.ctx, d.ctypes.data, d.size, int(storage), s.ctypes.data, e.ctypes.data, ty.ctypes.data, s.size,
                                                   info.ctypes.data))
        return s, e, info

    def debug_candidate_tests(self, depth, storage, span_all, RDmedian, cands, index, form, m=101, minmlen=3.01, chklen=2.5, buffer=0.05,
                              maxchkbp=100000):
        """The neighbourhood tests of list entries over a host array on the device (test hook).  cands: int32 [k, 4] (start, end, type,
        status); index: the entries to test, all in one call of the device tester; form: bit 0 split / one workgroup, bit 1 byte depth
        gathered as int32.  Returns (records, info): records a structured array with the fields of rsi_cand_record; info = waits, job
        lists in the mailbox, job lists copied, capacity of the per-job records before / after, of the folded histograms before / after, 0."""
        d = np.ascontiguousarray(depth, dtype=np.int32)
        c = np.ascontiguousarray(cands, dtype=np.int32).reshape(-1, 4)
        cols = [np.ascontiguousarray(c[:, j]) for j in range(4)]
        ix = np.ascontiguousarray(index, dtype=np.int32).reshape(-1)
        out = np.zeros(max(ix.size, 1), dtype=CAND_RECORD)
        info = np.zeros(8, dtype=np.int32)
        self.lib.rsi_hot_debug_candidate_tests.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_double, C.c_int, C.c_double,
                                                           C.c_double, C.c_double, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                                           C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        self._check(self.lib.rsi_hot_debug_candidate_tests(self.ctx, d.ctypes.data, d.size, int(storage), int(span_all), float(RDmedian), int(m),
                                                           float(minmlen), float(chklen), float(buffer), int(maxchkbp), cols[0].ctypes.data,
                                                           cols[1].ctypes.data, cols[2].ctypes.data, cols[3].ctypes.data, c.shape[0],
                                                           ix.ctypes.data, ix.size, int(form), out.ctypes.data, info.ctypes.data))
        return out[:ix.size], info

    def debug_range_sums(self, depth, storage, lo, hi):
        """Exact sums of a host array over inclusive ranges through the device tester (test hook): (int64 sums, info); info = waits,
        1 / 0 for the ranges in the mailbox / copied."""
        d = np.ascontiguousarray(depth, dtype=np.int32)
        a = np.ascontiguousarray(lo, dtype=np.int32).reshape(-1)
        b = np.ascontiguousarray(hi, dtype=np.int32).reshape(-1)
        assert a.size == b.size
        sums = np.zeros(max(a.size, 1), dtype=np.int64)
        info = np.zeros(2, dtype=np.int32)
        self.lib.rsi_hot_debug_range_sums.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        self._check(self.lib.rsi_hot_debug_range_sums(self.ctx, d.ctypes.data, d.size, int(storage), a.ctypes.data, b.ctypes.data, a.size,
                                                      sums.ctypes.data, info.ctypes.data))
        return sums[:a.size], info

    def debug_block_stage(self, binmedint, status, segs, ncompact, RDmedian, tester=True, sparse=False, **params):
        """areblockscnv on a segment list in bin space over host arrays (test hook).  segs: a CALL_RECORD array (start, end, type, score,
        status); params: make_params' keywords.  Returns (segments as judged, road per first-round test, info as a dict of LIST_INFO)."""
        b = np.ascontiguousarray(binmedint, dtype=np.int32)
        st = np.ascontiguousarray(status, dtype=np.int32)
        assert b.size == st.size
        L = np.array(segs, dtype=CALL_RECORD).reshape(-1)
        road = np.full(max(L.size, 1), -1, dtype=np.int32)
        info = np.zeros(10, dtype=np.int32)
        P = make_params(**params)
        self.lib.rsi_hot_debug_block_stage.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_double, C.c_void_p, C.c_void_p,
                                                       C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        self._check(self.lib.rsi_hot_debug_block_stage(self.ctx, b.ctypes.data, st.ctypes.data, b.size, int(ncompact), float(RDmedian), C.addressof(P),
                                                       L.ctypes.data, L.size, int(bool(tester)), int(bool(sparse)), road.ctypes.data, info.ctypes.data))
        return L, road[:L.size], dict(zip(LIST_INFO, (int(v) for v in info)))

    def debug_merge(self, depth, storage, cands, RDmedian, tester=True, **params):
        """mergesegments on a list in base coordinates over a host array (test hook).  cands: a CALL_RECORD array whose geno, status, p1 and
        refsd are the caller's.  Returns (the list after both passes, info as a dict of LIST_INFO)."""
        d = np.ascontiguousarray(depth, dtype=np.int32)
        L = np.ascontiguousarray(np.array(cands, dtype=CALL_RECORD).reshape(-1))
        out = np.zeros(max(L.size, 1), dtype=CALL_RECORD)
        nout = np.zeros(1, dtype=np.int32)
        info = np.zeros(10, dtype=np.int32)
        P = make_params(**params)
        self.lib.rsi_hot_debug_merge.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                                 C.c_void_p, C.c_void_p, C.c_void_p]
        self._check(self.lib.rsi_hot_debug_merge(self.ctx, d.ctypes.data, d.size, int(storage), float(RDmedian), C.addressof(P), L.ctypes.data, L.size,
                                                 int(bool(tester)), out.ctypes.data, nout.ctypes.data, info.ctypes.data))
        return out[:int(nout[0])], dict(zip(LIST_INFO, (int(v) for v in info)))

    def debug_calls(self, depth, storage, segs, noncode, RDmedian, RDsd, tester=True, **params):
        """Everything behind the block tests on tested segments in bin space over a host array (test hook).  noncode: (k, 2) regions.
        Returns (blocks, raw, kept, info as a dict of LIST_INFO)."""
        d = np.ascontiguousarray(depth, dtype=np.int32)
        L = np.ascontiguousarray(np.array(segs, dtype=CALL_RECORD).reshape(-1))
        nc = np.asarray(noncode, dtype=np.int32).reshape(-1, 2)
        a, b = np.ascontiguousarray(nc[:, 0]), np.ascontiguousarray(nc[:, 1])
        outs = [np.zeros(max(L.size, 1), dtype=CALL_RECORD) for _ in range(3)]
        counts = np.zeros(3, dtype=np.int32)
        info = np.zeros(10, dtype=np.int32)
        P = make_params(**params)
        self.lib.rsi_hot_debug_calls.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_int,
                                                 C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        self._check(self.lib.rsi_hot_debug_calls(self.ctx, d.ctypes.data, d.size, int(storage), float(RDmedian), float(RDsd), C.addressof(P),
                                                 L.ctypes.data, L.size, a.ctypes.data if a.size else None, b.ctypes.data if b.size else None, a.size,
                                                 int(bool(tester)), outs[0].ctypes.data, outs[1].ctypes.data, outs[2].ctypes.data, counts.ctypes.data,
                                                 info.ctypes.data))
        return outs[0][:counts[0]], outs[1][:counts[1]], outs[2][:counts[2]], dict(zip(LIST_INFO, (int(v) for v in info)))

    def debug_nb_transform(self, binsum, m, ncompact, RDmedian, r):
        """The NB transform of host bin sums on the device (test hook): (raw, T, info).  raw: the values before the minimum is taken off;
        info = raw minimum (float bits), the first quantile grid's plan (flags, buckets, minimum as float bits), the min/max record as
        it was left (0), t0 and t2 (float bits), 0."""
        b = np.ascontiguousarray(binsum, dtype=np.int64)
        raw = np.zeros(b.size, dtype=np.float32)
        T = np.zeros(b.size, dtype=np.float32)
        info = np.zeros(8, dtype=np.int32)
        self.lib.rsi_hot_debug_nb_transform.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_double, C.c_double, C.c_void_p,
                                                        C.c_void_p, C.c_void_p]
        self._check(self.lib.rsi_hot_debug_nb_transform(self.ctx, b.ctypes.data, b.size, int(m), int(ncompact), float(RDmedian), float(r),
                                                        raw.ctypes.data, T.ctypes.data, info.ctypes.data))
        return raw, T, info

    def debug_nb_keyed(self, binsum, m, K, RDmedian, r, mask=None):
        """The keyed form of the NB transform and its quantile chains over host bin sums (test hook, include/rsi_hot.h): (T, out, info).
        out = (median, count, MAD, count), of the bins with mask == 0 where a mask is given; info = flags and buckets of the median
        record, the same of the MAD record, the raw minimum (float bits), the form (1 keyed, 0 declined to the chain, -1 the route
        does not apply), host-driven medians, 0."""
        b = np.ascontiguousarray(binsum, dtype=np.int64)
        mk = None if mask is None else np.ascontiguousarray(mask, dtype=np.int32)
        assert mk is None or mk.size == b.size
        T = np.zeros(b.size, dtype=np.float32)
        out = np.zeros(4, dtype=np.float64)
        info = np.zeros(8, dtype=np.int32)
        self.lib.rsi_hot_debug_nb_keyed.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_double, C.c_double,
                                                    C.c_void_p, C.c_void_p, C.c_void_p]
        self._check(self.lib.rsi_hot_debug_nb_keyed(self.ctx, b.ctypes.data, None if mk is None else mk.ctypes.data, b.size, int(m), int(K),
                                                    float(RDmedian), float(r), T.ctypes.data, out.ctypes.data, info.ctypes.data))
        return T, out, info

    def debug_filterstatus(self, T, status, Lmax, dev):
        """filterstatus behind a scan pass over host arrays on the device (test hook): (status_out, info).  info = runs after the last
        is dropped, run list inline, boundary entries copied (-1 each where nothing was trimmed), level-sums route (0 device, 1 host
        loop after the device declined, 2 long scan), has_level0, trim, leveldel, leveladd, m0 (float bits), 0."""
        t = np.ascontiguousarray(T, dtype=np.float32)
        st = np.ascontiguousarray(status, dtype=np.int32)
        assert st.size == t.size
        out = np.zeros(t.size, dtype=np.int32)
        info = np.zeros(10, dtype=np.int32)
        self.lib.rsi_hot_debug_filterstatus.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_double, C.c_void_p, C.c_void_p]
        self._check(self.lib.rsi_hot_debug_filterstatus(self.ctx, t.ctypes.data, st.ctypes.data, t.size, int(Lmax), float(dev), out.ctypes.data,
                                                        info.ctypes.data))
        return out, info

    GRID_MODES = {"pair": 0, "mad": 1, "host": 2}

    def debug_grid_median(self, x, mask=None, mode="pair", center=0.0):
        """0.01-grid median and MAD of a host array on the device (test hook, include/rsi_hot.h): (out, info).
        x: float32 values, or int32 bin medians for mode "med" (-MED's MAD around `center`); mask: int32, 0 = selected.
        out = (median, count, MAD, count); info = flags and buckets of the median record, the same of the MAD record,
        16-bit counters (1 / 0, -1: no chain), host-driven medians, 0, 0."""
        out = np.zeros(4, dtype=np.float64)
        info = np.zeros(8, dtype=np.int32)
        if mode == "med":
            assert mask is None
            xi = np.ascontiguousarray(x, dtype=np.int32)
            self.lib.rsi_hot_debug_grid_mad_i32.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_double, C.c_void_p, C.c_void_p]
            self._check(self.lib.rsi_hot_debug_grid_mad_i32(self.ctx, xi.ctypes.data, xi.size, float(center), out.ctypes.data, info.ctypes.data))
            return out, info
        xf = np.ascontiguousarray(x, dtype=np.float32)
        mk = None if mask is None else np.ascontiguousarray(mask, dtype=np.int32)
        assert mk is None or mk.size == xf.size
        self.lib.rsi_hot_debug_grid_median.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_double, C.c_void_p, C.c_void_p]
        self._check(self.lib.rsi_hot_debug_grid_median(self.ctx, xf.ctypes.data, None if mk is None else mk.ctypes.data, xf.size,
                                                       self.GRID_MODES[mode], float(center), out.ctypes.data, info.ctypes.data))
        return out, info

    def set_exclude(self, exclude):
        """Arm the NEXT run on this context with excluded intervals: an (k, 2) integer array or a list of (start, end) pairs,
        0-based half-open, any order; their bases are treated as N (rsi_hot_set_exclude).  None or an empty list disarms."""
        if exclude is None or len(exclude) == 0:
            self._check(self.lib.rsi_hot_set_exclude(self.ctx, None, None, 0))
            return
        s, e = _interval_arrays(exclude)
        self._check(self.lib.rsi_hot_set_exclude(self.ctx, s.ctypes.data, e.ctypes.data, s.size))

    def debug_classify(self, fasta, exclude=None):
        """The GC and N bit planes of a host sequence after the classification kernel and, with `exclude`, the mask kernel (test
        hook): (gcbits, nbits), uint64[n // 64 + 1] each, bit j of word w for base 64 w + j."""
        f = np.ascontiguousarray(fasta, dtype=np.uint8)
        gc = np.zeros(f.size // 64 + 1, dtype=np.uint64)
        nb = np.zeros(f.size // 64 + 1, dtype=np.uint64)
        if exclude is None or len(exclude) == 0:
            rc = self.lib.rsi_hot_debug_classify(self.ctx, f.ctypes.data, f.size, None, None, 0, gc.ctypes.data, nb.ctypes.data)
        else:
            s, e = _interval_arrays(exclude)
            rc = self.lib.rsi_hot_debug_classify(self.ctx, f.ctypes.data, f.size, s.ctypes.data, e.ctypes.data, s.size, gc.ctypes.data, nb.ctypes.data)
        self._check(rc)
        return gc, nb

    def debug_per_base(self, params, depth, fasta, exclude=None):
        """The per-base phase alone on host arrays (test hook, rsi_hot_debug_per_base): the statistics it fills, as a dict.
        Afterwards fetch("rd_gc" / "rd_concat" / "binmedint" / "binsum" / "noncode"), phase_times() and kernel_times() are those
        of the phase; phase_times() ends with the "k4.form ..." entries."""
        d = np.ascontiguousarray(depth, dtype=np.int32)
        f = np.ascontiguousarray(fasta, dtype=np.uint8)
        if d.shape != f.shape or d.ndim != 1:
            raise ValueError("depth and fasta must be 1-D arrays of the same length")
        st = RsiChromStats()
        if exclude is None or len(exclude) == 0:
            rc = self.lib.rsi_hot_debug_per_base(self.ctx, C.byref(params), d.ctypes.data, f.ctypes.data, d.size, None, None, 0, C.byref(st))
        else:
            s, e = _interval_arrays(exclude)
            rc = self.lib.rsi_hot_debug_per_base(self.ctx, C.byref(params), d.ctypes.data, f.ctypes.data, d.size, s.ctypes.data, e.ctypes.data,
                                                 s.size, C.byref(st))
        self.last_stats = {k[0]: getattr(st, k[0]) for k in RsiChromStats._fields_}
        self._check(rc)
        return self.last_stats

    def run(self, params, depth, fasta, exclude=None):
        """depth: int32[n] raw per-base depth, fasta: uint8[n] sequence bytes (host arrays); exclude: intervals treated as N
        in this run (set_exclude)."""
        d = np.ascontiguousarray(depth, dtype=np.int32)
        f = np.ascontiguousarray(fasta, dtype=np.uint8)
        if d.shape != f.shape or d.ndim != 1:
            raise ValueError("depth and fasta must be 1-D arrays of the same length")
        out = C.c_void_p()
        if exclude is not None:
            self.set_exclude(exclude)
        self._check(self.lib.rsi_hot_run(self.ctx, C.byref(params), d.ctypes.data, f.ctypes.data, d.size, C.byref(out)))
        return Result(self.lib, out)

    def load_depth_text(self, path, n):
        """Parse a "pos depth" text file into the context's device depth buffer (rsi_hot_load_depth_text).
        Returns the statistics as a dict; fetch("depth_in") reads the result back."""
        st = RsiTextStats()
        self._check(self.lib.rsi_hot_load_depth_text(self.ctx, os.fsencode(path), int(n), C.byref(st)))
        return {f[0]: getattr(st, f[0]) for f in RsiTextStats._fields_ if f[0] != "pad"}

    def inflate_bgzf(self, data):
        """BGZF bytes (whole members) -> their text, inflated on the device (rsi_hot_inflate_bgzf; CRC32 and ISIZE checked
        there).  Raises RsiError on a bad member."""
        data = bytes(data)
        st = RsiInflateStats()
        src = np.frombuffer(data, dtype=np.uint8) if data else np.zeros(1, dtype=np.uint8)
        size = self._bgzf_text_size(data)
        out = np.zeros(max(size, 1), dtype=np.uint8)
        k = self.lib.rsi_hot_inflate_bgzf(self.ctx, src.ctypes.data, len(data), out.ctypes.data, size, C.byref(st))
        self._check(int(k) if k < 0 else 0)
        return out[:k].tobytes()

    @staticmethod
    def _bgzf_text_size(data):
        """Sum of the members' ISIZE (the footers), walking BSIZE; a malformed walk returns what it has (the device call
        reports the error)."""
        p, total = 0, 0
        while p + 18 <= len(data):
            xlen = data[p + 10] | (data[p + 11] << 8)
            bsize = None
            k = p + 12
            while k + 4 <= p + 12 + xlen and k + 4 <= len(data):
                slen = data[k + 2] | (data[k + 3] << 8)
                if data[k] == 66 and data[k + 1] == 67 and slen == 2 and k + 6 <= len(data):
                    bsize = (data[k + 4] | (data[k + 5] << 8)) + 1
                k += 4 + slen
            if bsize is None or p + bsize > len(data):
                break
            total += int.from_bytes(data[p + bsize - 4:p + bsize], "little")
            p += bsize
        return total

    def inflate_stats(self):
        """Format and inflate figures of the last load_depth_text / run_text / inflate_bgzf: format ("text", "bgzf",
        "gzip"), compressed_bytes, text_bytes, blocks, t_inflate_kernel_ms (device), t_host_inflate_ms (zlib)."""
        st = RsiInflateStats()
        self._check(self.lib.rsi_hot_last_inflate_stats(self.ctx, C.byref(st)))
        return _inflate_dict(st)

    def run_text(self, params, path, fasta, exclude=None):
        """Depth from a text file (parsed on the device), fasta: uint8[n] host array; exclude: as for run."""
        f = np.ascontiguousarray(fasta, dtype=np.uint8)
        if exclude is not None:
            self.set_exclude(exclude)
        out = C.c_void_p()
        st = RsiTextStats()
        self._check(self.lib.rsi_hot_run_text(self.ctx, C.byref(params), os.fsencode(path), f.ctypes.data, f.size, C.byref(out), C.byref(st)))
        res = Result(self.lib, out)
        res.text_stats = {f_[0]: getattr(st, f_[0]) for f_ in RsiTextStats._fields_ if f_[0] != "pad"}
        return res

    def load_depth_bam(self, bam, chrom, minq=0, min_baseq=13):
        """Per-base depth of `chrom` from a BAM file into the context's device depth buffer (rsi_hot_load_depth_bam)."""
        st = RsiBamStats()
        self._check(self.lib.rsi_hot_load_depth_bam(self.ctx, os.fsencode(bam), chrom.encode(), int(minq), int(min_baseq), C.byref(st)))
        return {f[0]: getattr(st, f[0]) for f in RsiBamStats._fields_}

    def set_bam_read(self, mode, chunk_bytes=0):
        """Where this context's BAM loads read the records from now on (rsi_hot_set_bam_read): "host" / 0, zlib threads and a
        host walk, or "device" / 1, BGZF inflated and records found on the GPU.  chunk_bytes: inflated bytes per chunk of the
        device mode (0: the default)."""
        m = BAM_READ_MODES.get(mode, mode) if isinstance(mode, str) else mode
        if isinstance(m, str) or isinstance(m, bool):
            raise ValueError(f"BAM read mode {mode!r}: expected 'host' or 'device'")
        self._check(self.lib.rsi_hot_set_bam_read(self.ctx, int(m), int(chunk_bytes)))

    def set_bam_pairs(self, on=True):
        """Arm (or disarm) this context's BAM loads to keep the pair table in HBM (rsi_hot_set_bam_pairs): what annotate_device
        needs.  fetch("pairs_pos" / "pairs_rend" / "pairs_mpos" / "pairs_isize" / "pairs_info") reads an armed load's table."""
        self._check(self.lib.rsi_hot_set_bam_pairs(self.ctx, int(bool(on))))

    def annotate_device(self, res):
        """RP / Q0 of the final calls of `res` from the pair table of the context's last armed load (rsi_result_annotate_device)."""
        self._check(self.lib.rsi_result_annotate_device(self.ctx, res._h))
        res._rows = None

    def pairs_stats(self):
        """The pair table of the last armed load and the last annotate_device (rsi_hot_last_pairs_stats); records == 0: no table."""
        st = RsiPairsStats()
        self._check(self.lib.rsi_hot_last_pairs_stats(self.ctx, C.byref(st)))
        return {f[0]: getattr(st, f[0]) for f in RsiPairsStats._fields_}

    @staticmethod
    def _pair_arrays(table):
        arrs = [np.ascontiguousarray(np.asarray(a).astype(np.int64) & 0xffffffff, dtype=np.uint32).view(np.int32) for a in table]
        assert len(arrs) == 5 and all(a.ndim == 1 and a.size == arrs[0].size for a in arrs)
        return arrs

    def debug_pair_sample(self, table, tid_len):
        """The insert-size sample over a caller's pair table (test hook, rsi_hot_debug_pair_sample): table = (pos, rend, mpos,
        isize, info).  Returns [count, sum |isize|, sum of wrapped squares, S]."""
        arrs = self._pair_arrays(table)
        out = np.zeros(4, dtype=np.int64)
        self._check(self.lib.rsi_hot_debug_pair_sample(self.ctx, arrs[0].size, *[a.ctypes.data for a in arrs], int(tid_len), out.ctypes.data))
        return [int(v) for v in out]

    def debug_pair_annotate(self, table, start, end, type_, isize_mean, isize_sd):
        """The annotation counts of calls over a caller's pair table, ascending in pos (test hook, rsi_hot_debug_pair_annotate):
        returns (rp, q0_all, q0_q0), one uint32 array each."""
        arrs = self._pair_arrays(table)
        s, e, ty = (np.ascontiguousarray(v, dtype=np.int32).reshape(-1) for v in (start, end, type_))
        assert s.size == e.size == ty.size
        rp, qa, qq = (np.zeros(max(s.size, 1), dtype=np.uint32) for _ in range(3))
        self._check(self.lib.rsi_hot_debug_pair_annotate(self.ctx, arrs[0].size, *[a.ctypes.data for a in arrs], s.size, s.ctypes.data, e.ctypes.data,
                                                         ty.ctypes.data, int(isize_mean), int(isize_sd), rp.ctypes.data, qa.ctypes.data, qq.ctypes.data))
        return rp[:s.size], qa[:s.size], qq[:s.size]

    def set_bam_pin(self, on=True):
        """Arm (or disarm) this context's BAM loads to keep every read's l_qseq and CIGAR beside the pair table
        (rsi_hot_set_bam_pin; arming arms the pair table too): what pin_sample and pin_calls need.  fetch("pin_lq" / "pin_coff" /
        "pin_pool") reads an armed load's arrays: pool[coff[k]] is read k's n_cigar, its CIGAR words follow."""
        self._check(self.lib.rsi_hot_set_bam_pin(self.ctx, int(bool(on))))

    def stat_calls(self, start, end, type_, p1e, p2e, isize=-1, isize_sd=-1):
        """RP / Q0 of a list's calls on the chromosome of the last armed load, with cnv_stat's windows given (rsi_hot_stat_calls).
        Returns (rp int32[], q0 float64[], isize, isize_sd): the insert size to carry to the next chromosome."""
        a = [np.ascontiguousarray(v, dtype=np.int32).reshape(-1) for v in (start, end, type_, p1e, p2e)]
        assert all(v.size == a[0].size for v in a)
        k = a[0].size
        rp, q0 = np.zeros(max(k, 1), dtype=np.int32), np.zeros(max(k, 1), dtype=np.float64)
        i1, i2 = C.c_int32(int(isize)), C.c_int32(int(isize_sd))
        self._check(self.lib.rsi_hot_stat_calls(self.ctx, k, *[v.ctypes.data for v in a], C.byref(i1), C.byref(i2), rp.ctypes.data, q0.ctypes.data))
        return rp[:k], q0[:k], i1.value, i2.value

    @staticmethod
    def _pin_dict(st):
        return {f[0]: getattr(st, f[0]) for f in RsiPinStats._fields_}

    def pin_sample(self):
        """The depth sample of the last load armed for pin (rsi_hot_pin_sample): l_qseq, rd, rd_sd, drd, drd_sd and the rest of
        pin_stats().  RsiError RSI_ERR_UNSUPPORTED where the chromosome cannot be sampled as the reference does."""
        st = RsiPinStats()
        self._check(self.lib.rsi_hot_pin_sample(self.ctx, C.byref(st)))
        return self._pin_dict(st)

    def pin_calls(self, m, start, end, type_):
        """The calls' breakpoints moved (rsi_hot_pin_calls, behind pin_sample): (new_start, new_end, sc1, sc2), int32 arrays."""
        a = [np.ascontiguousarray(v, dtype=np.int32).reshape(-1) for v in (start, end, type_)]
        k = a[0].size
        out = [np.zeros(max(k, 1), dtype=np.int32) for _ in range(4)]
        self._check(self.lib.rsi_hot_pin_calls(self.ctx, int(m), k, *[v.ctypes.data for v in a], *[v.ctypes.data for v in out]))
        return tuple(v[:k] for v in out)

    def pin_stats(self):
        """The CIGAR table of the last load armed for pin, its sample and its last pin_calls (rsi_hot_last_pin_stats); records == 0:
        no table."""
        st = RsiPinStats()
        self._check(self.lib.rsi_hot_last_pin_stats(self.ctx, C.byref(st)))
        return self._pin_dict(st)

    def geno_calls(self, m, start, end):
        """The copy-number statistics of regions of the last run's chromosome (rsi_hot_geno_calls): start / end are 1-based inclusive
        reference coordinates; a GENO_RECORD array, one record per region."""
        a = [np.ascontiguousarray(v, dtype=np.int32).reshape(-1) for v in (start, end)]
        assert a[0].size == a[1].size
        k = a[0].size
        out = np.zeros(max(k, 1), dtype=GENO_RECORD)
        self._check(self.lib.rsi_hot_geno_calls(self.ctx, int(m), k, a[0].ctypes.data, a[1].ctypes.data, out.ctypes.data))
        return out[:k]

    def debug_geno(self, depth, storage, lo, hi, flo0, fhi0, flo1, fhi1, tile=0):
        """The same kernels over a host array and explicit half-open compacted ranges (test hook, rsi_hot_debug_geno): the body
        [lo, hi), the flank's pieces [flo0, fhi0) and [flo1, fhi1) per job; tile: values per tile (0: the default).  A GENO_RECORD
        array (chrom_median 0)."""
        d = np.ascontiguousarray(depth, dtype=np.int32)
        a = [np.ascontiguousarray(v, dtype=np.int32).reshape(-1) for v in (lo, hi, flo0, fhi0, flo1, fhi1)]
        k = a[0].size
        assert all(v.size == k for v in a)
        out = np.zeros(max(k, 1), dtype=GENO_RECORD)
        self._check(self.lib.rsi_hot_debug_geno(self.ctx, d.ctypes.data, d.size, int(storage), *[v.ctypes.data for v in a], k, int(tile),
                                                out.ctypes.data))
        return out[:k]

    def geno_stats(self):
        """Launches, jobs, tiles, passes, bytes held and ms of the context's last geno_calls / debug_geno (rsi_hot_last_geno_stats)."""
        st = RsiGenoStats()
        self._check(self.lib.rsi_hot_last_geno_stats(self.ctx, C.byref(st)))
        return {k: getattr(st, k) for k, _ in RsiGenoStats._fields_}

    # ---- plot data: the numbers of planned figures from an array in HBM ----
    def plot_depth(self, d_depth_ptr, n, batch):
        """Fills a PlotBatch from int32[n] in HBM (rsi_hot_plot_depth); the batch can then write its files."""
        self._check(self.lib.rsi_hot_plot_depth(self.ctx, C.c_void_p(d_depth_ptr), int(n), batch._h))

    def plot_run(self, res, batch):
        """Fills a PlotBatch from the depth the run of `res` left in this context, expanded on the device (rsi_hot_plot_run)."""
        self._check(self.lib.rsi_hot_plot_run(self.ctx, res._h, batch._h))

    def debug_plot(self, depth, batch, tile=0, workspace_bytes=0):
        """plot_depth of a host array (test hook, rsi_hot_debug_plot); tile: values per window-sum tile, workspace_bytes: what a
        batch of calls may take on the device (0: the defaults)."""
        d = np.ascontiguousarray(depth, dtype=np.int32)
        self._check(self.lib.rsi_hot_debug_plot(self.ctx, d.ctypes.data, d.size, int(tile), int(workspace_bytes), batch._h))

    def debug_plot_expand(self, rdc, regions, n, storage=4):
        """rsi_plot_expand on the device (test hook, rsi_hot_debug_plot_expand): compacted values and (start, end) pairs -> int32[n]."""
        v = np.ascontiguousarray(rdc, dtype=np.int32)
        r = np.ascontiguousarray(regions, dtype=np.int32).reshape(-1)
        out = np.zeros(int(n), dtype=np.int32)
        self._check(self.lib.rsi_hot_debug_plot_expand(self.ctx, v.ctypes.data if v.size else None, v.size, int(storage),
                                                       r.ctypes.data if r.size else None, r.size // 2, out.ctypes.data, int(n)))
        return out

    def plot_stats(self):
        """launches, batches, tiles, calls, queries, bytes up / down, bytes held, ms and expand_ms of the context's last plot call
        (rsi_hot_last_plot_stats)."""
        st = RsiPlotStats()
        self._check(self.lib.rsi_hot_last_plot_stats(self.ctx, C.byref(st)))
        return {k: getattr(st, k) for k, _ in RsiPlotStats._fields_}

    # ---- `depth`: a per-base depth array in HBM summed up without a run ----
    def loaded_depth(self):
        """(device pointer, n) of the array the last load_depth_text / load_depth_bam (or a depth hook) left in the context's input
        buffer (rsi_hot_loaded_depth)."""
        p, n = C.c_void_p(), C.c_int64()
        self._check(self.lib.rsi_hot_loaded_depth(self.ctx, C.byref(p), C.byref(n)))
        return p.value, n.value

    @staticmethod
    def _regions(start, end):
        a = [np.ascontiguousarray(v, dtype=np.int64).reshape(-1) for v in (start, end)]
        assert a[0].size == a[1].size
        return a[0], a[1], a[0].size

    def depth_summary(self, d_depth_ptr, n, dist=True):
        """One pass over int32[n] in HBM (rsi_hot_depth_summary): (a DEPTH_SUMMARY record, the 65536-bin distribution as int64 or
        None).  A negative depth raises RsiError."""
        out = np.zeros(1, dtype=DEPTH_SUMMARY)
        bins = np.zeros(DEPTH_BINS, dtype=np.int64) if dist else None
        self._check(self.lib.rsi_hot_depth_summary(self.ctx, C.c_void_p(d_depth_ptr), int(n), out.ctypes.data,
                                                   bins.ctypes.data if dist else None, DEPTH_BINS if dist else 0))
        return out[0], bins

    def depth_regions(self, d_depth_ptr, n, start, end):
        """n, sum, min, max of regions [start, end) of int32[n] in HBM, each clipped to [0, n) (rsi_hot_depth_regions): a
        DEPTH_REGION array."""
        s, e, k = self._regions(start, end)
        out = np.zeros(max(k, 1), dtype=DEPTH_REGION)
        self._check(self.lib.rsi_hot_depth_regions(self.ctx, C.c_void_p(d_depth_ptr), int(n), k, s.ctypes.data, e.ctypes.data, out.ctypes.data))
        return out[:k]

    def write_window_track(self, d_depth_ptr, n, chrom, W, path, append=False, format=None):
        """The mean depth of every window of W bases of int32[n] in HBM as lines of `chrom` (rsi_hot_write_window_track)."""
        st = RsiTrackStats()
        with self._track_format_for(format):
            self._check(self.lib.rsi_hot_write_window_track(self.ctx, C.c_void_p(d_depth_ptr), int(n), self._name_bytes(chrom), int(W),
                                                            os.fsencode(path), int(bool(append)), C.byref(st)))
        return {f[0]: getattr(st, f[0]) for f in RsiTrackStats._fields_}

    def write_region_track(self, d_depth_ptr, n, chrom, start, end, path, append=False, format=None):
        """The mean depth of explicit regions, in the order given (rsi_hot_write_region_track)."""
        s, e, k = self._regions(start, end)
        st = RsiTrackStats()
        with self._track_format_for(format):
            self._check(self.lib.rsi_hot_write_region_track(self.ctx, C.c_void_p(d_depth_ptr), int(n), self._name_bytes(chrom), k, s.ctypes.data,
                                                            e.ctypes.data, os.fsencode(path), int(bool(append)), C.byref(st)))
        return {f[0]: getattr(st, f[0]) for f in RsiTrackStats._fields_}

    def depth_stats(self):
        """launches, workgroups (or tiles), bytes held, ms and kernel_ms of the context's last depth call (rsi_hot_last_depth_stats)."""
        st = RsiDepthStats()
        self._check(self.lib.rsi_hot_last_depth_stats(self.ctx, C.byref(st)))
        return {k: getattr(st, k) for k, _ in RsiDepthStats._fields_}

    def debug_depth_summary(self, values, span=0, dist=True):
        """depth_summary of a host array (test hook, rsi_hot_debug_depth_summary); span: values per workgroup (0: the default)."""
        v = np.ascontiguousarray(values, dtype=np.int32)
        out = np.zeros(1, dtype=DEPTH_SUMMARY)
        bins = np.zeros(DEPTH_BINS, dtype=np.int64) if dist else None
        rc = self.lib.rsi_hot_debug_depth_summary(self.ctx, v.ctypes.data if v.size else None, v.size, int(span), out.ctypes.data,
                                                  bins.ctypes.data if dist else None, DEPTH_BINS if dist else 0)
        self.last_depth_summary = out[0]   # (on a refusal its `negative` says how many)
        self._check(rc)
        return out[0], bins

    def debug_depth_regions(self, values, start, end, tile=0):
        """depth_regions of a host array (test hook, rsi_hot_debug_depth_regions); tile: values per tile (0: the default)."""
        v = np.ascontiguousarray(values, dtype=np.int32)
        s, e, k = self._regions(start, end)
        out = np.zeros(max(k, 1), dtype=DEPTH_REGION)
        self._check(self.lib.rsi_hot_debug_depth_regions(self.ctx, v.ctypes.data if v.size else None, v.size, int(tile), k, s.ctypes.data,
                                                         e.ctypes.data, out.ctypes.data))
        return out[:k]

    def debug_region_track(self, values, chrom, W=0, start=(), end=(), span=0, tile=0, slice_lines=0, pos0=0, format=None):
        """The window (W > 0) or region (W == 0) lines of a host array through the device's writer (test hook,
        rsi_hot_debug_region_track): (bytes, stats).  With the format "bgzf" the bytes are the BGZF members of the text."""
        v = np.ascontiguousarray(values, dtype=np.int32)
        s, e, k = self._regions(start, end)
        name = self._name_bytes(chrom)
        lines = (-(-v.size // min(int(W), max(v.size, 1))) if v.size else 0) if W > 0 else k
        cap = lines * (len(name) + 4 + 2 * 20 + 23 + 64) + 64   # room for every line at its longest, in a member of its own
        st = RsiTrackStats()
        out = np.zeros(max(cap, 1), dtype=np.uint8)
        with self._track_format_for(format):
            n = self.lib.rsi_hot_debug_region_track(self.ctx, v.ctypes.data if v.size else None, v.size, name, int(W), k, s.ctypes.data, e.ctypes.data,
                                                    int(span), int(tile), int(slice_lines), int(pos0), out.ctypes.data, cap, C.byref(st))
        if n < 0:
            self._check(int(n))
        if n > cap:
            raise RsiError(-6, "region track: more text than its lines can take")
        return out[:n].tobytes(), {f[0]: getattr(st, f[0]) for f in RsiTrackStats._fields_}

    @staticmethod
    def _pin_arrays(cigars):
        lq, coff, pool = (np.ascontiguousarray(np.asarray(a).astype(np.int64) & 0xffffffff, dtype=np.uint32) for a in cigars)
        return lq.view(np.int32), coff, pool

    def debug_pin_sample(self, table, cigars, tid_len, rd_cap=0):
        """pin_sample over a caller's pair table and cigars = (lq, coff, pool) (test hook, rsi_hot_debug_pin_sample).  Returns
        (stats, rd, drd): the last stretch's arrays from its start on, rd_cap entries at the most."""
        arrs = self._pair_arrays(table)
        lq, coff, pool = self._pin_arrays(cigars)
        st = RsiPinStats()
        rd, drd = np.zeros(max(rd_cap, 1), dtype=np.int32), np.zeros(max(rd_cap, 1), dtype=np.int32)
        self._check(self.lib.rsi_hot_debug_pin_sample(self.ctx, arrs[0].size, *[a.ctypes.data for a in arrs], lq.ctypes.data, coff.ctypes.data, pool.ctypes.data,
                                                      pool.size, int(tid_len), C.byref(st), rd.ctypes.data, drd.ctypes.data, int(rd_cap)))
        return self._pin_dict(st), rd[:rd_cap], drd[:rd_cap]

    def debug_pin_calls(self, table, cigars, tid_len, m, l_qseq, drd_sd, start, end, type_):
        """pin_calls over a caller's tables with the sample's two results given (test hook, rsi_hot_debug_pin_calls)."""
        arrs = self._pair_arrays(table)
        lq, coff, pool = self._pin_arrays(cigars)
        a = [np.ascontiguousarray(v, dtype=np.int32).reshape(-1) for v in (start, end, type_)]
        k = a[0].size
        out = [np.zeros(max(k, 1), dtype=np.int32) for _ in range(4)]
        self._check(self.lib.rsi_hot_debug_pin_calls(self.ctx, arrs[0].size, *[v.ctypes.data for v in arrs], lq.ctypes.data, coff.ctypes.data, pool.ctypes.data,
                                                     pool.size, int(tid_len), int(m), int(l_qseq), float(drd_sd), k, *[v.ctypes.data for v in a],
                                                     *[v.ctypes.data for v in out]))
        return tuple(v[:k] for v in out)

    def bam_read_stats(self):
        """The record reader's side of the last BAM load (rsi_hot_last_bam_read_stats): mode ("host" / "device"), and for the
        device mode chunks, members, segments, guessed, rewalked, passed, t_upload_ms, t_inflate_ms, t_find_ms."""
        st = RsiBamReadStats()
        self._check(self.lib.rsi_hot_last_bam_read_stats(self.ctx, C.byref(st)))
        d = {f[0]: getattr(st, f[0]) for f in RsiBamReadStats._fields_ if f[0] != "pad"}
        d["mode"] = {v: k for k, v in BAM_READ_MODES.items()}.get(d["mode"], d["mode"])
        return d

    def run_bam(self, params, bam, chrom, fasta, minq=0, min_baseq=13, exclude=None):
        f = np.ascontiguousarray(fasta, dtype=np.uint8)
        if exclude is not None:
            self.set_exclude(exclude)
        out = C.c_void_p()
        st = RsiBamStats()
        self._check(self.lib.rsi_hot_run_bam(self.ctx, C.byref(params), os.fsencode(bam), chrom.encode(), int(minq), int(min_baseq),
                                             f.ctypes.data, f.size, C.byref(out), C.byref(st)))
        res = Result(self.lib, out)
        res.bam_stats = {f_[0]: getattr(st, f_[0]) for f_ in RsiBamStats._fields_}
        return res

    def run_device(self, params, d_depth_ptr, d_fasta_ptr, n, exclude=None):
        """Inputs already in HBM (raw device pointers, 16-byte aligned); exclude: as for run."""
        out = C.c_void_p()
        if exclude is not None:
            self.set_exclude(exclude)
        self._check(self.lib.rsi_hot_run_device(self.ctx, C.byref(params), C.c_void_p(d_depth_ptr), C.c_void_p(d_fasta_ptr),
                                                n, C.byref(out)))
        return Result(self.lib, out)

    def fetch(self, name):
        for fn, ct, dt in ((self.lib.rsi_hot_fetch_i32, C.c_int32, np.int32), (self.lib.rsi_hot_fetch_f32, C.c_float, np.float32),
                           (self.lib.rsi_hot_fetch_i64, C.c_int64, np.int64)):
            n = fn(self.ctx, name.encode(), None, 0)
            if n >= 0:
                out = np.zeros(n, dtype=dt)
                k = fn(self.ctx, name.encode(), out.ctypes.data_as(C.POINTER(ct)), n)
                if k < 0:
                    raise RsiError(int(k), self.lib.rsi_hot_last_error(self.ctx).decode())
                return out
        raise KeyError(name)

    TRACK_DEPTHS = {"raw": 0, "gc": 1}

    @staticmethod
    def _name_bytes(chrom):
        return chrom if isinstance(chrom, bytes) else chrom.encode()

    def set_track_format(self, format):
        """The format of this context's track calls from now on (rsi_hot_set_track_format): "text" / 0 or "bgzf" / 1."""
        f = TRACK_FORMATS.get(format, format)
        if isinstance(f, str):
            raise ValueError("track format: 'text' or 'bgzf'")
        self._check(self.lib.rsi_hot_set_track_format(self.ctx, int(f)))
        self._track_format = int(f)

    @contextlib.contextmanager
    def _track_format_for(self, format):
        """format=None: the context's setting; else that format for one call, the setting as it was afterwards."""
        before = getattr(self, "_track_format", 0)
        if format is not None:
            self.set_track_format(format)
        try:
            yield
        finally:
            if format is not None:
                self.set_track_format(before)

    def set_track_index(self, index):
        """Every BGZF track call of this context from now on adds its chromosome to `index` (a TrackIndex; None: no indexing,
        the default) -- rsi_hot_set_track_index.  The debug_track / debug_bin_track hooks do too, for a file that starts at 0."""
        self._check(self.lib.rsi_hot_set_track_index(self.ctx, index.handle if index is not None else None))
        self._track_index = index   # kept alive while the context points at it

    def deflate_stats(self):
        """The compressed side of the last track call or debug_deflate (rsi_hot_last_deflate_stats): members, stored_members,
        text_bytes, file_bytes (no end-of-file block), t_kernel_ms of the deflate and pack launches; zeros after a text call."""
        st = RsiDeflateStats()
        self._check(self.lib.rsi_hot_last_deflate_stats(self.ctx, C.byref(st)))
        return {f[0]: getattr(st, f[0]) for f in RsiDeflateStats._fields_}

    def debug_deflate(self, text):
        """`text` (any bytes) as BGZF members of 65280 text bytes through the deflate and pack kernels alone (test hook,
        rsi_hot_debug_deflate): (bytes, stats).  No end-of-file block."""
        t = np.frombuffer(bytes(text), dtype=np.uint8)
        cap = t.size + 31 * (t.size // 65280 + 1)
        out = np.zeros(max(cap, 1), dtype=np.uint8)
        st = RsiDeflateStats()
        k = self.lib.rsi_hot_debug_deflate(self.ctx, t.ctypes.data if t.size else None, t.size, out.ctypes.data, cap, C.byref(st))
        if k < 0:
            self._check(int(k))
        if k > cap:
            raise RsiError(-6, "deflate: more bytes than stored members take")
        return out[:k].tobytes(), {f[0]: getattr(st, f[0]) for f in RsiDeflateStats._fields_}

    def write_track(self, which, chrom, path, append=False, format=None):
        """The last run's depth as bedGraph lines of `chrom` (rsi_hot_write_track), replacing `path` or appended to it.
        which: 0 / "raw" = the depth the run read, 1 / "gc" = the GC-adjusted depth (fetch("rd_gc"); RsiError after a
        -NOGC run).  format: "text" or "bgzf" for this call (None: the context's setting, set_track_format); a BGZF file is
        complete once bgzf_write_eof(path) has ended it.  Returns the statistics (RsiTrackStats) as a dict."""
        st = RsiTrackStats()
        w = self.TRACK_DEPTHS.get(which, which)
        with self._track_format_for(format):
            self._check(self.lib.rsi_hot_write_track(self.ctx, int(w), self._name_bytes(chrom), os.fsencode(path), int(bool(append)), C.byref(st)))
        return {f[0]: getattr(st, f[0]) for f in RsiTrackStats._fields_}

    def write_track_device(self, d_values_ptr, n, chrom, path, append=False, format=None):
        """Any int32[n] in HBM (a raw device pointer) as bedGraph lines of `chrom` (rsi_hot_write_track_device)."""
        st = RsiTrackStats()
        with self._track_format_for(format):
            self._check(self.lib.rsi_hot_write_track_device(self.ctx, C.c_void_p(d_values_ptr), int(n), self._name_bytes(chrom), os.fsencode(path),
                                                            int(bool(append)), C.byref(st)))
        return {f[0]: getattr(st, f[0]) for f in RsiTrackStats._fields_}

    def debug_track(self, values, chrom, pos0=0, slice_bases=0, format=None):
        """The bedGraph text of a host int32 array through the device's track writer (test hook, rsi_hot_debug_track):
        (bytes, stats).  pos0: added to every coordinate; slice_bases > 0: the slice length to work in.  With the format
        "bgzf" the bytes are the BGZF members of that text."""
        with self._track_format_for(format):
            return self._debug_track(values, chrom, pos0, slice_bases)

    def _debug_track(self, values, chrom, pos0, slice_bases):
        v = np.ascontiguousarray(values, dtype=np.int32)
        name = self._name_bytes(chrom)
        # room for every line at its longest; the call says when that was not enough
        lines = (int(np.count_nonzero(v[1:] != v[:-1])) + 1) if v.size else 0
        cap = lines * (len(name) + 4 + 2 * 20 + 11) + 64   # (a member's frame around a short text)
        st = RsiTrackStats()
        for _ in range(2):
            out = np.zeros(max(cap, 1), dtype=np.uint8)
            k = self.lib.rsi_hot_debug_track(self.ctx, v.ctypes.data if v.size else None, v.size, name, int(pos0), int(slice_bases),
                                             out.ctypes.data, cap, C.byref(st))
            if k < 0:
                self._check(int(k))
            if k <= cap:
                break
            cap = int(k)
        return out[:k].tobytes(), {f[0]: getattr(st, f[0]) for f in RsiTrackStats._fields_}

    BIN_TRACK_VALUES = {"median": 0, "ratio": 1}

    def write_bin_track(self, which, chrom, path, append=False, format=None):
        """The last run's bins as bedGraph lines of `chrom` (rsi_hot_write_bin_track), replacing `path` or appended to it.
        which: 0 / "median" = every bin's median, 1 / "ratio" = the median over the chromosome's median, three decimals.
        Returns the statistics (RsiTrackStats, n = the number of bins) as a dict."""
        st = RsiTrackStats()
        w = self.BIN_TRACK_VALUES.get(which, which)
        with self._track_format_for(format):
            self._check(self.lib.rsi_hot_write_bin_track(self.ctx, int(w), self._name_bytes(chrom), os.fsencode(path), int(bool(append)), C.byref(st)))
        return {f[0]: getattr(st, f[0]) for f in RsiTrackStats._fields_}

    def debug_bin_track(self, values, m, n, pairs, median2, which, name, slice_bins=0, format=None):
        """The bin track of host values[nb] (bins of m compacted bases of a chromosome of n bases whose removed regions are the
        inclusive (start, end) `pairs`) through the device's writer (test hook, rsi_hot_debug_bin_track): (bytes, stats)."""
        with self._track_format_for(format):
            return self._debug_bin_track(values, m, n, pairs, median2, which, name, slice_bins)

    def _debug_bin_track(self, values, m, n, pairs, median2, which, name, slice_bins):
        v = np.ascontiguousarray(values, dtype=np.int32)
        pr = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1)
        nm = self._name_bytes(name)
        w = self.BIN_TRACK_VALUES.get(which, which)
        cap = (v.size + pr.size // 2) * (len(nm) + 4 + 2 * 20 + 18) + 64   # room for every piece at its longest (and a member's frame)
        st = RsiTrackStats()
        out = np.zeros(max(cap, 1), dtype=np.uint8)
        k = self.lib.rsi_hot_debug_bin_track(self.ctx, v.ctypes.data if v.size else None, v.size, int(m), int(n),
                                             pr.ctypes.data if pr.size else None, pr.size // 2, int(median2), int(w), nm, int(slice_bins),
                                             out.ctypes.data, cap, C.byref(st))
        if k < 0:
            self._check(int(k))
        if k > cap:
            raise RsiError(-6, "bin track: more text than its pieces can take")
        return out[:k].tobytes(), {f[0]: getattr(st, f[0]) for f in RsiTrackStats._fields_}

    def phase_times(self):
        names = (C.c_char_p * 64)()
        ms = (C.c_double * 64)()
        k = self.lib.rsi_hot_phase_times(self.ctx, names, ms, 64)
        return [(names[i].decode(), float(ms[i])) for i in range(min(k, 64))]

    def kernel_times(self):
        names = (C.c_char_p * 4096)()
        ms = (C.c_float * 4096)()
        k = self.lib.rsi_hot_kernel_times(self.ctx, names, ms, 4096)
        return [(names[i].decode(), float(ms[i])) for i in range(min(k, 4096))]


class RsiPool:
    """Several chromosomes in flight on one GPU (rsi_pool_*): `workers` host threads, each with its
    own stream and workspace; the HBM-bound per-base phase is taken in turns."""

    def __init__(self, device=0, workers=8):
        self.lib = load_library()
        st = C.c_int(0)
        self.pool = self.lib.rsi_pool_create(device, workers, C.byref(st))
        if not self.pool:
            raise RsiError(st.value, self.lib.rsi_hot_last_error(None).decode())
        self.times = RsiBatchTimes()

    def close(self):
        if getattr(self, "pool", None):
            self.lib.rsi_pool_destroy(self.pool)
            self.pool = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def hw_queues(self):
        """The hardware queues the process had asked for when the pool was made (rsi_pool_hw_queues): with more workers than
        this minus two, workers share queues and the library has said so on stderr."""
        return self.lib.rsi_pool_hw_queues(self.pool)

    def set_timing(self, on=True):
        self.lib.rsi_pool_set_timing(self.pool, int(on))

    def set_timing_kernel(self, name):
        """The kernel timing mode 3 brackets (a name of kernel_table())."""
        self.lib.rsi_pool_set_timing_kernel(self.pool, name.encode())

    def set_schedule(self, isolate=False, streamers=0):
        """isolate: per-base phases run alone on the chip (clean kernel timings); streamers: per-base phases in flight (0 = keep)."""
        self.lib.rsi_pool_set_schedule(self.pool, 1 if isolate else 0, int(streamers))

    def reset_times(self):
        self.times = RsiBatchTimes()

    def run(self, params, chroms, collect_times=False, host=False):
        """chroms: list of (d_depth_ptr, d_fasta_ptr, n): device pointers, or with host=True host pointers (pinned for
        asynchronous transfers).  Returns a list of Result in input order."""
        k = len(chroms)
        dp = (C.c_void_p * k)(*[C.c_void_p(c[0]) for c in chroms])
        fp = (C.c_void_p * k)(*[C.c_void_p(c[1]) for c in chroms])
        nn = (C.c_int64 * k)(*[c[2] for c in chroms])
        out = (C.c_void_p * k)()
        st = (C.c_int * k)()
        fn = self.lib.rsi_pool_run_host if host else self.lib.rsi_pool_run
        rc = fn(self.pool, C.byref(params), k, dp, fp, nn, out, st, C.byref(self.times) if collect_times else None)
        if rc != RSI_OK:
            for i in range(k):
                if out[i]:
                    self.lib.rsi_result_free(out[i])
            raise RsiError(rc, self.lib.rsi_pool_last_error(self.pool).decode())
        return [Result(self.lib, C.c_void_p(out[i])) for i in range(k)]

    def submit(self, params, chroms, collect_times=False):
        """Queue a run (rsi_pool_submit) and return a handle for wait(): the chromosomes of queued runs go to the workers in
        submission order, so consecutive samples overlap.  chroms as for run() (device pointers)."""
        k = len(chroms)
        h = {"k": k, "params": params,
             "dp": (C.c_void_p * k)(*[C.c_void_p(c[0]) for c in chroms]), "fp": (C.c_void_p * k)(*[C.c_void_p(c[1]) for c in chroms]),
             "nn": (C.c_int64 * k)(*[c[2] for c in chroms]), "out": (C.c_void_p * k)(), "st": (C.c_int * k)()}
        h["times"] = self.times if collect_times else None   # the run writes into it when it finishes: alive as long as the handle
        h["ticket"] = self.lib.rsi_pool_submit(self.pool, C.byref(params), k, h["dp"], h["fp"], h["nn"], h["out"], h["st"],
                                               C.byref(h["times"]) if collect_times else None)
        if not h["ticket"]:
            raise RsiError(-2, "rsi_pool_submit: bad arguments")
        return h

    def wait(self, h):
        """The results of a submitted run, in input order (the calling thread works as one of the pool's workers meanwhile)."""
        rc = self.lib.rsi_pool_wait(self.pool, h["ticket"])
        k, out = h["k"], h["out"]
        if rc != RSI_OK:
            for i in range(k):
                if out[i]:
                    self.lib.rsi_result_free(out[i])
            raise RsiError(rc, self.lib.rsi_pool_last_error(self.pool).decode())
        return [Result(self.lib, C.c_void_p(out[i])) for i in range(k)]

    def kernel_table(self):
        t = self.times
        return {t.kernel_name[i].decode(): (t.kernel_ms[i], t.kernel_launches[i], t.kernel_bases[i]) for i in range(t.nkernels)}

    def phase_table(self):
        t = self.times
        return {t.phase_name[i].decode(): t.phase_ms[i] for i in range(t.nphases)}


class PlotBatch:
    """Calls planned as gnuplot figures against an array of n values (rsi_plot_batch_*): add() plans a call and
    returns 0 or what the writer refuses; a fill -- fill_host(array), RsiHot.plot_depth / plot_run / debug_plot -- provides the
    numbers; write(i, ...) then leaves call i's .dat and .gp files, byte for byte those of rsi_plot_write_files."""

    def __init__(self, n, m, minmlen=2.0, chklen=2.0):
        self.lib = load_library()
        self._h = self.lib.rsi_plot_batch_new(int(n), int(m), float(minmlen), float(chklen))
        if not self._h:
            raise RsiError(-2, "plot batch: bad array length or bin size")

    def close(self):
        if self._h:
            self.lib.rsi_plot_batch_free(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def add(self, start, end, type_=0, call=None):
        """Plans one call: start / end as in the output rows; call: an RsiCall whose length / type / p1 the data file's first line
        prints (default: cnv_st's, length 0 and p1 1)."""
        if call is not None:
            return self.lib.rsi_plot_batch_add(self._h, C.byref(call))
        return self.lib.rsi_plot_batch_add_span(self._h, int(start), int(end), int(type_))

    def __len__(self):
        return self.lib.rsi_plot_batch_size(self._h)

    def refusal(self, i):
        return self.lib.rsi_plot_batch_refusal(self._h, int(i))

    def refusal_text(self, i):
        return self.lib.rsi_plot_refusal_text(self.refusal(i)).decode()

    def queries(self):
        return self.lib.rsi_plot_batch_queries(self._h)

    def fill_host(self, depth):
        d = np.ascontiguousarray(depth, dtype=np.int32)
        rc = self.lib.rsi_plot_batch_fill_host(self._h, d.ctypes.data, d.size)
        if rc != RSI_OK:
            raise RsiError(rc, "plot batch: the array is not the length the batch was planned for")

    def chrom_median(self):
        return self.lib.rsi_plot_batch_chrom_median(self._h)

    def compare(self, other):
        """0 when both filled batches hold the same numbers for every call, else 1 + the first call that differs."""
        return self.lib.rsi_plot_batch_compare(self._h, other._h)

    def write(self, i, title, datfile, gpfile, imgfile, format="ps", gnuplot_version=5.0):
        """Call i's files from the last fill; False for a refused call (no file is written)."""
        return self.lib.rsi_plot_batch_write(self._h, int(i), title.encode(), format.encode(), float(gnuplot_version), os.fsencode(datfile),
                                             os.fsencode(gpfile), os.fsencode(imgfile)) == RSI_OK


class GenomeText:
    """Streaming reader of a whole-genome depth file, "RNAME pos depth" lines (rsi_genome_text_*): iterating yields
    (name, d_depth_ptr, n, stats) per chromosome in the file's order, its depth resident in HBM.  names / lengths: the
    reference's sequences (the .fai's), looked up as read_fasta does; a name that is not among them comes with d_depth_ptr
    None; names with "MT" or "." are skipped.  stats carries the slice counts and the depth buffer's "slot".

    auto_release=True: a chromosome's buffer is given back when the next one is asked for (read it inside the loop, e.g.
    with depth()).  auto_release=False: the caller gives it back with release(slot); at most max_resident buffers exist, and
    the reader needs one for each new chromosome.

    samples=[k1, k2, ...]: a cohort file, "RNAME pos d1 ... dK" (rsi_genome_text_open_samples): sample j is depth column
    samples[j] (1-based); the stats are every sample's, d_depth_ptr is sample 0's, and sample_ptr() / sample_depth() give
    sample j.  The reader may use fewer than max_resident buffers when device memory holds fewer (self.max_resident).

    bedgraph=True: a bedGraph file, "RNAME start end d" (rsi_genome_bedgraph_open): each line is read as the lines
    "RNAME p d", p = start + 1 .. end; the stats are those of that expanded file, bytes aside.  index=PATH (with bedgraph=True,
    a BGZF file): the .tbi or .csi beside it; only the members that hold the lines of `names` are read
    (rsi_genome_bedgraph_open_indexed), index_range() says which."""

    def __init__(self, path, names, lengths, chunk_bytes=0, device=0, max_resident=2, auto_release=True, samples=None, bedgraph=False,
                 index=None):
        self.lib = load_library()
        enc = [n.encode() for n in names]
        self._names = (C.c_char_p * max(len(enc), 1))(*enc)
        self._lens = (C.c_int64 * max(len(enc), 1))(*[int(x) for x in lengths])
        st = C.c_int(0)
        if bedgraph and samples is not None:
            raise ValueError("a bedGraph file has one depth column")
        if index is not None and not bedgraph:
            raise ValueError("an index serves a bedGraph file")
        if index is not None:
            self.g = self.lib.rsi_genome_bedgraph_open_indexed(int(device), os.fsencode(path), os.fsencode(index), len(enc), self._names, self._lens,
                                                               int(max_resident), int(chunk_bytes), C.byref(st))
        elif samples is None:
            opener = self.lib.rsi_genome_bedgraph_open if bedgraph else self.lib.rsi_genome_text_open
            self.g = opener(int(device), os.fsencode(path), len(enc), self._names, self._lens, int(max_resident), int(chunk_bytes), C.byref(st))
        else:
            cols = (C.c_int32 * max(len(samples), 1))(*[int(k) for k in samples])
            self.g = self.lib.rsi_genome_text_open_samples(int(device), os.fsencode(path), len(enc), self._names, self._lens, cols,
                                                           len(samples), int(max_resident), int(chunk_bytes), C.byref(st))
        if not self.g:
            raise RsiError(st.value, self.lib.rsi_hot_last_error(None).decode())
        self.samples = list(samples) if samples is not None else [1]
        self.max_resident = self.lib.rsi_genome_text_max_resident(self.g)
        self.auto_release = auto_release
        self._last = None

    def close(self):
        if getattr(self, "g", None):
            self.lib.rsi_genome_text_close(self.g)
            self.g = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def release(self, slot):
        if slot is not None and slot >= 0:
            self.lib.rsi_genome_text_release(self.g, int(slot))

    def next(self):
        """(name, d_depth_ptr or None, n, stats), or None at the end of the file; raises on errors (RsiError)."""
        if self.auto_release and self._last is not None:
            self.release(self._last)
            self._last = None
        c = RsiGenomeChrom()
        rc = self.lib.rsi_genome_text_next(self.g, C.byref(c))
        if rc == 0:
            return None
        if rc < 0:
            raise RsiError(rc, self.lib.rsi_genome_text_last_error(self.g).decode())
        stats = {f[0]: getattr(c.stats, f[0]) for f in RsiTextStats._fields_ if f[0] != "pad"}
        stats["slot"] = c.slot
        if c.slot >= 0:
            self._last = c.slot
        return c.name.decode(), (c.d_depth if c.slot >= 0 else None), c.n, stats

    def __iter__(self):
        while True:
            item = self.next()
            if item is None:
                return
            yield item

    def depth(self, slot):
        """A handed-over chromosome's depth as a host int32 array."""
        n = self.lib.rsi_genome_text_copy_depth(self.g, int(slot), None, 0)
        if n < 0:
            raise RsiError(int(n), self.lib.rsi_genome_text_last_error(self.g).decode())
        out = np.zeros(n, dtype=np.int32)
        k = self.lib.rsi_genome_text_copy_depth(self.g, int(slot), out.ctypes.data, n)
        if k < 0:
            raise RsiError(int(k), self.lib.rsi_genome_text_last_error(self.g).decode())
        return out

    def sample_ptr(self, slot, j):
        """Sample j's depth of a handed-over chromosome: its device pointer (int32[n] in HBM)."""
        p = self.lib.rsi_genome_text_sample_depth(self.g, int(slot), int(j))
        if not p:
            raise RsiError(-2, f"no sample {j} in depth buffer {slot}")
        return p

    def sample_depth(self, slot, j):
        """Sample j's depth of a handed-over chromosome as a host int32 array."""
        n = self.lib.rsi_genome_text_copy_sample_depth(self.g, int(slot), int(j), None, 0)
        if n < 0:
            raise RsiError(int(n), self.lib.rsi_genome_text_last_error(self.g).decode())
        out = np.zeros(n, dtype=np.int32)
        k = self.lib.rsi_genome_text_copy_sample_depth(self.g, int(slot), int(j), out.ctypes.data, n)
        if k < 0:
            raise RsiError(int(k), self.lib.rsi_genome_text_last_error(self.g).decode())
        return out

    def index_range(self):
        """(begin, stop): the compressed bytes an indexed reader takes from its file (rsi_genome_text_index_range)."""
        b, e = C.c_int64(), C.c_int64()
        k = self.lib.rsi_genome_text_index_range(self.g, C.byref(b), C.byref(e))
        if k < 0:
            raise RsiError(k, "the reader was opened without an index")
        return b.value, e.value

    def inflate_stats(self):
        """The file's format and the inflate figures so far (see RsiHot.inflate_stats)."""
        st = RsiInflateStats()
        self.lib.rsi_genome_text_inflate_stats(self.g, C.byref(st))
        return _inflate_dict(st)

    def kernel_ms(self):
        """(boundary pass, parse pass): summed HIP-event milliseconds so far."""
        b, p = C.c_double(0), C.c_double(0)
        self.lib.rsi_genome_text_kernel_ms(self.g, C.byref(b), C.byref(p))
        return b.value, p.value


def run_genome_text(path, names, lengths, fasta, params=None, pool=None, device=0, workers=4, chunk_bytes=0, samples=None, bedgraph=False):
    """Every chromosome of a whole-genome depth file through an RsiPool, each submitted as soon as its depth is parsed:
    {name: Result} in the file's order (names not among `names` are left out).  fasta: {name: uint8 array} or a callable
    name -> uint8 array (the chromosome's sequence, length n).  samples=[k1, k2, ...] (a cohort file, see GenomeText): one
    such dict per sample, in the order of `samples`; all samples of a chromosome go to the pool as one batch.  bedgraph=True:
    a bedGraph file (see GenomeText)."""
    import torch
    params = params if params is not None else make_params()
    own = pool is None
    pool = pool or RsiPool(device, workers)
    get = fasta if callable(fasta) else fasta.__getitem__
    inflight = []   # (name, handle, slot, the device sequence: kept alive until the run is through)
    out = [{} for _ in (samples or [1])]
    g = GenomeText(path, names, lengths, chunk_bytes=chunk_bytes, device=device, max_resident=workers + 1, auto_release=False,
                   samples=samples, bedgraph=bedgraph)
    held = max(1, min(workers, g.max_resident - 1))

    def collect():
        name, h, slot, _ = inflight.pop(0)
        for j, r in enumerate(pool.wait(h)):
            out[j][name] = r
        g.release(slot)

    try:
        for name, d_depth, n, st in g:
            if d_depth is None:
                continue
            while len(inflight) >= held:
                collect()
            seq = np.ascontiguousarray(get(name), dtype=np.uint8)
            if seq.size != n:
                g.release(st["slot"])
                raise ValueError(f"{name}: sequence of {seq.size} bases, the reference index says {n}")
            d_fa = torch.from_numpy(seq).to(f"cuda:{device}")
            torch.cuda.synchronize(device)
            batch = [(d_depth if samples is None else g.sample_ptr(st["slot"], j), d_fa.data_ptr(), n) for j in range(len(out))]
            inflight.append((name, pool.submit(params, batch), st["slot"], d_fa))
        while inflight:
            collect()
    finally:
        for name, h, slot, _ in inflight:   # an error above: the queued runs still have to be waited for
            try:
                pool.wait(h)
            except RsiError:
                pass
        g.close()
        if own:
            pool.close()
    return out if samples is not None else out[0]
