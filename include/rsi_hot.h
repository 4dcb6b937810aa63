/* rsi_hot.h -- C ABI of the MI355X-native RSI read-depth CNV hot path (librsi_hot.so).
 *
 * The reference (yhwu/rsicnv) has no plugin / FFI interface; its hot path sits behind a seam of
 * free functions operating on `Array<int>& RD` plus `rsi::` globals, called from main's
 * per-chromosome loop (rsi.cpp:2189-2217).  One rsi_hot_run() call replaces, for one chromosome:
 *
 *   load_data_from_text, after its parse loop        loaddata.cpp:478-486, 519-531
 *     GC mask + get_noseq_regions                    loaddata.cpp:481-486, 243-273; readref.cpp:88
 *     checkgccontent / adjustgccontent               gccontent.cpp:95, 43
 *     apply_cap                                      loaddata.cpp:229
 *   concatenate_data                                 loaddata.cpp:48      (rsi.cpp:2200)
 *   rsi::RDmedian = _median(RD); rsi::RDsd = ...     rsi.cpp:2202-2203    (wufunctions.cpp:364, 766)
 *   detectcnv                                        rsi.cpp:1795         (rsi.cpp:2206)
 *   sd_filters                                       rsi.cpp:1753         (rsi.cpp:2208)
 *
 * Conventions: inputs are borrowed for the call; results are owned by the rsi_result and freed
 * by rsi_result_free; every entry point returns RSI_OK or a negative rsi_status and leaves a
 * message for rsi_hot_last_error().  There is NO CPU fallback: without a HIP device
 * rsi_hot_create() fails with RSI_ERR_NO_DEVICE.  One context per host thread / GPU; contexts are
 * independent (no shared mutable globals), so chromosomes can be processed concurrently.
 */
#ifndef RSI_HOT_H
#define RSI_HOT_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef enum rsi_status {
  RSI_OK = 0,
  RSI_ERR_NO_DEVICE = -1,    /* no HIP device / extension unusable: the product never falls back */
  RSI_ERR_BAD_ARG = -2,
  RSI_ERR_HIP = -3,          /* a HIP runtime call failed */
  RSI_ERR_TOO_SMALL = -4,    /* chromosome shorter than 20*202 bases under GC adjust (gccontent.cpp:66-71) */
  RSI_ERR_UNSUPPORTED = -5,  /* e.g. negative depth, a scan longer than 4 M lengths, N-run list overflow */
  RSI_ERR_INTERNAL = -6
} rsi_status;

/* rsi:: statics that the path reads (rsi.h:54-122, defaults rsi.cpp:34-98). */
typedef struct rsi_params {
  int32_t m;          /* -m      bin size, forced odd by the caller as rsi.cpp:2061-2064 does */
  int32_t gcadjust;   /* !-NOGC  */
  int32_t trans;      /* 0 = NBN (-NB, default), 1 = MED (-MED), 2 = ALL (-ALL) */
  int32_t merge;      /* !-nomerge */
  int32_t maxchkbp;   /* -maxchkbp */
  int32_t debug;      /* -debug */
  double cap;         /* -cap */
  double epsilon;     /* -e */
  double threshold;   /* -threshold */
  double chklen;      /* -reflen */
  double minmlen;
  double buffer;
  double p;
} rsi_params;

/* POD mirror of cnv_st (rsi.h:8-51); qscore is the SCORE column of cnv_format1 (rsi.cpp:583-615). */
typedef struct rsi_call {
  int32_t start, end;   /* 0-based indices on the reference (N regions re-inserted), inclusive */
  int32_t type;         /* 0 DEL, 1 DUP, 2 UNKNOWN (rsi.h:4-6) */
  int32_t geno, status, length, qscore, pad;
  double score, p1, cnvmed, cnvsd, cnviqr, refmed, refsd, refiqr;
} rsi_call;

/* Per-chromosome scalars the reference keeps in rsi:: globals or prints to its log. */
typedef struct rsi_chrom_stats {
  int64_t n;            /* chromosome length */
  int64_t n_compact;    /* after N-region removal (rsi::end) */
  int64_t nbins;
  int32_t n_noncode;    /* padded N regions */
  int32_t Lmax;         /* scan length actually used */
  double gc_rdmean;     /* "RD mean before GC adjust" (gccontent.cpp:154) */
  double cap_median;    /* median used by apply_cap (loaddata.cpp:233) */
  double RDmedian, RDsd;
  double nb_mad, nb_r, nb_tmin;
  double tmedian1, tsigma1, tlamda1;   /* first scan pass */
  double tmedian2, tsigma2, tlamda2;   /* second scan pass */
  int32_t trim_escapes; /* trim walks that left the array (the reference aborts there, App. A Q12) */
  int32_t inexact_sums; /* bins whose value breaks the exact-window-sum precondition */
  double t_device_ms;   /* wall time of the call, inputs already on the device */
  double t_kernels_ms;  /* sum of HIP-event times around the per-base kernels */
  int64_t byte_escapes; /* bases of depth >= 255: the per-base kernels fetch those from the int32 array instead of the byte copy */
  int32_t scan_tiles;        /* tiles of 256 bins per scan pass */
  int32_t scan_tiles_listed; /* tiles the detection passes of the (last) scan listed for the exact sweep, both passes together */
} rsi_chrom_stats;

typedef struct rsi_ctx rsi_ctx;
typedef struct rsi_result rsi_result;

/* Reference defaults (rsi.cpp:34-98). */
void rsi_default_params(rsi_params* p);

/* The process-wide setting the library depends on, applied to the environment: call it BEFORE the process's first HIP call
 * (the HIP runtime reads GPU_MAX_HW_QUEUES once, when it initialises; later the call changes the environment and nothing else).
 * It makes no HIP call itself.  A pool runs one stream per worker and wants each on a hardware queue of its own, so:
 *   GPU_MAX_HW_QUEUES missing, not a number, or below 32   -> set to 32;   32 or more -> left as it is (nothing above 32 is
 *   ever written);
 *   RSI_HOT_HW_QUEUES=keep   -> the environment is left exactly as found;
 *   RSI_HOT_HW_QUEUES=N      -> N clamped to 4 .. 32 is written, whatever was there (anything else in that variable is ignored).
 * A number is one to nine decimal digits and nothing else.  Returns the number GPU_MAX_HW_QUEUES holds afterwards, or 0 when
 * it holds none (possible under `keep` only: the runtime then uses its default of 4).  Not thread-safe
 * against other writers of the environment, like setenv itself. */
int rsi_hot_process_setup(void);

/* Context on HIP device `device`.  Returns NULL on failure; *status receives the reason. */
rsi_ctx* rsi_hot_create(int device, int* status);
void rsi_hot_destroy(rsi_ctx* ctx);
const char* rsi_hot_last_error(const rsi_ctx* ctx);   /* ctx may be NULL: last global error */

/* One chromosome, inputs in host memory: depth[n] raw per-base depth, fasta[n] sequence bytes. */
int rsi_hot_run(rsi_ctx* ctx, const rsi_params* p, const int32_t* depth, const uint8_t* fasta, int64_t n,
                rsi_result** out);

/* ---- Depth text ingestion on the device --------------------------------------------
 * Replaces the parse loop of load_data_from_text (loaddata.cpp:496-517): "pos depth" lines read as
 * libstdc++'s `iss >> pos >> d` reads them (an int outside its range is clamped and fails); empty lines
 * and '#' lines skipped; pos < 1 skipped; reading stops at the first pos >= n (the last base is never
 * set); RD[pos-1] = depth; positions that never appear stay 0.  The file is streamed to HBM in pinned
 * chunks and parsed by a kernel; files whose positions are not strictly increasing (where the order-
 * dependent rules matter) are parsed by the sequential host loop instead (stats->fallback = 1). */
typedef struct rsi_text_stats {
  int64_t bytes, lines, stored, beyond;   /* file size; lines with pos >= 1; lines stored; lines with pos >= n */
  int32_t fallback, pad;                  /* 1: parsed on the host (unsorted positions) */
  double t_total_ms, t_parse_kernel_ms;   /* wall time of the load; summed kernel time when timing is on */
} rsi_text_stats;
/* Parses `path` into the context's device depth buffer (int32[n]); rsi_hot_fetch_i32("depth_in") reads it back. */
int rsi_hot_load_depth_text(rsi_ctx* ctx, const char* path, int64_t n, rsi_text_stats* stats);
/* rsi_hot_load_depth_text + rsi_hot_run on the loaded depth: fasta[n] in host memory.  stats may be NULL. */
int rsi_hot_run_text(rsi_ctx* ctx, const rsi_params* p, const char* depth_path, const uint8_t* fasta, int64_t n,
                     rsi_result** out, rsi_text_stats* stats);

/* ---- Compressed depth files ------------------------------------------------------------------------------------
 * Both text readers (rsi_hot_load_depth_text / _run_text and rsi_genome_text_*) take plain text, BGZF (bgzip's output;
 * inflated on the device, CRC32 and ISIZE checked there) or ordinary gzip (single- or multi-member; inflated on the host
 * with zlib).  The format comes from the first bytes: 1f 8b 08 with FEXTRA holding a "BC" subfield of length 2 is BGZF, any
 * other 1f 8b start gzip, anything else text.  Depth, counts and rows are those of the text; rsi_text_stats.bytes and the
 * genome reader's byte ranges count text bytes.  A bad member (CRC32 / ISIZE mismatch, invalid deflate data, a member past
 * the end of the file, a non-BGZF member inside a BGZF file) is RSI_ERR_BAD_ARG naming its compressed offset. */
typedef struct rsi_inflate_stats {
  int32_t format;              /* 0 text, 1 BGZF, 2 gzip */
  int32_t eof_block;           /* BGZF: 1 when the file ends with the empty EOF member */
  int32_t input_error;         /* 1: the load failed on the compressed data itself (bad member, truncated file) */
  int32_t pad;
  int64_t compressed_bytes;    /* bytes of the file read */
  int64_t text_bytes;          /* bytes of text they gave */
  int64_t blocks;              /* BGZF members inflated on the device */
  double t_inflate_kernel_ms;  /* summed HIP-event time of the inflate launches (BGZF) */
  double t_host_inflate_ms;    /* wall time in zlib on the host (gzip) */
} rsi_inflate_stats;
/* The format and the inflate figures of the context's last rsi_hot_load_depth_text / rsi_hot_run_text / rsi_hot_inflate_bgzf. */
int rsi_hot_last_inflate_stats(const rsi_ctx* ctx, rsi_inflate_stats* out);
/* comp[0, comp_len): whole BGZF members, inflated on the device into out[0, out_cap).  Returns the text length (>= 0), or
 * an error code (out_cap too small: RSI_ERR_BAD_ARG).  For tests and tools. */
int64_t rsi_hot_inflate_bgzf(rsi_ctx* ctx, const uint8_t* comp, int64_t comp_len, uint8_t* out, int64_t out_cap,
                             rsi_inflate_stats* stats);

/* ---- Whole-genome depth text: "RNAME pos depth" lines, every chromosome in one file --------------------
 * (samtools depth -a, or mpileup | cut -f1,2,4).  A streaming reader that parses the file on the device and hands over each
 * chromosome's depth, resident in HBM, as soon as its last line has been parsed.  Lines: empty ones and those whose first
 * byte is '#' are skipped; the name is the first token (leading blanks skipped, up to the next blank); what follows it is
 * read by rsi_hot_load_depth_text's rules.  Each chromosome X gives exactly what rsi_hot_load_depth_text gives on its slice
 * (its lines without the name), counts and fallback included -- the fallback per chromosome.  Names: looked up in
 * names[] as read_fasta does (names[i] == X or "chr" + X, the first match); names containing "MT" or '.' are skipped
 * silently (the BAM walk's filter); other names not in names[] are handed over with slot = -1 and no depth.  Chromosomes
 * come in order of first appearance; a name that comes back after another one is an error (the lines of a chromosome
 * must be contiguous).  At most max_resident depth buffers exist: the reader needs one free for each new chromosome, so
 * a caller that holds max_resident - 1 of them releases one before asking for the next.  chunk_bytes: bytes of text per
 * transfer (0: 64 MB).  Every wait has the library's 60 s deadline. */
typedef struct rsi_genome_text rsi_genome_text;
typedef struct rsi_genome_chrom {
  int32_t slot;            /* depth buffer, -1: the name is not in names[] (no depth) */
  int32_t pad;
  int64_t n;               /* chromosome length (lengths[i]) */
  const void* d_depth;     /* int32[n] in HBM; valid until rsi_genome_text_release(slot) */
  rsi_text_stats stats;    /* bytes: the chromosome's byte range in the file; lines / stored / beyond / fallback as for its slice */
  char name[256];          /* the name as in the file */
} rsi_genome_chrom;
rsi_genome_text* rsi_genome_text_open(int device, const char* path, int nref, const char* const* names, const int64_t* lengths,
                                      int max_resident, size_t chunk_bytes, int* status);
/* 1: one chromosome complete (*out); 0: end of the file; < 0: error (rsi_genome_text_last_error) */
int rsi_genome_text_next(rsi_genome_text* g, rsi_genome_chrom* out);
void rsi_genome_text_release(rsi_genome_text* g, int slot);   /* its device buffer may be reused */
/* a handed-over chromosome's depth into host memory (tests); returns the element count, < 0 on error */
int64_t rsi_genome_text_copy_depth(rsi_genome_text* g, int slot, int32_t* out, int64_t cap);
/* summed HIP-event time of the boundary and the parse launches so far */
int rsi_genome_text_kernel_ms(const rsi_genome_text* g, double* bound_ms, double* parse_ms);
void rsi_genome_text_close(rsi_genome_text* g);
const char* rsi_genome_text_last_error(const rsi_genome_text* g);
/* the file's format and the inflate figures so far (rsi_inflate_stats) */
int rsi_genome_text_inflate_stats(const rsi_genome_text* g, rsi_inflate_stats* out);
/* Cohort files, "RNAME pos d1 d2 ... dK" (samtools depth -a s1.bam ... sK.bam): the same reader, calling each selected depth
 * column as a sample of its own.  cols: ncols 1-based depth columns, distinct, ncols in [1, 64]; sample j is column cols[j].
 * Sample j of a line is what `iss >> pos >> d1 >> ... >> dc` leaves in dc for c = cols[j]: the clamped bound when dc itself
 * overflows, 0 once an earlier extraction has failed (an overflow included) or the line has fewer columns.  For every sample the depth and the counts are those rsi_genome_text_open gives on the file
 * whose lines carry that column alone; the counts (and the fallback, for all samples together) depend on the positions
 * only, so one rsi_genome_chrom serves every sample, and its d_depth is sample 0.  A depth buffer holds all samples of its
 * chromosome and is allocated at the size of the longest of lengths[]: when fewer than two such buffers fit in the device's
 * free memory the call fails with RSI_ERR_UNSUPPORTED, and with fewer than max_resident it uses as many as fit
 * (rsi_genome_text_max_resident). */
rsi_genome_text* rsi_genome_text_open_samples(int device, const char* path, int nref, const char* const* names,
                                              const int64_t* lengths, const int32_t* cols, int ncols, int max_resident,
                                              size_t chunk_bytes, int* status);
int rsi_genome_text_samples(const rsi_genome_text* g);        /* ncols (1 for rsi_genome_text_open) */
int rsi_genome_text_max_resident(const rsi_genome_text* g);   /* the depth buffers the reader uses */
/* sample j (< ncols) of a handed-over chromosome: int32[n] in HBM, 16-byte aligned; valid until rsi_genome_text_release(slot) */
const void* rsi_genome_text_sample_depth(const rsi_genome_text* g, int slot, int j);
/* sample j of a handed-over chromosome into host memory; returns the element count, < 0 on error */
int64_t rsi_genome_text_copy_sample_depth(rsi_genome_text* g, int slot, int j, int32_t* out, int64_t cap);
/* bedGraph files, "RNAME start end d" (mosdepth per-base.bed.gz, bedtools genomecov -bg / -bga): the same reader and handle.
 * A line stands for the lines "RNAME p d", p = start + 1 .. end (0-based, half-open; start and end read as long long, none
 * when either fails, an overflow included, or end <= start), and every
 * chromosome's depth, counts, hand-over order and errors are those rsi_genome_text_open gives on that expanded file; only
 * stats.bytes is the chromosome's byte range in the bedGraph text.  "track" and "browser" lines are skipped.  Parse time goes
 * to rsi_genome_text_kernel_ms's parse_ms. */
rsi_genome_text* rsi_genome_bedgraph_open(int device, const char* path, int nref, const char* const* names, const int64_t* lengths,
                                          int max_resident, size_t chunk_bytes, int* status);
/* The same for a BGZF file with a tabix index beside it (index_path: a .tbi, as rsi_track_index_write_tbi or tabix write it, or a
 * .csi, as mosdepth writes it): only the members between the smallest chunk begin and the largest chunk end the index holds for
 * names[] (each matched with or without a leading "chr") are read and inflated, the first one's text from the begin's in-member
 * offset on.  Depth, counts, names, hand-over order and errors are those of rsi_genome_bedgraph_open with the same names (the
 * sequences outside names[] that the whole-file reader names and passes over are met only as far as they lie inside the range); only
 * rsi_inflate_stats' blocks, compressed_bytes and text_bytes count the members of that range alone.  An index that does not fit
 * the file is RSI_ERR_BAD_ARG naming it: a begin that is no member header or lies behind a byte other than a line end, a first
 * line of another sequence, a line of names[] directly behind the range's end inside its last member; so is a file that is not
 * BGZF or an index that cannot be parsed.  No name in the index: the reader hands over nothing, as for a file without their lines. */
rsi_genome_text* rsi_genome_bedgraph_open_indexed(int device, const char* path, const char* index_path, int nref, const char* const* names,
                                                  const int64_t* lengths, int max_resident, size_t chunk_bytes, int* status);
/* The compressed byte range [begin, stop) an indexed reader takes from its file (both 0: no name in the index); RSI_ERR_BAD_ARG for
 * a reader opened without an index. */
int rsi_genome_text_index_range(const rsi_genome_text* g, int64_t* begin, int64_t* stop);
/* One chromosome whose depth is already in HBM (e.g. a genome reader's buffer, not modified) and whose fasta[n] is in
 * host memory: the sequence goes to the context's own device buffer, then rsi_hot_run_device. */
int rsi_hot_run_depth_device(rsi_ctx* ctx, const rsi_params* p, const void* d_depth, const uint8_t* fasta, int64_t n,
                             rsi_result** out);

/* ---- BAM pileup -> per-base depth, GPU-assisted -------------------------------------
 * Replaces the read loop of load_data_from_bam (loaddata.cpp:277-333): reads of chromosome `chrom`
 * (all of them, as bam_iter_query(ref, 0, 0x7fffffff) yields) that pass pos != 0, mapq >= minq, not
 * secondary, not duplicate; every base of an M or '=' CIGAR operation with base quality >= min_baseq
 * adds one to the depth at its reference position as resolve_cigar_pos computes it (samfunctions.cpp:
 * 38-100, including that '=' / 'X' do not advance the position).  The host inflates the BGZF blocks
 * (threads) and finds record boundaries; filters, CIGAR and qualities are evaluated on the device, one
 * thread per read, into a difference array that a scan turns into the depth.  A `BAM.bai` next to the
 * file is used to start at the chromosome's first read; without it the file is scanned from the top.
 * Reference defaults: minq 0 (-q), min_baseq 13 (-Q), rsi.cpp:57-58. */
typedef struct rsi_bam_stats {
  int64_t n;                         /* length of the chromosome (header) */
  int64_t bytes_compressed, bytes_inflated, records, on_chrom, used, runs;   /* records walked, reads of `chrom`, reads that passed the filters, runs of counted bases */
  int32_t tid, indexed;              /* reference id of `chrom`; 1 if the .bai was used */
  double t_total_ms, t_inflate_ms, t_walk_ms, t_wait_ms;   /* wall time of the load; of which: inflate (threads), record walk, waiting for the device */
  int64_t malformed;                 /* records whose name / CIGAR / sequence lengths overrun their block_size: skipped, never followed */
} rsi_bam_stats;
/* Depth of `chrom` into the context's device depth buffer (int32[stats->n]); rsi_hot_fetch_i32("depth_in") reads it back. */
int rsi_hot_load_depth_bam(rsi_ctx* ctx, const char* bam_path, const char* chrom, int minq, int min_baseq, rsi_bam_stats* stats);
/* Where rsi_hot_load_depth_bam / rsi_hot_run_bam / _run_bam_dfasta of this context read the file's records from now on
 * (RSI_BAM_READ_HOST when never called; any other mode is RSI_ERR_BAD_ARG).  RSI_BAM_READ_DEVICE: the compressed BGZF members
 * go to the GPU, are inflated there (CRC32 and ISIZE checked), the records of the chromosome are found there and piled up by the
 * same kernel; nothing inflated crosses PCIe and the host touches member headers only (the BAM header's few blocks and the .bai
 * excepted).  The depth and the stats fields n, tid, indexed, records, on_chrom, used, runs and malformed are the host mode's for
 * the same file; bytes_* and t_* describe this mode's own chunks (t_inflate_ms: the inflate kernels, t_walk_ms: the record
 * finder's).  chunk_bytes: inflated bytes per chunk, rounded up to whole members, at least 64 KiB and at most 32 MiB; 0: the
 * default (32 MiB).  Errors of the device mode, the context usable afterwards: a member that fails its CRC32, ISIZE or the decoder
 * (RSI_ERR_BAD_ARG naming the member's file offset and the reason), a file cut inside a member, a block_size below 32 where a
 * record must start ("malformed BAM record"), both RSI_ERR_BAD_ARG; a record longer than 8 MB that spans chunks,
 * RSI_ERR_UNSUPPORTED as in the host mode. */
enum { RSI_BAM_READ_HOST = 0, RSI_BAM_READ_DEVICE = 1 };
int rsi_hot_set_bam_read(rsi_ctx* ctx, int mode, size_t chunk_bytes);
typedef struct rsi_bam_read_stats {
  int32_t mode, pad;                 /* of the context's last BAM load; the rest is 0 after a host-mode load */
  int64_t chunks, members, segments; /* chunks read, BGZF members inflated, 16 384-byte segments searched */
  int64_t guessed, rewalked, passed; /* segments whose guessed record start was the true one / that were walked again from the
                                        true one / that a long record covers */
  double t_upload_ms, t_inflate_ms, t_find_ms;   /* HIP events: compressed bytes and member table to the device, inflate kernels,
                                                    guess + walk + stitch kernels */
} rsi_bam_read_stats;
int rsi_hot_last_bam_read_stats(const rsi_ctx* ctx, rsi_bam_read_stats* out);
/* RP / Q0 annotation of the final calls (cnv_stat, pairrd.cpp:622-748; host only): the insert-size statistics are
 * sampled from the window the reference uses (1 Mb of reads from position 10 Mb of the chromosome on, pairrd.cpp:636),
 * then, per call, the read pairs within max(1000, length) <= 5000 bases are classified.  Needs BAM.bai.  The result's
 * rows (rsi_result_format_row) print the values afterwards; rsi_result_pairs reads them (-1 / -1.0 before annotation,
 * rsi.h:49-50).  On chromosomes shorter than 10 Mb the reference crashes in this step; here the statistics keep their
 * defaults (-1) there. */
int rsi_result_annotate_bam(rsi_result* r, const char* bam_path, const char* chrom);
int rsi_result_pairs(const rsi_result* r, int i, int32_t* rp, double* q0);
/* ---- The same annotation on the device, with no second pass over the BAM ----
 * rsi_hot_set_bam_pairs(ctx, 1) arms the context's BAM loads from now on (off when never called; 0 disarms): beside the pileup,
 * in either read mode, a load then keeps five int32 words per read of the chromosome in HBM -- the pair table, entry k = record
 * k in file order: pos, rend (bam_calend, or pos + 1 without CIGAR), mpos, isize, and info = mapq | flag << 8 | cigar class (0,
 * 1, 2 for two or more operations) << 24 | (mtid != tid && mtid > 0) << 26 | (mtid == tid) << 27 -- 20 bytes per read, held
 * until the context's next BAM load; rsi_hot_fetch_i32 reads the arrays as "pairs_pos", "pairs_rend", "pairs_mpos",
 * "pairs_isize", "pairs_info".  An unarmed load allocates nothing and launches nothing for it.
 * rsi_result_annotate_device fills the result's RP / Q0 from that table exactly as rsi_result_annotate_bam does from the file
 * (same integers, same doubles): it needs an armed load of the result's chromosome still held by ctx, no .bai and no file.
 * It refuses what the host pass cannot make sense of either: a table whose positions are not ascending (RSI_ERR_UNSUPPORTED,
 * "BAM not sorted by position") and one with a record whose name and CIGAR overrun its block_size (RSI_ERR_BAD_ARG, the host
 * reader's message) -- the latter wherever the record lies, where the host fails only if it reads it. */
int rsi_hot_set_bam_pairs(rsi_ctx* ctx, int on);
int rsi_result_annotate_device(rsi_ctx* ctx, rsi_result* r);
typedef struct rsi_pairs_stats {
  int64_t records, table_bytes;     /* entries of the pair table the context holds and their bytes; 0 / 0: no table */
  int64_t maxspan;                  /* the largest rend - pos */
  int64_t sample_count, sample_abs, sample_sq, sample_stop;   /* the insert-size sample: proper pairs, sum |isize|, sum of the
                                       squares wrapped to int32, and S, the index among the sampled reads at which it stopped */
  int32_t isize, isize_sd;          /* bam_pair_sample's results from those sums (-1 / -1 with fewer than three pairs) */
  int64_t calls, examined;          /* calls annotated; table entries their workgroups looked at */
  double t_table_ms, t_sample_ms, t_annotate_ms;   /* HIP events: the load's k_bam_pairs launches, the sample, the annotation */
} rsi_pairs_stats;
/* of the context's last armed load and its last rsi_result_annotate_device (the sample and annotation fields 0 before one) */
int rsi_hot_last_pairs_stats(const rsi_ctx* ctx, rsi_pairs_stats* out);
/* Test hooks: a table from the caller in place of a BAM's (n entries, five arrays as above; the context's own table is dropped).
 * rsi_hot_debug_pair_sample: the insert-size sample over it, out[4] = count, sum |isize|, sum of wrapped squares, S (-1: no
 * read sampled).  rsi_hot_debug_pair_annotate: the counts of ncalls calls (start, end, type as in rsi_call) with the windows
 * rsi_result_annotate_device gives them; the table must be ascending in pos. */
int rsi_hot_debug_pair_sample(rsi_ctx* ctx, int64_t n, const int32_t* pos, const int32_t* rend, const int32_t* mpos, const int32_t* isize,
                              const int32_t* info, int64_t tid_len, int64_t* out);
int rsi_hot_debug_pair_annotate(rsi_ctx* ctx, int64_t n, const int32_t* pos, const int32_t* rend, const int32_t* mpos, const int32_t* isize,
                                const int32_t* info, int ncalls, const int32_t* start, const int32_t* end, const int32_t* type,
                                int isize_mean, int isize_sd, uint32_t* rp_out, uint32_t* q0all_out, uint32_t* q0q0_out);
/* ---- `stat` and `pin`: a list of CNVs that exists already, annotated and sharpened from the BAM ----
 * rsi_hot_stat_calls: RP / Q0 of ncalls calls of the chromosome of the context's last armed load (rsi_hot_set_bam_pairs), with
 * the windows given: start / end / type as in the list (type 2: unknown, RP 0), p1e / p2e the window cnv_stat reads for the
 * call -- the caller carries DIS through its whole list, across chromosomes.  isize_io / isize_sd_io: on entry what the
 * chromosome before left (-1 / -1 at first), on return this chromosome's insert size and deviation, or the values unchanged
 * when it has fewer than three proper pairs in the sample, as cnv_stat's one bamstat_st does.
 * rsi_hot_set_bam_pin(ctx, 1) arms the context's BAM loads (and with them the pair table) to keep, beside each pair-table
 * entry, the read's l_qseq and its CIGAR: 8 bytes per read plus 4 + 4 n_cigar bytes in a pool of words, fetchable as "pin_lq",
 * "pin_coff" (the read's place in the pool: pool[coff] = n_cigar, then the words) and "pin_pool".  Unarmed, nothing is kept.
 * rsi_hot_pin_sample: the depth sample of bam_rd_pr_stats from 10 Mb on -- read length, rd and drd mean and deviation -- kept
 * by the context for rsi_hot_pin_calls.  RSI_ERR_UNSUPPORTED with the reason as the error text where the chromosome cannot be
 * sampled as the reference does: no accepted read from 10 Mb on, or a sampled read more than 1 000 900 bases behind its
 * stretch's start; an unsorted table and an overrun record are refused as rsi_result_annotate_device refuses them.
 * rsi_hot_pin_calls: every call with |end - start| >= 800 and type 0 / 1 gets each breakpoint moved to the best-scoring base of
 * its window of max(m, read length, 50) bases on each side, where at least two clipped reads end; sc1 / sc2: the clip counts
 * (0 for a call not looked at).  RSI_ERR_UNSUPPORTED when that window's counters do not fit the workgroup's LDS. */
typedef struct rsi_pin_stats {
  int64_t records, table_bytes, pool_words;   /* reads kept, bytes of their two arrays plus the pool, words of the pool in use */
  int64_t sample_reads;                       /* reads of the sample's last stretch */
  int32_t pos_start, pos_end;                 /* that stretch: its first read's pos, the pos of the last read counted */
  int32_t l_qseq, r_len;                      /* the sample's read length; the half window rsi_hot_pin_calls last used */
  double rd, rd_sd, drd, drd_sd;
  int64_t breakpoints;                        /* workgroups of the last rsi_hot_pin_calls */
  double t_table_ms, t_sample_ms, t_windows_ms;   /* HIP events: the load's k_bam_pin launches, the sample, the windows */
} rsi_pin_stats;
int rsi_hot_set_bam_pin(rsi_ctx* ctx, int on);
int rsi_hot_stat_calls(rsi_ctx* ctx, int ncalls, const int32_t* start, const int32_t* end, const int32_t* type, const int32_t* p1e, const int32_t* p2e,
                       int32_t* isize_io, int32_t* isize_sd_io, int32_t* rp, double* q0);
int rsi_hot_pin_sample(rsi_ctx* ctx, rsi_pin_stats* out);
int rsi_hot_pin_calls(rsi_ctx* ctx, int m, int ncalls, const int32_t* start, const int32_t* end, const int32_t* type, int32_t* new_start,
                      int32_t* new_end, int32_t* sc1, int32_t* sc2);
int rsi_hot_last_pin_stats(const rsi_ctx* ctx, rsi_pin_stats* out);
/* Test hooks: a pair table plus lq[n], coff[n] and pool[npool] from the caller in place of a BAM's.  _sample: rsi_hot_pin_sample
 * over it, and rd[rd_cap] / drd[rd_cap] (may be null) get the last stretch's arrays from its start on.  _calls:
 * rsi_hot_pin_calls over it with the read length and drd deviation given. */
int rsi_hot_debug_pin_sample(rsi_ctx* ctx, int64_t n, const int32_t* pos, const int32_t* rend, const int32_t* mpos, const int32_t* isize,
                             const int32_t* info, const int32_t* lq, const uint32_t* coff, const uint32_t* pool, int64_t npool, int64_t tid_len,
                             rsi_pin_stats* out, int32_t* rd, int32_t* drd, int64_t rd_cap);
int rsi_hot_debug_pin_calls(rsi_ctx* ctx, int64_t n, const int32_t* pos, const int32_t* rend, const int32_t* mpos, const int32_t* isize,
                            const int32_t* info, const int32_t* lq, const uint32_t* coff, const uint32_t* pool, int64_t npool, int64_t tid_len,
                            int m, int l_qseq, double drd_sd, int ncalls, const int32_t* start, const int32_t* end, const int32_t* type,
                            int32_t* new_start, int32_t* new_end, int32_t* sc1, int32_t* sc2);
/* ---- `geno`: the copy number of a list of regions, from the depth a run leaves in HBM ----
 * After a successful run the context holds the GC-adjusted, capped, N-free depth the calls were made from, the removed regions
 * and the chromosome's median.  rsi_hot_geno_calls reduces ncalls regions of that array, in a number of launches that does not
 * depend on ncalls: start / end are 1-based inclusive reference coordinates as in the output rows (swapped when start > end,
 * clipped to [1, n]); the body is their kept bases, N of them; the flank is the max(N, m) kept bases on each side, clipped to the
 * array, both sides feeding one statistic.  body_q / flank_q: lower quartile, median, upper quartile as the reference's
 * _lowerquartile / _median / _upperquartile give them on ints (partition_stat_tp, wufunctions.cpp:364-424): of n sorted values
 * s[], s[max(n/4,1)-1], s[max(n/2,1)-1], s[max(3n/4,1)-1]; all 0 for an empty range.  RSI_ERR_BAD_ARG when the context's last
 * run failed, there was none, or a debug hook has overwritten its depth since.  ncalls == 0 is RSI_OK and launches nothing. */
/* rsi_geno_record layout: int32 n_body, n_flank, body_min, body_max; int64 body_sum, flank_sum; double body_q[3], flank_q[3], chrom_median */
typedef struct rsi_geno_record {
  int32_t n_body, n_flank, body_min, body_max;
  int64_t body_sum, flank_sum;
  double body_q[3], flank_q[3], chrom_median;
} rsi_geno_record;
typedef struct rsi_geno_stats {
  int64_t launches, jobs, tiles, passes;   /* kernel launches of the last call; its jobs (two per line) and tiles; histogram passes (1 for bytes) */
  int64_t bytes;                           /* device memory the context holds for this step (0 until the first call with lines) */
  double ms;                               /* wall time of the last call's device part, tables up and records back included */
} rsi_geno_stats;
int rsi_hot_geno_calls(rsi_ctx* ctx, int m, int ncalls, const int32_t* start, const int32_t* end, rsi_geno_record* out);
int rsi_hot_last_geno_stats(const rsi_ctx* ctx, rsi_geno_stats* out);
/* Test hook: the same kernels through the same function over the HOST array depth[n], which becomes the context's compacted depth
 * as bytes (storage 1; a value outside 0 .. 255 is RSI_ERR_BAD_ARG) or as int32 (storage 4), with explicit half-open compacted
 * ranges per job: the body [lo, hi), the flank's pieces [flo0, fhi0) and [flo1, fhi1); any may be empty, a range outside [0, n]
 * or with hi < lo is RSI_ERR_BAD_ARG.  tile: values per tile (0: the default, 16384).  chrom_median comes back 0. */
int rsi_hot_debug_geno(rsi_ctx* ctx, const int32_t* depth, int64_t n, int storage, const int32_t* lo, const int32_t* hi, const int32_t* flo0,
                       const int32_t* fhi0, const int32_t* flo1, const int32_t* fhi1, int njobs, int tile, rsi_geno_record* out);
/* Fixed-layout summary of a chromosome's result for the one exchange of a multi-GPU run (the gather of per-chromosome
 * results that replaces the reference's sequential output loop, rsi.cpp:1594-1608):
 *   out[0..7]  = chromosome id (the caller's), chromosome median, SD, number of final calls, number stored here, 0, 0, 0
 *   then RSI_SUMMARY_CALL doubles per stored call: start, end, type, qscore, cnvmed, cnviqr, refmed, refiqr,
 * at most max_calls of them (stored < number of calls means the block was too small: callers treat that as an error).
 * Returns the number of doubles written.  rsi_summary_format_row: the output row of stored call i of such a block. */
#define RSI_SUMMARY_HEAD 8
#define RSI_SUMMARY_CALL 8
int rsi_result_summary(const rsi_result* r, int chrom_id, double* out, int max_calls);
int rsi_summary_format_row(const double* block, int i, const char* chrom, char* buf, int cap);
/* every stored call of the block, one row per line (each ended by '\n'); returns the bytes written, < 0 if buf is too small */
int rsi_summary_format_rows(const double* block, const char* chrom, char* buf, int cap);
/* The diagnostic lines of the chromosome's (last) scan as the reference writes them to its log, in its order: the NB
 * transform's "RD median : " / "RD median absolute deviation : " (rsi.cpp:1140-1141), the first pass' per-L lines
 * (rsi.cpp:1221-1224 "DEL-", 1251-1254 "DUP+": L, bins marked so far, bins, portion), filterstatus' level table (level, bins,
 * float mean; then the two chosen levels; rsi.cpp:991-1002), the second pass' per-L lines.  This is the log sink of SURVEY
 * 8(b) as a pull interface: line i (0-based) into buf; returns i + 1, or 0 when there is no such line. */
int rsi_result_log_line(const rsi_result* r, int i, char* buf, int cap);
/* Reference sequences of the BAM header: names as one '\n'-separated string into names[names_cap], lengths into
 * lengths[max_refs]; returns their number (also when the buffers are too small or NULL), < 0 on error. */
int rsi_bam_references(const char* bam_path, char* names, int names_cap, int64_t* lengths, int max_refs);
/* rsi_hot_load_depth_bam + rsi_hot_run on the loaded depth; fasta[n] in host memory, n must equal the header's length. */
int rsi_hot_run_bam(rsi_ctx* ctx, const rsi_params* p, const char* bam_path, const char* chrom, int minq, int min_baseq,
                    const uint8_t* fasta, int64_t n, rsi_result** out, rsi_bam_stats* stats);
/* Same, inputs already resident in device memory (HBM); they are not modified. */
int rsi_hot_run_device(rsi_ctx* ctx, const rsi_params* p, const void* d_depth, const void* d_fasta, int64_t n,
                       rsi_result** out);

/* ---- The reference sequence read on the device ------------------------------------------------------------------
 * An rsi_ref is an indexed FASTA file (FILE with FILE.fai; samtools faidx), plain text or BGZF (bgzip; then with FILE.gzi, or
 * without: the members are walked once).  A load reads the bytes of one sequence's lines -- for BGZF the compressed bytes of the
 * members that hold them, inflated on the device with their CRC32 and ISIZE checked -- and a kernel unfolds them by the .fai's
 * arithmetic (base k lies at OFFSET + k / LINEBASES * LINEWIDTH + k % LINEBASES) into one byte per base, unchanged: no case
 * folding, no classification.  While unfolding, every line terminator position must hold '\n' or '\r' and no base position
 * '\n', '\r' or '>': otherwise the .fai does not fit the file and the load fails with RSI_ERR_BAD_ARG naming the sequence.
 * The format comes from the file's first bytes as for depth files; plain gzip is RSI_ERR_UNSUPPORTED (recompress with bgzip).
 * rsi_ref_open parses only and makes no GPU call.  fai_path / gzi_path NULL: fasta_path + ".fai" / ".gzi"; gzi_path "none" (or a
 * default .gzi that is not there): the member table is built at the first load from the members' BSIZE and ISIZE fields.  A
 * .gzi that does not fit the file -- an offset that is no member header, text offsets that disagree with the members' ISIZE,
 * offsets that do not increase -- is RSI_ERR_BAD_ARG.  One handle serves one device (the first it loads on) and one load at a time. */
typedef struct rsi_ref rsi_ref;
typedef struct rsi_ref_seq {
  int64_t length, offset;         /* the .fai's LENGTH and OFFSET */
  int32_t linebases, linewidth;   /* LINEBASES, LINEWIDTH */
  char name[256];
} rsi_ref_seq;
typedef struct rsi_ref_stats {
  int64_t bytes_read;     /* bytes of the file read (BGZF: compressed bytes) */
  int64_t text_bytes;     /* bytes of text unfolded from */
  int64_t members;        /* BGZF members inflated */
  int32_t format;         /* 0 text, 1 BGZF */
  int32_t index_used;     /* BGZF: 1 the .gzi, 0 members walked */
  double t_kernel_ms;     /* summed HIP-event time of the inflate and unfold launches */
  double t_wall_ms;       /* wall time of the load */
} rsi_ref_stats;
int rsi_ref_open(const char* fasta_path, const char* fai_path, const char* gzi_path, rsi_ref** out);
void rsi_ref_close(rsi_ref* ref);
const char* rsi_ref_last_error(const rsi_ref* ref);   /* ref may be NULL: why the last rsi_ref_open failed */
int rsi_ref_count(const rsi_ref* ref);
int rsi_ref_sequence(const rsi_ref* ref, int i, rsi_ref_seq* out);
/* read_fasta's rule: the first sequence named rname or "chr" + rname; -1: none */
int rsi_ref_find(const rsi_ref* ref, const char* rname);
int rsi_ref_format(const rsi_ref* ref);               /* 0 text, 1 BGZF */
/* The path of the .gzi in use, "" when the members are (to be) walked */
const char* rsi_ref_index_path(const rsi_ref* ref);
/* Sequence i unfolded into d_out[0, length) in HBM of `device`: d_out 16-byte aligned, cap >= length + 64 (what the run entry
 * points want of d_fasta).  stream: a hipStream_t of that device, NULL for the handle's own; the call returns when the bytes are there.  st may be NULL. */
int rsi_ref_load_device(rsi_ref* ref, int device, int i, void* d_out, int64_t cap, void* stream, rsi_ref_stats* st);
/* The same into a device buffer of the handle's own, then copied to out[0, length); cap >= length. */
int rsi_ref_load_host(rsi_ref* ref, int device, int i, uint8_t* out, int64_t cap);
/* rsi_hot_run_text / rsi_hot_run_bam with the sequence already in HBM (d_fasta[n], 16-byte aligned, not modified): no copy of it. */
int rsi_hot_run_text_dfasta(rsi_ctx* ctx, const rsi_params* p, const char* depth_path, const void* d_fasta, int64_t n,
                            rsi_result** out, rsi_text_stats* stats);
int rsi_hot_run_bam_dfasta(rsi_ctx* ctx, const rsi_params* p, const char* bam_path, const char* chrom, int minq, int min_baseq,
                           const void* d_fasta, int64_t n, rsi_result** out, rsi_bam_stats* stats);
/* `bytes` of device memory on `device` (hipMalloc: 256-byte aligned), for callers without a HIP runtime of their own: the command
 * line's sequence buffers.  NULL when there is none. */
void* rsi_ref_device_alloc(int device, int64_t bytes);
void rsi_ref_device_free(int device, void* p);
/* Test hooks for the reader's host decisions (ref_host.h), no file and no device.
 * _fai_line: one .fai line parsed (0, or RSI_ERR_BAD_ARG with the reason in rsi_ref_last_error(NULL)).
 * _ranges: for the layout `s` (name unused), out[0] = flen (read_fasta's byte count); out[1], out[2] = the text [a, b) the bases
 *   [k0, k1) need; out[3], out[4] = the bases [k0', k1') the text span [a_in, b_in) holds whole (at_eof: b_in is the file's end).
 * _gzi: a .gzi image parsed; the table (the first member's (0, 0) in front) as pairs into table[2 * cap]; returns the number of
 *   members (also when cap is too small), RSI_ERR_BAD_ARG when it cannot be parsed.
 * _cover: the members [out[0], out[1]) of such a table (n pairs) that cover the text [a, b), out[2] = a - their first text offset. */
int rsi_ref_debug_fai_line(const char* line, rsi_ref_seq* out);
/* Test hook: the sizes a load works in -- a text file's bases per transfer and unfold launch (any number from 1 on, also no
 * multiple of 16) and a BGZF file's text per inflate launch (from 1024 on; a launch takes one member at least) -- so that
 * sequences of a few kilobases take the many-chunk paths of a chromosome.  0: the default (32 Mi each). */
int rsi_ref_debug_set_chunks(rsi_ref* ref, int64_t text_chunk_bases, int64_t bgzf_span_bytes);
int rsi_ref_debug_ranges(const rsi_ref_seq* s, int64_t k0, int64_t k1, int64_t a_in, int64_t b_in, int at_eof, int64_t* out);
int64_t rsi_ref_debug_gzi(const uint8_t* image, int64_t len, int64_t* table, int64_t cap);
int rsi_ref_debug_cover(const int64_t* table, int64_t n, int64_t a, int64_t b, int64_t* out);

/* ---- Excluded regions: a mask applied on the device ---------------------------------------------------------------------
 * An excluded base behaves exactly like an N of the reference sequence: it is not GC, its run is padded by max(50, m/4) and
 * merged with its neighbours (get_noseq_regions, loaddata.cpp:243-273), removed before binning and re-inserted when the calls
 * are mapped back -- a run with mask M on sequence F gives what a run without a mask gives on F with M's bases replaced by
 * 'N'.  The sequence itself is not touched (it is const host memory, or the caller's HBM): a kernel behind the classification
 * edits the two bit planes everything else reads.  The mask's runs count like the sequence's own: more than 128 padded regions
 * take the general compaction kernel, more than 512 runs leave region building to the host, more than 4096 padded regions
 * are RSI_ERR_UNSUPPORTED.
 * rsi_hot_set_exclude: `count` intervals, 0-based half-open [start[i], end[i]), in any order, overlapping or not; end <= start is
 * ignored, a negative start counts as 0; the library sorts and merges them and clips them to the run's n.  The mask arms the
 * NEXT run on this context only -- rsi_hot_run, _run_text, _run_bam, _run_device or _run_depth_device -- which consumes it whether
 * it succeeds or fails (a context serves one chromosome after another: a mask that stayed would land on the wrong one).
 * count == 0 disarms (the arrays may then be NULL); count < 0, or count > 0 with a NULL array, is RSI_ERR_BAD_ARG.  The pool's
 * entry points (rsi_pool_run / _run_host / _submit) take no mask; arming a pool worker's context while pool runs are queued is
 * the caller's error. */
int rsi_hot_set_exclude(rsi_ctx* ctx, const int64_t* start, const int64_t* end, int count);
/* The intervals a BED file holds for `chrom` (length n), normalised: sorted, merged (touching ones too), end clipped to n.  Host
 * only.  Returns their number -- also when cap is too small or the arrays are NULL, as rsi_bam_references does -- and writes the
 * first min(number, cap).  Fields are separated by tabs or blanks, the first three count; empty lines, '#' lines and "track" /
 * "browser" lines are skipped; the file is read through zlib (plain text or gzip).  A name matches `chrom` when they are equal or
 * differ by a leading "chr" in either direction.  Every other line must be well formed whichever sequence it names: fewer than
 * three fields, a coordinate that is not a non-negative integer, or end <= start is RSI_ERR_BAD_ARG, with the line number in
 * rsi_hot_last_error(NULL). */
int rsi_exclude_read_bed(const char* path, const char* chrom, int64_t n, int64_t* start, int64_t* end, int cap);

/* ---- Depth tracks: bedGraph written from the device --------------------------------------------------------------------------
 * An int32[n] array in HBM as the text of `bedtools genomecov -bga`: one line "NAME<TAB>start<TAB>end<TAB>value" per maximal run of
 * equal values, start 0-based, end exclusive, zeros included, value as %d (negative values too), coordinates as %lld.  Runs are
 * found, measured and formatted by kernels; only finished text crosses PCIe, slice by slice through two pinned buffers, so
 * that the workspace does not grow with n.  A bedGraph reader (rsi_genome_bedgraph_open, -d track.bedgraph) takes
 * the file back.  An empty name, one longer than 255 bytes or one with a tab or a newline is RSI_ERR_BAD_ARG; n == 0 writes
 * nothing and is RSI_OK; a write() that fails is RSI_ERR_INTERNAL with errno's text in rsi_hot_last_error.  Every wait has the
 * library's 60 s deadline. */
typedef struct rsi_track_stats { int64_t n, lines, bytes, slices; double t_total_ms, t_kernel_ms, t_write_ms; } rsi_track_stats;
/* The last run's depth of this context as bedGraph, appended to (append != 0) or replacing `path`.
 * which: 0 = the raw input depth of the run, 1 = the GC-adjusted depth ("rd_gc", before the cap; RSI_ERR_BAD_ARG after a -NOGC run).
 * The raw depth is what the run read: the context's own buffer after rsi_hot_run / _run_text / _run_bam, the CALLER's buffer
 * after rsi_hot_run_device / _run_depth_device -- borrowed, so both forms are valid only while the caller still holds that
 * buffer unchanged (a genome reader's slot: before rsi_genome_text_release; the context's own buffer: before the next
 * rsi_hot_load_depth_*).  RSI_ERR_BAD_ARG when the context has run nothing, or rsi_hot_debug_track has taken its buffer since. */
int rsi_hot_write_track(rsi_ctx* ctx, int which, const char* chrom, const char* path, int append, rsi_track_stats* stats);
/* Any int32[n] in HBM (not modified), e.g. a genome reader's buffer. */
int rsi_hot_write_track_device(rsi_ctx* ctx, const void* d_values, int64_t n, const char* chrom, const char* path, int append,
                               rsi_track_stats* stats);
/* Test hook: host values[n] uploaded (into the context's input depth buffer), formatted with coordinates offset by pos0, text
 * into out[cap]; slice_bases > 0 forces that slice length (0: the default).  Returns the text length (also when out == NULL or
 * cap is too small, writing nothing then), < 0 on error. */
int64_t rsi_hot_debug_track(rsi_ctx* ctx, const int32_t* values, int64_t n, const char* chrom, int64_t pos0, int64_t slice_bases,
                            char* out, int64_t cap, rsi_track_stats* stats);

/* ---- Per-bin tracks: the signal the caller worked on, one value per bin ----------------------------------------
 * After a run the context holds nb bins of m compacted bases, their exact medians, the removed regions and the chromosome's
 * median.  Bin b covers the compacted positions [b m, (b + 1) m), mapped back to the reference through the removed regions; it
 * is written as one line "NAME<TAB>start<TAB>end<TAB>value" (0-based half-open, %lld) per maximal stretch of consecutive reference
 * positions: cut where a removed region lies strictly inside it, never covering a removed base.  Lines come in increasing
 * order and do not overlap; equal neighbours are not merged; the ncompact mod m bases behind the last bin get no line.
 * which: 0 = the bin's median as %d; 1 = the median over the chromosome's median with three decimals, rounded half up in
 * integers: q = (4000 v + M2) / (2 M2) with M2 = twice the chromosome's median, written as q / 1000 "." q % 1000.
 * stats.n is the number of bins.  RSI_ERR_BAD_ARG: a context that has run nothing or whose last run failed (or whose bins a
 * test hook has overwritten since), a bad name (as above), which outside 0 and 1, a chromosome median of 0 with which = 1. */
int rsi_hot_write_bin_track(rsi_ctx* ctx, int which, const char* chrom, const char* path, int append, rsi_track_stats* stats);
/* Test hook: host values[nb] and regions (npairs inclusive pairs, sorted, apart by at least one kept base) of a chromosome of n
 * bases, bins of m compacted bases, median2 = twice the chromosome's median; slice_bins > 0 forces that slice length.  The
 * values go into the context's bin-median buffer.  RSI_ERR_BAD_ARG also for regions that are unsorted, touching or outside
 * [0, n), and for nb m above the kept bases.  Returns the text length as rsi_hot_debug_track does. */
int64_t rsi_hot_debug_bin_track(rsi_ctx* ctx, const int32_t* values, int64_t nb, int m, int64_t n, const int32_t* pairs, int npairs,
                                int64_t median2, int which, const char* chrom, int64_t slice_bins, char* out, int64_t cap,
                                rsi_track_stats* stats);

/* ---- BGZF tracks: the writers' text deflated on the device ------------------------------------------------------
 * With the format set to RSI_TRACK_BGZF, rsi_hot_write_track, _write_track_device, rsi_hot_write_bin_track and the two test hooks
 * (rsi_hot_debug_track, rsi_hot_debug_bin_track: their out[] then holds the BGZF bytes, their return value is that length) write
 * what `bgzip` makes of the text: a sequence of BGZF members, each holding at most 65280 bytes of text (members are cut per
 * slice, so a slice's last member may be short), deflated with dynamic Huffman codes or, where that would not be shorter,
 * stored.  The bytes depend on the text alone.  Only the compressed bytes cross PCIe.  rsi_track_stats goes on counting text
 * (bytes, lines); the compressed side is in rsi_deflate_stats.  The writers write members only: a file is complete once
 * rsi_bgzf_write_eof has appended the end-of-file block -- once, after the last chromosome appended to it.  Every reader of
 * this library (-d FILE.bedgraph.gz, rsi_genome_bedgraph_open) takes the file back, inflating it on the device. */
enum { RSI_TRACK_TEXT = 0, RSI_TRACK_BGZF = 1 };
/* The format of this context's track calls from now on (RSI_TRACK_TEXT when never called); any other value is RSI_ERR_BAD_ARG. */
int rsi_hot_set_track_format(rsi_ctx* ctx, int format);
typedef struct rsi_deflate_stats {
  int64_t members;          /* BGZF members written */
  int64_t stored_members;   /* those that are one stored block (text that does not compress) */
  int64_t text_bytes;       /* bytes of text they hold */
  int64_t file_bytes;       /* their bytes in the file (no end-of-file block) */
  double t_kernel_ms;       /* summed HIP-event time of the deflate and pack launches */
} rsi_deflate_stats;
/* The figures of the context's last track call or rsi_hot_debug_deflate (all zero after a plain-text one). */
int rsi_hot_last_deflate_stats(const rsi_ctx* ctx, rsi_deflate_stats* out);
/* Appends the 28-byte BGZF end-of-file block to `path` (created when missing).  RSI_ERR_INTERNAL when that fails. */
int rsi_bgzf_write_eof(const char* path);
/* Test hook for the two kernels alone: text[len] (any bytes) uploaded, cut into members of 65280 bytes, deflated and packed;
 * the BGZF bytes (no end-of-file block) into out[cap].  Returns their length (also when out == NULL or cap is too small,
 * writing nothing then; 0 for len == 0), < 0 on error. */
int64_t rsi_hot_debug_deflate(rsi_ctx* ctx, const uint8_t* text, int64_t len, uint8_t* out, int64_t cap, rsi_deflate_stats* stats);

/* ---- The tabix index of a BGZF track, built from the device -----------------------------------------------------
 * An rsi_track_index collects, chromosome by chromosome in the order of the calls, what a .tbi file holds: per bin (tabix's
 * reg2bin over 0-based half-open lines) the chunks of the file with that bin's lines, as BGZF virtual offsets (compressed offset
 * of a member << 16 | offset in its text), and per 16 384-base window the offset of the first line that reaches into it.  While
 * one is set on a context, every BGZF rsi_hot_write_track, rsi_hot_write_track_device and rsi_hot_write_bin_track (and the two
 * test hooks, whose file starts at offset 0) adds its chromosome: each slice's records come from one more launch behind its
 * deflate and pack launches and cross PCIe with the slice, at no wait of their own.  Offsets are absolute in the file the call
 * wrote: with `append`, the file's size before the call is added.  A call of the name the index ends with goes on with that
 * chromosome.  A line that ends beyond 2^29 is RSI_ERR_UNSUPPORTED (the format's limit; checked before anything is written), a
 * text-format call with an index set RSI_ERR_BAD_ARG.  A chromosome that wrote no line is not listed.  A track call that fails
 * after its first slice leaves the slices it had written in the index: the index is then of no use (a retry of the same name would
 * go on with the partial chromosome); free it and begin a new one, as the command line does. */
typedef struct rsi_track_index rsi_track_index;
rsi_track_index* rsi_track_index_create(void);
void rsi_track_index_free(rsi_track_index* ix);
/* ix == NULL turns indexing off (the default).  The index must outlive its use by the context; the context does not own it. */
int rsi_hot_set_track_index(rsi_ctx* ctx, rsi_track_index* ix);
/* src's chromosomes behind dst's, their compressed offsets moved by `shift` bytes (a part file appended at that offset).  A first
 * chromosome of src with the name dst ends with goes on with that chromosome (two parts of one chromosome), as a later call would. */
int rsi_track_index_append(rsi_track_index* dst, const rsi_track_index* src, int64_t shift);
/* PATH as a .tbi: the index for a BED-like file (columns 1, 2, 3; 0-based; '#' comments), BGZF-compressed on the host, without
 * the optional pseudo-bin and unplaced count.  RSI_ERR_INTERNAL when the file cannot be written. */
int rsi_track_index_write_tbi(rsi_track_index* ix, const char* path);
/* What it holds: chromosomes, chunks and linear-index windows (any pointer may be NULL). */
int rsi_track_index_counts(const rsi_track_index* ix, int64_t* nref, int64_t* nchunks, int64_t* nwindows);
/* Test hook: the .tbi stream before compression into out[cap]; returns its length (also when it does not fit: nothing written). */
int64_t rsi_track_index_debug_tbi(const rsi_track_index* ix, uint8_t* out, int64_t cap);

/* ---- `depth`: what a chromosome's per-base depth says about itself, without a run ----
 * Every function below takes d_depth, an int32[n] in HBM that is not modified: the context's own input buffer
 * (rsi_hot_loaded_depth) or any other, a genome reader's slot for one, as rsi_hot_write_track_device does.  n == 0 and zero
 * regions are RSI_OK and launch nothing.  Every wait has the library's 60 s deadline.
 * rsi_hot_loaded_depth: the array the context's last successful rsi_hot_load_depth_text / _load_depth_bam left in its input buffer
 * (valid until the next load, run from host arrays or debug hook of the context); RSI_ERR_BAD_ARG when the buffer holds nothing. */
int rsi_hot_loaded_depth(rsi_ctx* ctx, const void** d_depth, int64_t* n);
/* rsi_depth_summary layout: int64 n, sum, over, negative; int32 min, max */
typedef struct rsi_depth_summary {
  int64_t n, sum;      /* bases, and the exact sum of their depth */
  int64_t over;        /* bases deeper than 65535 (counted in dist[65535]) */
  int64_t negative;    /* negative depths met: the call then fails and nothing else of the record counts */
  int32_t min, max;    /* the real ones, whatever the distribution's cap (0, 0 for n == 0) */
} rsi_depth_summary;
/* One pass over the array: the record, and dist[d] = bases of depth d for d < min(dist_cap, 65536), depths above 65535 counted at
 * 65535 (dist may be NULL).  Integer atomics only: the same array gives the same numbers on every call.  A negative depth indexes
 * nothing: it is counted in out->negative and the call returns RSI_ERR_BAD_ARG ("negative depth"). */
int rsi_hot_depth_summary(rsi_ctx* ctx, const void* d_depth, int64_t n, rsi_depth_summary* out, int64_t* dist, int dist_cap);
/* rsi_depth_region layout: int64 n, sum; int32 min, max */
typedef struct rsi_depth_region { int64_t n, sum; int32_t min, max; } rsi_depth_region;
/* nreg regions [start, end), 0-based half-open, in any order, overlapping or equal ones too, each clipped to [0, n): the bases
 * left, their exact sum, minimum and maximum (all 0 for a region with nothing left, end < start included).  Reduced through geno's
 * tile table and min / max kernels, in a number of launches that does not depend on nreg. */
int rsi_hot_depth_regions(rsi_ctx* ctx, const void* d_depth, int64_t n, int nreg, const int64_t* start, const int64_t* end, rsi_depth_region* out);
/* The mean depth of every window [k W, min((k + 1) W, n)) (the last one short; W >= 1) as lines "chrom<TAB>start<TAB>end<TAB>mean",
 * appended to (append != 0) or replacing `path`: summed slice by slice into a workspace that does not grow with n, formatted on
 * the device and sent through the track writer's slices, as text or as BGZF members (rsi_hot_set_track_format; a BGZF file is
 * complete once rsi_bgzf_write_eof has ended it).  The mean has two decimals and is rounded half up in integers: with a = S / L
 * and r = S mod L the hundredths are (200 r + L) / (2 L), a hundred of them carrying into a.  The depth must not be negative
 * (rsi_hot_depth_summary says whether it is): a sum that is not positive is written as 0.00.  An index set with
 * rsi_hot_set_track_index is left alone: these lines are not indexed.  stats->n counts the lines. */
int rsi_hot_write_window_track(rsi_ctx* ctx, const void* d_depth, int64_t n, const char* chrom, int64_t W, const char* path, int append,
                               rsi_track_stats* stats);
/* The same for nreg explicit regions, in the order given: a region is clipped to [0, n) and written with its clipped
 * coordinates; one with nothing left is written with the coordinates given and 0.00.  The sums are rsi_hot_depth_regions'. */
int rsi_hot_write_region_track(rsi_ctx* ctx, const void* d_depth, int64_t n, const char* chrom, int nreg, const int64_t* start,
                               const int64_t* end, const char* path, int append, rsi_track_stats* stats);
typedef struct rsi_depth_stats {
  int64_t launches;     /* kernel launches of the last rsi_hot_depth_summary / _depth_regions (or their hooks) */
  int64_t workgroups;   /* of its summary pass, or tiles of its regions */
  int64_t bytes;        /* device memory the context holds for these two */
  double ms;            /* wall time of the call's device part, results back included */
  double kernel_ms;     /* HIP-event time of the summary pass alone (0 for regions) */
} rsi_depth_stats;
int rsi_hot_last_depth_stats(const rsi_ctx* ctx, rsi_depth_stats* out);
/* Test hooks: host values[n] uploaded into the context's input depth buffer (what rsi_hot_loaded_depth then returns), then the
 * same functions.  span / tile: values per workgroup of the summary pass, values per tile of the regions (0: the defaults, 131072
 * and 16384). */
int rsi_hot_debug_depth_summary(rsi_ctx* ctx, const int32_t* values, int64_t n, int64_t span, rsi_depth_summary* out, int64_t* dist, int dist_cap);
int rsi_hot_debug_depth_regions(rsi_ctx* ctx, const int32_t* values, int64_t n, int tile, int nreg, const int64_t* start, const int64_t* end,
                                rsi_depth_region* out);
/* ... and of the two track writers: W > 0 writes the windows, W == 0 the nreg regions.  span: bases per workgroup of the window
 * sums (0: the default, 4096, which is also the most); slice_lines > 0 forces that slice length in lines; tile as above; pos0 is
 * added to every coordinate written (the means are not touched).  The text (or, with the format BGZF, its members) into out[cap];
 * returns its length as rsi_hot_debug_track does.  stats->slices counts the slices; stats->lines the lines. */
int64_t rsi_hot_debug_region_track(rsi_ctx* ctx, const int32_t* values, int64_t n, const char* chrom, int64_t W, int nreg, const int64_t* start,
                                   const int64_t* end, int span, int tile, int64_t slice_lines, int64_t pos0, char* out, int64_t cap,
                                   rsi_track_stats* stats);

/* Results.  which: 0 = calls after sd_filters (what write_cnv_to_file prints),
 *                  1 = detectcnv output before sd_filters,
 *                  2 = bin-space segments after the scan (rsicnvnbn / rsicnvmed output),
 *                  3 = bin-space segments after areblockscnv + sort. */
int rsi_result_ncalls(const rsi_result* r, int which);
const rsi_call* rsi_result_calls(const rsi_result* r, int which);
const rsi_chrom_stats* rsi_result_stats(const rsi_result* r);
/* Padded N regions as (start,end) inclusive pairs; returns the number of regions. */
int rsi_result_noncode(const rsi_result* r, int32_t* pairs, int cap);
/* One output row exactly as cnv_format1 prints it (rsi.cpp:581-631), without the newline. */
int rsi_result_format_row(const rsi_result* r, int i, const char* chrom, char* buf, int cap);
void rsi_result_free(rsi_result* r);

/* Intermediates for the parity tests (copied device -> host on demand while the context still
 * holds the chromosome: valid until the next rsi_hot_run* on the same context).
 * int32 names: "rd_gc" (after GC adjust, n), "rd_concat" (capped + compacted, n_compact),
 *              "binmedint", "status1", "status1f", "status2" (nbins each)
 * f32   names: "binnb", "binmed" (nbins)
 * i64   names: "binsum" (nbins)
 * Returns the element count (also when out == NULL), or a negative rsi_status. */
int64_t rsi_hot_fetch_i32(rsi_ctx* ctx, const char* name, int32_t* out, int64_t cap);
int64_t rsi_hot_fetch_f32(rsi_ctx* ctx, const char* name, float* out, int64_t cap);
int64_t rsi_hot_fetch_i64(rsi_ctx* ctx, const char* name, int64_t* out, int64_t cap);

/* Test hook: filterstatus' per-level sums (rsi.cpp:967-976: float accumulation in index order per status level) of HOST arrays
 * T[nb], status[nb] (values in [-Lmax, Lmax]) through the device's exact parallel form; sums / counts: 2 Lmax + 1 entries, index
 * = level + Lmax.  counts[Lmax] == -1: the device declined the input (the pipeline then runs the sequential loop itself).  A status
 * value outside [-Lmax, Lmax]: RSI_ERR_BAD_ARG, checked on the host before anything is launched. */
int rsi_hot_debug_level_sums(rsi_ctx* ctx, const float* T, const int32_t* status, int64_t nb, int Lmax, float* sums, int32_t* counts);
/* Test hook: one scan pass (rsistatus) over host arrays with the caller's thresholds; status[nb] out, info[4] = tiles the
 * detection pass listed, trimming walks that left the array, inexact-threshold flags, 0. */
int rsi_hot_debug_scan(rsi_ctx* ctx, const float* T, const int32_t* medint, int64_t nb, double RDmedian, double tmedian, double tlamda,
                       int Lmax, int32_t* status, int32_t* info);
/* Test hook: get_rsi_segments (rsi.cpp:1060-1117) over HOST arrays: T[nb], status[nb] and the marked runs as nruns (start, end)
 * pairs -- sorted, disjoint, inside [0, nb); anything else is RSI_ERR_BAD_ARG -- through the function the scan calls behind its
 * second pass: the runs' prefixes, the best (L, offset) per work item, the fold over the items, the type by the median of the
 * status values covered.  pairs_per_item: (L, offset) pairs a work item takes; 0 = what a run chooses for this context.  A segment
 * whose |score| is below tlamda / 2 is dropped as the scan drops it: with tlamda = 0 every run gives one segment.  seg_*: room for
 * nruns entries.  info[8] = runs, work items, 1 / 0 for lists in the kernel arguments / behind pointers, 1 / 0 for the runs' status
 * values through the mailbox / a copy of the array, runs longer than the LDS staging holds, segments kept, pairs per item, 0.
 * Overwrites the bin arrays the rsi_hot_fetch_* calls read. */
int rsi_hot_debug_segments(rsi_ctx* ctx, const float* T, const int32_t* status, int64_t nb, const int32_t* runs, int nruns, double tmedian,
                           double tlamda, int64_t pairs_per_item, int32_t* seg_start, int32_t* seg_end, int32_t* seg_type, double* seg_score,
                           int32_t* info);
/* Test hook: optimize_with_derivative (rsi.cpp:889-944), called twice (rsi.cpp:1876-1877), for njobs candidates (start, end, type;
 * updated in place) over the HOST array depth[n], which becomes the context's compacted depth as bytes (storage 1; a value outside
 * 0 .. 255 is RSI_ERR_BAD_ARG) or as int32 (storage 4).  The candidate stages' own function with the context's own workspace, grown as
 * a run grows it.  info[4] (may be NULL) = jobs the workspace was laid out for before, and after, 1 / 0 for the job list in the mailbox /
 * copied, waits. */
int rsi_hot_debug_sharpen(rsi_ctx* ctx, const int32_t* depth, int64_t n, int storage, int32_t* start, int32_t* end, const int32_t* type,
                          int njobs, int32_t* info);
/* One record of rsi_hot_debug_candidate_tests: the plan the host made from the list, the record the device wrote for it (flags -1:
 * the plan was never sent), which road judged the candidate (0: the device's statistics, 1: the host walk because the device
 * declined), and the candidate as judged. */
typedef struct rsi_cand_record {
  int32_t capacity, top, margin, cut, nleft, nright;                                 /* plan_test */
  int32_t road;
  int32_t flags, nref, nbody, nwin, left_reach, right_reach, body_min, body_max;     /* the device's record */
  int32_t type, status, geno;                                                        /* the candidate as judged */
  double body_q[3], body_s1, body_s2, ref_q[3], ref_s1, ref_s2;                      /* the device's record */
  double p1, cnvmed, cnvsd, cnviqr, refmed, refsd, refiqr;                           /* the candidate as judged */
} rsi_cand_record;
/* Test hook: the neighbourhood test of a candidate (isitcnvwrap + isitcnv, rsi.cpp:101-287) over the HOST array depth[n], which
 * becomes the context's compacted depth as bytes (storage 1; a value outside 0 .. 255 is RSI_ERR_BAD_ARG) or as int32 (storage 4).
 * span_all: the compacted length the stage compares n with (n == span_all: the per-base form, n < span_all / 2: the form of the
 * block tests on bin medians).  The list is ncand candidates (start, end, type, status); for every one of the nindex indices the
 * road of a run is taken against the list as handed in: the plan, ONE call of the device tester over all plans, the judgement --
 * by the host walk where the device declined.  form: bit 0 = the split form (three launches) / the one-workgroup form, bit 1 =
 * gathered values of byte depth kept as int32.  The environment switches of whole runs are not read.  out[nindex].
 * RSI_ERR_BAD_ARG, with the context left usable: a candidate outside 0 <= start <= end < n, a type other than 0 (DEL) / 1 (DUP)
 * (the reference exits), an index outside the list, m < 1, maxchkbp < 1, minmlen or chklen not positive, a negative buffer, a
 * negative depth, a plan without capacity.  info[8] (may be NULL) = waits, job lists that rode in the mailbox, job lists that were copied, the capacity in bytes
 * of the per-job records before and after, of the folded histograms before and after, 0.  The kernels' names: rsi_hot_kernel_times. */
int rsi_hot_debug_candidate_tests(rsi_ctx* ctx, const int32_t* depth, int64_t n, int storage, int64_t span_all, double RDmedian, int m,
                                  double minmlen, double chklen, double buffer, int maxchkbp, const int32_t* start, const int32_t* end,
                                  const int32_t* type, const int32_t* status, int ncand, const int32_t* index, int nindex, int form,
                                  rsi_cand_record* out, int32_t* info);
/* Test hook: exact sums of depth[n] (storage as above) over nranges inclusive ranges (lo[k], hi[k]) through the device tester's
 * range_sums (mean_tp of mergesegments, rsi.cpp:775-779); sums[nranges].  A range with hi < lo, lo < 0 or hi >= n is
 * RSI_ERR_BAD_ARG, as the tester refuses the whole list.  info[2] (may be NULL) = waits, 1 / 0 for ranges in the mailbox / copied. */
int rsi_hot_debug_range_sums(rsi_ctx* ctx, const int32_t* depth, int64_t n, int storage, const int32_t* lo, const int32_t* hi, int nranges,
                             int64_t* sums, int32_t* info);
/* Test hooks: the three list stages behind the scan, each alone over HOST arrays, with the context's own workspace and the device
 * tester a run attaches (use_tester 1) or none (0: the host walks).  Lists travel as rsi_call records (qscore and pad unused); P: the
 * fields the stage reads (m, minmlen, chklen, buffer, maxchkbp, p, merge).  The environment switches of whole runs are not read.
 * RSI_ERR_BAD_ARG, with the context left usable: an entry outside the array or with end < start, a type other than 0 (DEL) / 1 (DUP),
 * m < 1, maxchkbp < 1, minmlen or chklen not positive, a negative buffer, a negative value in the array.  RSI_ERR_UNSUPPORTED: a test
 * whose neighbourhood is no longer than its candidate (the reference aborts).  info[10] (may be NULL) = tests judged from a result
 * launched ahead (spec_hits), tests launched alone (single_tests), tests the device declined (host_fallbacks), first-round block tests
 * judged from the batch (block_batch_hits), the tester's waits, calls of its range sums, merge means answered from the batch of sums,
 * merge means taken by a call of their own, tests with a tester attached, 0.
 *
 * rsi_hot_debug_block_stage: areblockscnv (rsi.cpp:415-546) on nsegs segments in bin space (start, end, type, score, status; judged in
 * place) over binmedint[nb] and status[nb]; ncompact: the compacted length the tests compare nb with.  The bin medians become the
 * context's compacted depth as int32.  sparse 1: the status array is read through the sparse form a scan leaves -- the values inside
 * the maximal runs of non-zero status, run after run -- and needs one such run.  road[nsegs] (may be NULL): the road of every
 * first-round test: 0 the batch's result, 1 the host walk because no batch was run, 2 because a segment rejected since reaches into
 * the left walk, 3 because the left chain was cut, 4 because the device declined. */
int rsi_hot_debug_block_stage(rsi_ctx* ctx, const int32_t* binmedint, const int32_t* status, int64_t nb, int64_t ncompact, double RDmedian,
                              const rsi_params* P, rsi_call* segs, int nsegs, int use_tester, int sparse, int32_t* road, int32_t* info);
/* rsi_hot_debug_merge: mergesegments (rsi.cpp:694-885) on a list in base coordinates whose geno, status, p1 and refsd are the caller's,
 * over depth[n] as bytes (storage 1; a value outside 0 .. 255 is RSI_ERR_BAD_ARG) or as int32 (storage 4).  out[nlist], *nout: the list
 * after both passes. */
int rsi_hot_debug_merge(rsi_ctx* ctx, const int32_t* depth, int64_t n, int storage, double RDmedian, const rsi_params* P, const rsi_call* list,
                        int nlist, int use_tester, rsi_call* out, int32_t* nout, int32_t* info);
/* rsi_hot_debug_calls: everything detectcnv does behind the block tests (rsi.cpp:1860-1931) and sd_filters (rsi.cpp:1753-1792) on nsegs
 * tested segments in bin space over depth[n] (storage as above), with nnoncode regions (sorted, disjoint, end > start, reference coordinates).
 * blocks, raw, kept: room for nsegs records each; counts[3]: how many of each. */
int rsi_hot_debug_calls(rsi_ctx* ctx, const int32_t* depth, int64_t n, int storage, double RDmedian, double RDsd, const rsi_params* P,
                        const rsi_call* segs, int nsegs, const int32_t* noncode_start, const int32_t* noncode_end, int nnoncode, int use_tester,
                        rsi_call* blocks, rsi_call* raw, rsi_call* kept, int32_t* counts, int32_t* info);
/* Test hook: the NB transform (negative_binomial_transfer, rsi.cpp:1145-1185) of the HOST bin sums binsum[nb] through the function a
 * run calls: the formula and the raw minimum (raw[nb]: the array between the two launches), then the subtraction, the scaling and
 * the three overwritten bins (T[nb]).  nb >= 3 (the reference writes bins 0..2) and nb == ncompact / m (the reference's bin count),
 * r > 0; anything else is RSI_ERR_BAD_ARG.  info[8] = the raw minimum as float bits; flags, bucket count and minimum (float bits)
 * of the plan the scale kernel leaves for the first quantile grid (flags: 2 = a non-finite value, 4 = range below 0.01, 8 = too wide
 * for the resident buckets; buckets = (max - min) / 0.01 + 2); the min/max record's words or-ed together, as the kernel leaves them
 * for the next user (0); the scaled levels t0, t2 (float bits) as the scan derives them from the raw minimum; 0.
 * Overwrites the bin arrays the rsi_hot_fetch_* calls read. */
int rsi_hot_debug_nb_transform(rsi_ctx* ctx, const int64_t* binsum, int64_t nb, int m, int64_t ncompact, double RDmedian, double r,
                               float* raw, float* T, int32_t* info);
/* Test hook: filterstatus (rsi.cpp:948-1047) behind a scan pass, over the HOST arrays T[nb] and status[nb] (values in [-Lmax, Lmax],
 * 1 <= Lmax <= 4194304; anything else is RSI_ERR_BAD_ARG).  The pass's last launch is reproduced (first lengths taken from status,
 * both stop levels Lmax), so the status array, its copy, the run boundaries and their export are the production ones; then the
 * function the scan calls: level sums, level choice, run list, edge trimming.  status_out[nb]: the trimmed copy.  info[10] = runs
 * after the last is dropped (-1: nothing was trimmed); 1 / 0 for the run list in the kernel arguments / behind pointers (-1); 1 / 0
 * for boundary entries beyond the eager ones copied / none (-1); level sums by the device (0), by the host loop because the device
 * declined (1), by the host loop of a long scan (2); an unmarked level exists; trimming applies; leveldel; leveladd; the unmarked
 * bins' mean as float bits; 0.  Overwrites the bin arrays the rsi_hot_fetch_* calls read. */
int rsi_hot_debug_filterstatus(rsi_ctx* ctx, const float* T, const int32_t* status, int64_t nb, int Lmax, double dev, int32_t* status_out,
                               int32_t* info);
/* Test hook: the 0.01-grid median and MAD (partition_stat_tp, wufunctions.cpp:364-424) of the HOST array x[nb], restricted to
 * mask[i] == 0 when mask != NULL, through the forms the scan's thresholds take:
 *   mode 0: the device chain of a (median, MAD) pair, the MAD centred on the chain's own median;
 *   mode 1: the device chain of the MAD alone, around `center`;
 *   mode 2: the host-driven form (a min/max launch, a histogram launch, the walk on the host) for the median, then the MAD.
 * Where the chain reports a range too wide for its buckets, or a degenerate median, the pipeline's own fall-backs follow.
 * out[4] = median, its count, MAD, its count (modes 1 and 3: out[0] = center, out[1] = 0).  info[8] = the raw flags and bucket
 * count of the chain's median record, the same of its MAD record (-1 and 0 for a record no chain wrote), 1 / 0 for 16-bit /
 * 32-bit counters in the chain's histogram launch (-1: no chain ran), the number of host-driven medians, 0, 0.
 * A non-finite selected value fails with RSI_ERR_UNSUPPORTED.  Overwrites the bin arrays the rsi_hot_fetch_* calls read. */
int rsi_hot_debug_grid_median(rsi_ctx* ctx, const float* x, const int32_t* mask, int64_t nb, int mode, double center, double* out,
                              int32_t* info);
/* Mode 3 of the same hook, -MED's form: the int32 bin medians x[nb] become floats in the kernel that also plans the MAD's grid
 * around `center`, then the MAD's chain. */
int rsi_hot_debug_grid_mad_i32(rsi_ctx* ctx, const int32_t* x, int64_t nb, double center, double* out, int32_t* info);
/* Test hook: the keyed form of the NB transform and of its two quantile chains, over the HOST bin sums binsum[nb]: every statistic
 * comes from the histogram of the sums (K possible sums, 0 .. K - 1; bins 0..2 apart), T from the table of their values -- through the
 * functions a run calls.  mask == NULL: the transform and the (median, MAD) pair of all bins, as in front of the first scan pass;
 * mask != NULL: after them the pair of the bins with mask[b] == 0, as in front of the second.  nb >= 3, r > 0.
 * T[nb]: the transformed bins.  out[4] = median, its count, MAD, its count (of the masked selection where a mask is given).
 * info[8] = the flags and bucket count of the median record, the same of the MAD record (-1 and 0: no record), the raw minimum as
 * float bits, the form taken (1: keyed; 0: a bin sum lay outside [0, K), the keyed launch declined and the chain of launches ran; -1:
 * the route does not apply -- K above 2^15 or nb < 8 -- and nothing ran), the number of host-driven medians, 0.
 * A non-finite value fails with RSI_ERR_UNSUPPORTED.  Overwrites the bin arrays the rsi_hot_fetch_* calls read. */
int rsi_hot_debug_nb_keyed(rsi_ctx* ctx, const int64_t* binsum, const int32_t* mask, int64_t nb, int m, int64_t K, double RDmedian, double r,
                           float* T, double* out, int32_t* info);

/* Test hook: the classification alone, at any length: fasta[n] is uploaded and classified (K1), the intervals -- taken as
 * rsi_hot_set_exclude takes them -- are applied by the mask kernel when count > 0, and the two planes come back: n/64 + 1 words
 * each, bit j of word w for base 64 w + j, zero beyond n.  Neither arms nor consumes the context's mask. */
int rsi_hot_debug_classify(rsi_ctx* ctx, const uint8_t* fasta, int64_t n, const int64_t* start, const int64_t* end, int count,
                           uint64_t* gcbits, uint64_t* nbits);

/* Test hook: the per-base phase alone -- K1 / K1b, K2j or its fallbacks, the cap, then the K4 route the plan picks -- on a host
 * chromosome uploaded as rsi_hot_run uploads it, with the intervals (count > 0: as rsi_hot_set_exclude takes them) applied, and
 * nothing behind it: chromosomes of a few bins or without spread, which the scan refuses, still show their per-base result.
 * Afterwards "rd_gc", "rd_concat", "binmedint", "binsum" and "noncode" (int32 (start, end) pairs) are fetchable and the phase /
 * kernel names are those of the phase, followed by "k4.form ..." entries whose VALUE is what the K4 launcher chose inside its
 * route: "vr" (LDS histogram range), "sw7" (0 / 1), "parts" (K4m's lanes per bin), "tile bins", "int32 template" (100 MV + EP).
 * out: n, n_noncode, gc_rdmean, byte_escapes, cap_median, n_compact, nbins, RDmedian, RDsd; the rest zero.  On an error out holds
 * what the phase had derived before it. */
int rsi_hot_debug_per_base(rsi_ctx* ctx, const rsi_params* p, const int32_t* depth, const uint8_t* fasta, int64_t n, const int64_t* start,
                           const int64_t* end, int count, rsi_chrom_stats* out);

/* Timing hooks for bench.py: per-kernel HIP-event times (ms) of the last run, by kernel name.
 * names/ms receive up to cap entries; returns the number of timed launches. */
int rsi_hot_kernel_times(const rsi_ctx* ctx, const char** names, float* ms, int cap);
/* Host wall-clock per pipeline phase of the last run (ms, includes waits on the device). */
int rsi_hot_phase_times(const rsi_ctx* ctx, const char** names, double* ms, int cap);
/* Per-kernel event timing: 0 off, 1 an event pair around every launch, 2 around the per-base (HBM-bound)
 * kernels only -- some sixty launches per chromosome make the event records themselves cost 13 % of a pooled step. */
void rsi_hot_set_timing(rsi_ctx* ctx, int on);
/* Mode 3: an event pair around the launches of ONE kernel, named as in rsi_hot_kernel_times' table (e.g. "gc_hist",
 * "cap_compact_bin", "rsi_scan"): what bench.py's timed steps use for the kernel that an untimed pass measured as the
 * dominant one.  NULL / "" = "cap_compact_bin". */
void rsi_hot_set_timing_kernel(rsi_ctx* ctx, const char* name);

/* ---- Pool: several chromosomes in flight on one GPU ------------------------------------------
 * The reference's per-chromosome loop (rsi.cpp:2189-2217) has independent iterations.  A pool owns
 * `nworkers` host threads (created with the pool, asleep while no run is queued; worker 0 is a thread waiting for a run),
 * each with its own context (stream + workspace); the chromosomes of a run are handed out longest first.  Runs may be queued
 * (rsi_pool_submit / rsi_pool_wait below) and are worked on in submission order; several pools (one per GPU) are independent.  At most three HBM-bound
 * per-base phases are in flight per GPU (rsi_pool_set_schedule); bin-level and candidate kernels,
 * copies and the host stages of different chromosomes overlap. */
typedef struct rsi_pool rsi_pool;
#define RSI_MAX_TIMED 64
typedef struct rsi_batch_times {   /* accumulated over rsi_pool_run calls; zero it to start */
  int32_t nkernels, nphases;
  const char* kernel_name[RSI_MAX_TIMED];
  double kernel_ms[RSI_MAX_TIMED];       /* sum of HIP-event durations */
  int64_t kernel_launches[RSI_MAX_TIMED];
  int64_t kernel_bases[RSI_MAX_TIMED];   /* sum over launches of the chromosome length */
  const char* phase_name[RSI_MAX_TIMED];
  double phase_ms[RSI_MAX_TIMED];        /* host wall-clock per pipeline phase, summed over workers */
} rsi_batch_times;

rsi_pool* rsi_pool_create(int device, int nworkers, int* status);
void rsi_pool_destroy(rsi_pool* pool);
int rsi_pool_workers(const rsi_pool* pool);
/* The hardware queues the process had asked for when the pool was made: GPU_MAX_HW_QUEUES as rsi_pool_create found it, 4 (the
 * runtime's default) when it held no number.  A pool with more workers than that minus two (the copy stream's and the host
 * framework's own) shares queues between workers -- the regime of "22 workers: 14-17 ms" -- and rsi_pool_create says so on
 * stderr, once per process, naming GPU_MAX_HW_QUEUES and rsi_hot_process_setup. */
int rsi_pool_hw_queues(const rsi_pool* pool);
rsi_ctx* rsi_pool_worker(rsi_pool* pool, int w);
void rsi_pool_set_timing(rsi_pool* pool, int on);
void rsi_pool_set_timing_kernel(rsi_pool* pool, const char* name);   /* rsi_hot_set_timing_kernel on every worker */
/* Scheduling of the pool's workers on the GPU.  isolate != 0: a chromosome's per-base (HBM-bound) phase runs
 * alone on the chip -- bin-level work of the other workers waits -- so that every streaming launch is a clean
 * bandwidth sample (profiling); 0 (default): bin-level work overlaps it (about 20 % more throughput).
 * streamers: per-base phases allowed in flight at once (default 2; ignored while isolating). */
void rsi_pool_set_schedule(rsi_pool* pool, int isolate, int streamers);
const char* rsi_pool_last_error(const rsi_pool* pool);
/* d_depth[i], d_fasta[i], n[i]: chromosome i, resident in HBM.  out[i] receives its result (or NULL),
 * status[i] (optional) its rsi_status; returns the first failure or RSI_OK.  times may be NULL. */
int rsi_pool_run(rsi_pool* pool, const rsi_params* p, int nchrom, const void* const* d_depth,
                 const void* const* d_fasta, const int64_t* n, rsi_result** out, int* status,
                 rsi_batch_times* times);

/* ---- Plot files (plotcnv.cpp:245-610): from an array in host memory ---------------------------------------------------------
 * The gnuplot data (.dat) and script (.gp) file of one call as plot_icnv writes them.  rd: the capped, GC-adjusted per-base
 * depth with the removed N regions back in as zeros (expand_data, loaddata.cpp:140; rsi_plot_expand builds it from
 * rsi_hot_fetch_i32("rd_concat") and rsi_result_noncode); chrom_median: _median of that array (plot::RDmed).  The reference
 * pipes the script through gnuplot and deletes both files; the writer stops at the files. */
int rsi_plot_expand(const int32_t* rdc, int64_t ncompact, const int32_t* regions, int npairs, int32_t* out, int64_t n);
int rsi_plot_write_files(const rsi_call* c, const char* title, const int32_t* rd, int64_t n, double chrom_median, int m,
                         double minmlen, double chklen, const char* format, double gnuplot_version, const char* datfile,
                         const char* gpfile, const char* imgfile);

/* ---- Plot data from the device -----------------------------------------------------------------------------
 * rsi_plot_write_files in three steps, so that the array never has to leave HBM.  A rsi_plot_batch is a list of calls planned
 * against an array of n values with the run's m / minmlen / chklen: per call the body, the two pieces of the neighbourhood, the
 * running mean's band and one query per printed row (which position, which array value, which running-mean window) -- all of
 * it from the coordinates alone.  A fill then provides a value per query, the exact integer sum of every queried window, the
 * quartiles and sums of body and neighbourhood and the array's median: rsi_plot_batch_fill_host from host memory (what
 * rsi_plot_write_files does), rsi_hot_plot_depth from any int32[n] in HBM (not modified), rsi_hot_plot_run from the last
 * successful run's compacted depth, expanded on the device by its removed regions into a buffer the context keeps.
 * rsi_plot_batch_write writes call i's two files from a filled batch, with the bytes rsi_plot_write_files gives.
 * rsi_plot_batch_add returns 0 or what the writer refuses (1 beyond the array, 2 size error, 3 empty body, 4 no band;
 * rsi_plot_refusal_text): a refused call keeps its index, costs nothing on the device and cannot be written.  _add_span: a
 * call with cnv_st's defaults (length 0, p1 1).
 * On the device 20 bytes per query cross PCIe (two indices up, a value and a sum back) and about 100 bytes per call; a list is
 * processed in batches of as many calls as fit a workspace of 64 MB (at least one), with a number of launches per batch that
 * does not depend on the calls in it.  Every wait has the library's 60 s deadline.  A batch without plannable calls is RSI_OK and
 * launches nothing; a context that never plots allocates nothing for it. */
typedef struct rsi_plot_batch rsi_plot_batch;
rsi_plot_batch* rsi_plot_batch_new(int64_t n, int m, double minmlen, double chklen);
void rsi_plot_batch_free(rsi_plot_batch* b);
int rsi_plot_batch_add(rsi_plot_batch* b, const rsi_call* c);
int rsi_plot_batch_add_span(rsi_plot_batch* b, int start, int end, int type);
int rsi_plot_batch_size(const rsi_plot_batch* b);
int rsi_plot_batch_refusal(const rsi_plot_batch* b, int i);
const char* rsi_plot_refusal_text(int refusal);
int64_t rsi_plot_batch_queries(const rsi_plot_batch* b);
int rsi_plot_batch_fill_host(rsi_plot_batch* b, const int32_t* rd, int64_t n);
double rsi_plot_batch_chrom_median(const rsi_plot_batch* b);   /* of the last fill; 0 before one */
/* Two filled batches of the same calls: 0 when every number of every call is the same (values, window sums, quantiles, sums, the
 * array's median), else 1 + the index of the first call that differs (1 + the number of calls: only the array's median does). */
int rsi_plot_batch_compare(const rsi_plot_batch* a, const rsi_plot_batch* b);
int rsi_plot_batch_write(const rsi_plot_batch* b, int i, const char* title, const char* format, double gnuplot_version, const char* datfile,
                         const char* gpfile, const char* imgfile);
typedef struct rsi_plot_stats {
  int64_t launches, batches, tiles;   /* kernel launches of the last call (geno's and the expansion included), its batches, its window-sum tiles */
  int64_t calls, queries;             /* planned calls filled, and their queries */
  int64_t bytes_up, bytes_down;       /* what crossed PCIe */
  int64_t bytes;                      /* device memory the context holds for this step, the expanded array included (0 until the first call) */
  double ms, expand_ms;               /* wall time of the last call; of its expansion (rsi_hot_plot_run) */
} rsi_plot_stats;
int rsi_hot_plot_depth(rsi_ctx* ctx, const void* d_depth, int64_t n, rsi_plot_batch* b);
int rsi_hot_plot_run(rsi_ctx* ctx, const rsi_result* res, rsi_plot_batch* b);
int rsi_hot_last_plot_stats(const rsi_ctx* ctx, rsi_plot_stats* out);
/* Test hook: the HOST array depth[n] becomes the context's input depth (what rsi_hot_loaded_depth returns) and goes through the
 * same function, with `tile` values per window-sum tile (0: the default, 2048; at most 4096) and a workspace of
 * workspace_bytes (0: the default). */
int rsi_hot_debug_plot(rsi_ctx* ctx, const int32_t* depth, int64_t n, int tile, int64_t workspace_bytes, rsi_plot_batch* b);
/* Test hook: rsi_plot_expand on the device -- compacted values (storage 1: bytes, 4: int32) and (start, end) pairs up, int32[n] back. */
int rsi_hot_debug_plot_expand(rsi_ctx* ctx, const int32_t* rdc, int64_t ncompact, int storage, const int32_t* regions, int npairs, int32_t* out, int64_t n);

/* The same from host memory (load_data_from_text / load_data_from_bam leave the reference's RD in host memory, loaddata.cpp:473-539):
 * every worker moves its chromosome over its own stream (pinned buffers: asynchronous DMA; pageable ones work, staged by
 * the runtime), so the transfers of some chromosomes overlap the kernels of others.  PCIe-bound at 5 bytes per base. */
int rsi_pool_run_host(rsi_pool* pool, const rsi_params* p, int nchrom, const int32_t* const* depth,
                      const uint8_t* const* fasta, const int64_t* n, rsi_result** out, int* status,
                      rsi_batch_times* times);

/* Samples back to back (the reference is started once per sample; a sequencing centre runs them one after the other): queue a
 * run and return at once.  The pool's workers take chromosomes in submission order, so a worker that finds no chromosome left
 * in one run starts on the next -- the last, short chromosomes of one sample run beside the first, long ones of the next
 * instead of leaving most of the GPU idle.  The pointer arrays are copied; `out`, `status`, `times` and the data they point
 * to must stay valid until rsi_pool_wait has returned for the ticket.  Returns 0 for bad arguments.  rsi_pool_wait returns
 * the run's worst status; the calling thread works as one of the pool's workers while it waits (on the runs up to its own).
 * rsi_pool_run is submit + wait; any number of threads may call the three.  Every ticket must be waited for before
 * rsi_pool_destroy. */
uint64_t rsi_pool_submit(rsi_pool* pool, const rsi_params* p, int nchrom, const void* const* d_depth,
                         const void* const* d_fasta, const int64_t* n, rsi_result** out, int* status,
                         rsi_batch_times* times);
int rsi_pool_wait(rsi_pool* pool, uint64_t ticket);

#ifdef __cplusplus
}
#endif
#endif
