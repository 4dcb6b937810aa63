// kernels.h -- launch wrappers of the gfx950 kernels behind librsi_hot.so.
// Every wrapper enqueues on `stream` and returns without synchronising.  Pointers are device
// pointers unless the name says otherwise.  Kernel list and the roofline that bounds each one:
// DESIGN.md section 4.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <mutex>
#include "device_util.h"
#include "bam_walk_core.h"

namespace rsik {

// A rejected launch (too much dynamic LDS, a bad grid) raises no error where it happens: the wrappers below return nothing.
// Every launch of the library therefore goes through RSI_LAUNCH, which reads the runtime's last error right behind the launch
// and keeps the first failure in a thread-local slot; the pipeline's next wait (ctx_sync) collects it.  A context's launches all
// come from the thread that runs it, and the entry points drain whatever the host application's own calls left in the runtime's
// slot before the first launch (drain_stale_errors), so only this library's launches are attributed to a run.
inline void note_launch() {   // tl_launch_error: device_util.h
  const hipError_t e = hipGetLastError();   // cleared by the read
  if (e != hipSuccess && tl_launch_error == hipSuccess) tl_launch_error = e;
}
inline void drain_stale_errors() { (void)hipGetLastError(); tl_launch_error = hipSuccess; }
inline hipError_t take_launch_error() { const hipError_t e = tl_launch_error; tl_launch_error = hipSuccess; return e; }
#define RSI_LAUNCH(...) do { hipLaunchKernelGGL(__VA_ARGS__); rsik::note_launch(); } while (0)

constexpr int kGcLevels = 202;        // window GC count 0..201 (gccontent.cpp:102, 115)
constexpr int kHistValues = 65536;    // directly indexed integer histogram range
constexpr int kResClasses = 32;       // 31 MAD residues (rsi.cpp:1130) + 1 class for the tail
constexpr int kTileBases = 4096;      // bases per workgroup tile in the streaming kernels

// ---- K1: FASTA bytes -> GC bitmask + N bitmask (loaddata.cpp:481-483; readref.cpp:95) ----
// gcbits/nbits hold nwords = n/64 + 1 words, bit j of word w <-> base 64*w + j, zero beyond n.
// `fill`: ranges cleared for the kernels that follow in the stream (K1 is the first kernel of a chromosome's chain)
void launch_fasta_classify(const uint8_t* fasta, int64_t n, uint64_t* gcbits, uint64_t* nbits, int64_t nwords,
                           const FillList& fill, hipStream_t stream);
void launch_fill(const FillList& fill, hipStream_t stream);   // the same clearing as a launch of its own (rare paths)
// ---- K1x: excluded intervals -> N in both planes (nbits |= bit, gcbits &= ~bit), behind K1 and before anything reads them ----
// starts / ends: `count` intervals [s, e) in device memory, sorted, disjoint and not touching, all inside [0, n);
// first_start = starts[0], last_end = ends[count - 1] (host copies: the grid covers the mask's span only).  count <= 0: no launch.
void launch_exclude_mask(const int64_t* starts, const int64_t* ends, int count, int64_t first_start, int64_t last_end,
                         uint64_t* gcbits, uint64_t* nbits, hipStream_t stream);
// Scratch for the in-kernel folds of the per-workgroup slabs (device_util.h, fold_slabs): group sums of the widest slab.
// counters: kFoldGroups + 1 arrival counters per kernel, zero before the launch (every launch leaves them zero).
size_t fold_scratch_bytes();
// What the per-base kernels hand each other on the device, so that K4j can be queued behind K2j without the host in between:
// the regions K4j removes (K1b's last workgroup), the cap (K2j's last workgroup), and K4j's verdict on its launch configuration.
struct PhaseParams {
  int32_t nreg;        // padded, merged N regions (cbreak / cum in device memory)
  int32_t capval;      // (int)(cap median * cap), or < 0: not known on the device (escapes pending, deep coverage, wrapped counters)
  int64_t ncompact;    // n minus the removed bases
  int32_t regions_ok;  // 0: the boundary list was too long or malformed for the device: the host's regions count
  int32_t redo;        // set by K4j: launched with a configuration that does not fit the cap -- nothing written, launch again
  int32_t pad[2];
};
// K1b's arguments, for the launch that does its work on the way (K2j, round 5): the N mask, the boundary list and its count (zero before),
// the padding of get_noseq_regions (loaddata.cpp:243-273), where the compacted break points and removed lengths go
struct NRuns { const uint64_t* nbits; uint64_t* list; uint32_t* count; uint32_t cap; int32_t dx; int64_t* cbreak; int64_t* cum; };
// ---- K1b: run boundaries of the N bitmask -> unordered list of (pos << 1 | is_end) ----
// pp != NULL: the last workgroup also builds cbreak[4100] / cum[4097] (regions padded by dx, merged) and fills pp's region fields;
// counter: an arrival counter, zero before and after.
void launch_n_transitions(const uint64_t* nbits, int64_t nwords, uint64_t* list, uint32_t* count, uint32_t cap, int64_t n, int dx,
                          PhaseParams* pp, int64_t* cbreak, int64_t* cum, unsigned int* counter, hipStream_t stream);

// ---- K2: GC table accumulation (checkgccontent pass 1, gccontent.cpp:105-145) ----
struct GcAccum {
  unsigned long long sum[kGcLevels];   // sum of depth per window GC count
  unsigned long long cnt[kGcLevels];
  unsigned long long possum, poscnt;   // over depth > 0
  unsigned int negatives;              // bit 0: depth < 0 seen (unsupported); bit 1: depth >= 2^21, packed form invalid
  unsigned int escapes;                // bases of kByteEscape and more (saturating count): their byte copy is the escape code
};
// K2 leaves a byte copy of the depth behind (depth8[i] = min(depth[i], kByteEscape)): the later per-base passes stream one
// byte per base instead of four and turn to the int32 array only where a byte says kByteEscape.
constexpr int kByteEscape = 255;
// K3' leaves a byte copy of the GC-RESCALED depth behind, saturated at kByteSat ("this much or more"): K4' streams it when
// the cap is below that (a saturated value is capped either way).
constexpr int kByteSat = 254;
// packed = 1: one LDS atomic per base (count and sum in one 64-bit word), valid for depths < 2^21;
// when the result carries flag bit 1 the caller zeroes acc and launches again with packed = 0.
// slabs: scratch of gc_hist_slab_bytes(n) bytes (per-workgroup partial results, folded by a second tiny kernel).
// The last workgroup to finish folds the slabs into acc, adds the last n % 4 bases and builds table[kGcLevels + 1]
// (level means, then the mean of the positive depths): gccontent.cpp:109-112, 141-145.
size_t gc_hist_slab_bytes(int64_t n);
void launch_gc_hist(const int32_t* depth, const uint64_t* gcbits, int64_t n, GcAccum* acc, double* table, int packed, void* slabs,
                    void* gsum, unsigned int* counters, uint8_t* depth8 /* n + 16 bytes, or NULL */, hipStream_t stream);

// ---- K3: GC rescale + value histogram (adjustgccontent, gccontent.cpp:43-92; feeds apply_cap) ----
// table[202] and rdmean as computed on the host from GcAccum.  out may be NULL (histogram only);
// adjust=0 copies depth through unchanged (the -NOGC path only needs the histogram).
// hist[kHistValues] counts output values < kHistValues; *big counts the rest; *vmax: the largest value of 256 and more seen
// (0: none) -- counters beyond it are zero, which bounds the median walk.
struct ValueHistAux { unsigned long long big; unsigned int vmax; unsigned int negatives; };
// Median walk of partition_stat_tp (wufunctions.cpp:398-420, dy = 1) over hist[kHistValues] for `total` values, on the device:
// inrange = sum of the counters, lo / hi = smallest / largest value present (lo > hi: none), med = the bucket where the
// cumulated count first reaches total/2 (-1: never).
struct ValueMedian { unsigned long long inrange; int32_t lo, hi, med, pad; };
// ---- K2j: K2 with the joint histogram [window GC count][depth byte] (kernels_base.hip): its last workgroup builds the GC table,
// the value histogram of the RESCALED depth (what K3' computed per base), walks it to the cap median (*vm) and hands the
// header over (head_src -> head_dst, mapped host memory) -- the chromosome needs no K3'.  acc->negatives bit 2: a
// workgroup's 16-bit counters wrapped, the launch's results are void (the caller runs K2 + K3' instead); acc->escapes > 0:
// the histogram lacks the depths of 255 and more until launch_escape_hist has run.  totals: gc_joint_totals_bytes(), zero
// before the launch; hist / aux zero before the launch; counters: kFoldGroups + 1 arrival counters.
// esc_list: gc_joint_esc_list_bytes() of scratch (the workgroups' first escapes by position: the last workgroup adds them to the
// histogram itself; info->esc_pending says when there were too many for that).  rtab: kGcLevels words, per level the 16.16
// fixed-point ratio K4j rescales depth bytes with (verified against the reference's expression for every byte; bit 31: not
// usable, take the exact expression).
struct JointInfo { int32_t gmin, gmax;   // GC levels that occur
                   int32_t vmax;         // largest depth byte below kByteEscape that occurs
                   int32_t esc_pending;  // 1: the value histogram lacks the escapes (launch_escape_hist), or the coverage is deep (int32 kernels)
};
size_t gc_joint_slab_bytes(int64_t n);
size_t gc_joint_totals_bytes();
size_t gc_joint_esc_list_bytes();
void launch_gc_joint_hist(const int32_t* depth, const uint64_t* gcbits, int64_t n, GcAccum* acc, double* table, void* slabs, void* totals,
                          unsigned int* counters, uint8_t* depth8 /* n + 2048 bytes */, uint32_t* hist, ValueHistAux* aux, ValueMedian* vm,
                          const void* head_src, void* head_dst, size_t head_bytes, void* esc_list, unsigned int* rtab, JointInfo* info,
                          PhaseParams* pp /* capval (and redo = 0) for a K4j queued behind */, double cap_mult, hipStream_t stream,
                          const NRuns* nruns = nullptr /* K1b's work inside this launch (see NRuns) */);
void launch_escape_hist(const uint8_t* depth8, const int32_t* depth, const uint64_t* gcbits, int64_t n, const double* table, uint32_t* hist,
                        ValueHistAux* aux, unsigned int* counter, ValueMedian* vm, const void* head_src, void* head_dst, size_t head_bytes,
                        hipStream_t stream);

size_t gc_rescale_slab_bytes(int64_t n);   // scratch for the per-workgroup histograms
// table: kGcLevels level means followed by the mean of the positive depths (K2's last workgroup builds it).
// The last workgroup to finish folds the slabs into hist, fixes the tail quirks of the 20-slice write-back (SURVEY App. A
// Q2/Q3) in out[] and hist[], adds the last n % 4 bases (which the streaming loop leaves out), walks hist to *vm and
// copies head_bytes from head_src (device) to head_dst (mapped host memory; NULL: no copy).
void launch_gc_rescale(const int32_t* depth, const uint64_t* gcbits, int64_t n, const double* table,
                       int adjust, int32_t* out, uint32_t* hist, ValueHistAux* aux, void* slabs, void* gsum,
                       unsigned int* counters, ValueMedian* vm, const void* head_src, void* head_dst, size_t head_bytes,
                       hipStream_t stream, uint8_t* out8 = nullptr,
                       PhaseParams* pp = nullptr /* the launch's last workgroup leaves the cap there (median x cap_mult, or -1) for a K4 queued behind it */,
                       double cap_mult = 0.0);
// Only the rescaled array: out[] as the launch above leaves it, nothing else touched (rsi_hot_fetch of "rd_gc" when the run
// itself streamed the byte copy and never wrote the int32 array).
void launch_gc_materialize(const int32_t* depth, const uint64_t* gcbits, int64_t n, const double* table, int32_t* out,
                           unsigned int* counter, hipStream_t stream);
// The value histogram of the rescaled depth from the byte copy, nothing written per base (what apply_cap's median needs,
// loaddata.cpp:233); same last-workgroup work as launch_gc_rescale.
size_t value_hist8_slab_bytes(int64_t n);
void launch_value_hist8(const uint8_t* depth8, const int32_t* depth, const uint64_t* gcbits, int64_t n, const double* table,
                        uint32_t* hist, ValueHistAux* aux, void* slabs, void* gsum, unsigned int* counters, ValueMedian* vm,
                        const void* head_src, void* head_dst, size_t head_bytes, uint8_t* rescaled8 /* n + 2048 bytes */,
                        const unsigned int* escapes /* K2's count of bases that did not fit a byte (GcAccum::escapes) */, hipStream_t stream);
// Above this many escaped bases (n / 8) the byte path is not worth taking: K3' only hands the header over and the host
// runs the int32 kernels (deep coverage, 250x and more).
unsigned int byte_escape_limit(int64_t n);

// ---- K4: cap + N-region compaction + per-bin median/sum + chromosome statistics ----
// (apply_cap loaddata.cpp:229; concatenate_data loaddata.cpp:48; _median/variance rsi.cpp:2202;
//  median_transfer rsi.cpp:1363; bin sums + MAD subsamples rsi.cpp:1127-1157)
struct BinAccum {
  unsigned long long big;        // values >= kHistValues (not in the histograms): unsupported by the caller
  unsigned int vmax;
  unsigned int pad;
};
// cbreak[k]: compacted index where region k is cut out; cum[k]: bases removed before compacted
// index cbreak[k] (cum[nreg] = total).  res_hist: [kHistValues][kResClasses] counts of value by
// class (compacted index mod 31, or 31 for the tail beyond 31*floor(n'/31)); the chromosome's sum,
// sum of squares and median all derive from it.
// slabs: scratch of cap_compact_slab_bytes(...) bytes for the per-workgroup histograms.
// The last workgroup to finish folds the slabs into res_hist and copies exp_bytes from exp_src (device) to exp_dst
// (mapped host memory).  cap_compact_overwrites(): every value is below the LDS range (the cap is), res_hist is
// overwritten and needs no clearing; otherwise it must be zero before the launch.  Region lists of up to kRegInline
// entries travel in `inl` with the kernel arguments (cbreak / cum may then be NULL).
constexpr int kRegInline = 48;
struct K4Regions { long long brk[kRegInline]; long long cum[kRegInline + 1]; };
// The arguments of the K4 launchers below (pipeline.hip fills them once per launch site; each form reads its own).  src: the depth as
// int32 (what K4 / K4w compact, what the byte forms recompute edge tiles from); src8: the byte forms' input, K2 / K2j's copy of the
// raw depth (K4j, K4s) or the histogram pass' copy (K4', RAW K4s); rdc8 / rdc: the output as bytes / as int32; acc: K4 only;
// gsum: K4, K4', K4j; rtab, escapes, pp: see K4j and K4s; vbase: K4 / K4w; raw: K4' on the raw depth (-NOGC).
// What a K4 launcher chose inside its route, reported by the launcher itself where K4Args::form is set (test hook
// rsi_hot_debug_per_base; -1 / 0: the route has no such choice): the LDS histogram's value range, the median phase's packing,
// K4m's lanes per bin, the tile's bins (K4', K4j, K4w, K4), the int32 K4's template <MV, EP> as 100 MV + EP.
struct K4Form { int vr = 0, sw7 = -1, parts = 0, tile_bins = 0, tmpl = -1; };
struct K4Args {
  const int32_t* src; const uint8_t* src8; const uint64_t* gcbits; int64_t n; const double* table;
  const int64_t* cbreak; const int64_t* cum; const K4Regions* inl; int nreg; int64_t ncompact; int32_t capval; int m;
  uint8_t* rdc8; int32_t* rdc; int32_t* binmed; int64_t* binsum; uint32_t* res_hist; BinAccum* acc;
  void* slabs; void* gsum; unsigned int* counters; const void* exp_src; void* exp_dst; size_t exp_bytes;
  const unsigned int* rtab; const unsigned int* escapes; PhaseParams* pp; int vbase; int raw; hipStream_t stream;
  K4Form* form;   // NULL, or where the launcher notes its choice
};
size_t cap_compact_slab_bytes(int m, int32_t capval, int64_t ncompact, int vbase);
int cap_compact_overwrites(int m, int32_t capval, int64_t ncompact, int vbase);
// First value of the window the LDS histograms of the int32 kernels cover: 0 unless the distribution's centre (mean / median
// depth) is 160 and more, then centre - 3/8 width; values outside the window are counted with global atomics, slowly but
// exactly.  K3 derives its window on the device (1024 values); K4's (kK4Window = 512 values) comes from the host.
constexpr int kK4Window = 512;
int hist_window_base(double center, int width);
void launch_cap_compact_bin(const K4Args& a);

// K4w: the same for caps of 254 .. 32766 (deep coverage): int32 in, 16-bit tile and 16-bit window counters in LDS, int32 out.
// res_hist must be zero before the launch (the window's sums and the stray values are added to it); vbase as for K4.
int cap_compact16_applies(int m, int32_t capval, int64_t ncompact);
size_t cap_compact16_slab_bytes(int m, int64_t ncompact);
void launch_cap_compact_bin16(const K4Args& a);

// K4' fed from K3''s byte copy of the rescaled depth (src8): the rescaled int32 array is never needed.  Applies when
// cap_compact8_applies(): 1 <= capval < kByteSat (every capped value fits a byte, res_hist is overwritten) and m <= 440.
// src / gcbits / table: for the tiles at the chromosome's ends and across removed regions, which recompute the rescale per
// element.  rdc8: ncompact + 64 bytes.
int cap_compact8_applies(int m, int32_t capval);
size_t cap_compact8_slab_bytes(int m, int32_t capval, int64_t ncompact);
// The byte forms' shape under a cap (K4', K4j, K4s, K4m): the value range of the LDS histogram (64, 128 or 256 values, covering
// the cap) and the median phase's packing (SW7: four values to a register up to a cap of 127).
struct ByteShape { int vr; bool sw7; bool operator==(const ByteShape& o) const { return vr == o.vr && sw7 == o.sw7; } };
inline ByteShape byte_shape(int32_t capval) { int vr = 64; while (vr < 256 && vr <= capval) vr <<= 1; return {vr, capval <= 127}; }
void launch_cap_compact_bin8(const K4Args& a);

// K4j: K4' fed from the byte copy of the RAW depth (K2 / K2j's depth8), rescaling on the way with the GC table -- same outputs.
// rtab: K2j's fixed-point ratios, or NULL: the float form with its exactness margin.  pp: NULL, or nreg / ncompact / capval are
// read from it on the device (cbreak / cum from device memory); the arguments of those names only shape the launch (capval: a
// guess, checked).
void launch_rescale_compact_bin8(const K4Args& a);

// K4 as two launches (kernels_k4s.hip): K4s -- rescale, cap, compaction, byte store, residue-class histogram, wave-autonomous at
// eight waves per SIMD, fixed point in the loop, the chunks it cannot do that way (region cuts, chromosome ends, escape bytes, GC
// levels without a verified ratio) exactly behind it -- and K4m -- the bins' medians and sums from the bytes K4s leaves, no LDS.
// Together the arguments and results of launch_rescale_compact_bin8 with rtab (no gsum: the groups' sums are atomic adds) wherever
// rescale_compact_split_applies(); slabs: rescale_compact_split_slab_bytes(); rdc8: rescale_compact_split_rdc_bytes() (padded to
// whole sub-tiles); escapes: K2j's count of depths of 255 and more (GcAccum::escapes, device memory).
int rescale_compact_split_applies(int m, int32_t capval, int64_t ncompact, int nreg);
size_t rescale_compact_split_slab_bytes(int32_t capval, int64_t ncompact);
size_t rescale_compact_split_rdc_bytes(int64_t ncompact);
void launch_rescale_compact_stream(const K4Args& a);
void launch_bin_median8(const K4Args& a);

// ---- which K4 form a chromosome takes ----
// The per-base phase's A/B switches (RSI_HOT_<NAME>=0 turns each off, RSI_HOT_K1B_INSIDE=1 turns that one on), read once per run.
struct PerBaseSwitches {
  bool joint;        // K2j (RSI_HOT_JOINT); off: the three-pass chain K2, K3', K4'
  bool spec;         // K4 queued behind K2j / the -NOGC histogram pass (RSI_HOT_SPEC)
  bool k4j_fix;      // K2j's verified fixed-point ratios (RSI_HOT_K4J_FIX); off: K4j's float form
  bool k4split;      // K4s + K4m where they apply (RSI_HOT_K4SPLIT); off: K4j
  bool nogc_bytes;   // -NOGC on bytes (RSI_HOT_NOGC_BYTES); off: the int32 kernels
  bool k4w;          // K4w for caps of 254 .. 32766 (RSI_HOT_K4W); off: the int32 K4
  bool k1b_inside;   // K1b inside K2j's launch (RSI_HOT_K1B_INSIDE)
};
// stream: K4s + K4m; joint: K4j; bytes: K4'; wide16: K4w; int32: K4
enum class K4Route { stream, joint, bytes, wide16, int32 };
struct K4Plan {
  K4Route route;
  bool fixed;            // K4s / K4j rescale with K2j's verified fixed-point ratios (K4j without them: the float form)
  bool raw;              // -NOGC: the bytes are the values (K4s in RAW mode, K4' with raw = 1)
  bool bytes_fit;        // a cap under which every value fits a byte (cap_compact8_applies), whatever the route
  ByteShape shape;       // byte_shape(capval)
  const char* marks[2];  // the route's phase markers (rsi_hot_phase_times), NULL where none
};
// The route for what the host knows after the cap: capped = a cap applies; deep: the rescale went through the int32 kernel;
// joint_ok: K2j ran to the end and its ratios verified.  The queued launch asks with its guessed cap, ncompact = n and nreg = 0.
K4Plan k4_plan(bool gcadjust, bool capped, int32_t capval, int m, int64_t ncompact, int nreg, bool deep, bool joint_ok,
               const PerBaseSwitches& sw);

// ---- K5: NB variance-stabilising transform (negative_binomial_transfer, rsi.cpp:1155-1185) ----
// raw[b] = (float)(2 sqrt(r) log(sqrt(q) + sqrt(1+q))), q = (sum+0.25)/(m2*r-0.5); *rawmin_bits =
// complement of the smallest order key over the bins (atomicMax; zero on entry = nothing seen).
void launch_nb_raw(const int64_t* binsum, int64_t nb, int m, int64_t ncompact, double r, float* raw,
                   uint32_t* rawmin_bits, hipStream_t stream);
// ---- K6: 0.01-grid histogram quantiles of float arrays (partition_stat_tp, wufunctions.cpp:364) ----
// min_inv = complement of the smallest order key seen, max_bits = largest key; all zero = nothing seen yet
struct MinMaxF { uint32_t min_inv, max_bits; unsigned int nonfinite; unsigned int pad; };
// The whole median as a chain of two launches (min/max + grid plan by the last workgroup -> histogram + walk by the last
// workgroup); `out` receives the result, or the flag of the first test that failed.
struct GridMedian { double med, ymin; unsigned long long count; uint32_t np, flags; };
enum { kGridEmpty = 1, kGridNonFinite = 2, kGridDegenerate = 4, kGridTooWide = 8,
       kGridDeclined = 16 /* the keyed form met a bin sum outside its table: the chain of launches follows (launch_nb_keys) */ };
// Shared state of a context's chains: mm holds "nothing seen" (all zero) before a chain and again after it; hist has cap
// entries; counters: two arrival counters (plan, walk), zero before and after.
struct GridChain { MinMaxF* mm; uint32_t* hist; uint32_t cap; unsigned int* counters; };
// what the last workgroup of launch_hist_walk copies to mapped host memory (NULL dst: nothing)
struct GridExport { const void* src[2]; void* dst[2]; size_t bytes[2]; };

// x = (float)(raw - tmin); x = (float)(x / med_nbt * med); bins 0..2 <- the three reference levels (rsi.cpp:1176-1185), where
// tmin is the minimum launch_nb_raw left in *rawmin_bits and med_raw / del_raw / dup_raw are the transform of the median,
// half and one-and-a-half times the median depth computed by the host (the kernel and the host derive the scaled levels
// with the same IEEE operations).  The values' min/max are taken on the way and the last workgroup plans the median's grid
// into *out: first link of a chain, continue with launch_hist_walk.
void launch_nb_scale_minmax(float* x, int64_t nb, const uint32_t* rawmin_bits, double med_raw, double del_raw, double dup_raw,
                            double RDmedian, const GridChain& c, GridMedian* out, hipStream_t stream);
// -MED: out_f = (float)in, min/max of |out_f - center| taken on the way (first link of the MAD chain)
void launch_i32_to_f32_minmax(const int32_t* in, float* out_f, int64_t nb, double center, const GridChain& c, GridMedian* out,
                              hipStream_t stream);
// min/max over x[i] (or |x[i]-center| rounded to float when use_abs), restricted to mask[i]==0 when mask != NULL
void launch_minmax_f32(const float* x, const int32_t* mask, int64_t nb, int use_abs, double center, MinMaxF* mm,
                       hipStream_t stream);
// hist[(size_t)((v - ymin)/0.01 + 0.5)] += 1, same selection as above; hist has np entries
void launch_hist_f32(const float* x, const int32_t* mask, int64_t nb, int use_abs, double center, double ymin,
                     uint32_t* hist, uint32_t np, hipStream_t stream);
// first link: min/max of the selection, grid planned into *out.  d_center != NULL: the centre is read from device memory
// (an earlier chain's `med`).
void launch_minmax_plan(const float* x, const int32_t* mask, int64_t nb, int use_abs, double center, const double* d_center,
                        const GridChain& c, GridMedian* out, hipStream_t stream);
// second link: histogram on the planned grid, median into *out; then the export, and `fill` for the kernels behind it
void launch_hist_walk(const float* x, const int32_t* mask, int64_t nb, int use_abs, double center, const double* d_center,
                      const GridChain& c, GridMedian* out, const GridExport* ex, const FillList* fill, hipStream_t stream);
// whether launch_hist_walk counts nb values with 16-bit LDS counters (else 32-bit)
bool hist_walk_pack16(int64_t nb);

// ---- K5 + K6 from the histogram of the bin sums (the "keyed" form) ----
// The NB value of a whole bin is a function of its integer sum, so the transformed array's minimum, both 0.01 grids, their bucket
// counts and the walks to the median and the MAD follow from H[sum] alone.  launch_nb_keys counts the sums in [0, K) of the bins
// with mask[b] == 0 (mask NULL: all), bins 0..2 apart (they hold the three levels, not their sums' values); its last workgroup
// evaluates the chain's expressions once per occupied sum and leaves the two GridMedian records at g[0], g[1] and the export exactly
// as launch_nb_scale_minmax + launch_hist_walk + launch_minmax_plan + launch_hist_walk would.  Without a mask it also finds the raw
// minimum (*rawmin_bits) and writes the table tval[sum] (tval[K + b]: the level of bin b < 3); with one it reads that table.
// launch_nb_apply then writes T[b] = tval[binsum[b]].  A sum outside [0, K): g[0].flags = kGridDeclined and nothing else is valid.
// ws: nb_keys_workspace_bytes() bytes, zero before the first launch (the kernels leave its counters zero again).
constexpr int64_t kNbKeyMax = 1 << 15;   // the widest table (pipeline_steps.h: nb_keyed_applies)
size_t nb_keys_workspace_bytes();
void launch_nb_keys(const int64_t* binsum, const int32_t* mask, int64_t nb, int m, int64_t K, double r, double med_raw, double del_raw,
                    double dup_raw, double RDmedian, void* ws, uint32_t* rawmin_bits, const GridChain& c, GridMedian* g,
                    const GridExport* ex, const FillList* fill, hipStream_t stream);
void launch_nb_apply(const int64_t* binsum, int64_t nb, int64_t K, const void* ws, float* T, const FillList* fill, hipStream_t stream);

// ---- K7: RSI scan (rsistatus, rsi.cpp:1191-1259; runmeantp wufunctions.cpp:573-647) ----
struct ScanParams {
  int64_t nb;
  int32_t Lmax;
  int16_t pad;
  int16_t kcap;      // set by launch_rsi_scan: highest block level of the mark tables
  double tmedian;
  double lim_del;    // 0.75 * RDmedian
  double lim_dup;    // 1.25 * RDmedian
};
// Longest scan: the reference's Lmax is max(20, 10000/m, cal_max) (rsi.cpp:1830-1831): 10000 at -m 1.  Up to kScanLdsL the exact
// sweep's tile (256 bins + a halo of Lmax/2 + 1 each side, staged with its rank and mark tables) fits the 160 KB of LDS; longer
// scans keep the same code on a tile in device memory (a workspace slice per workgroup): slow per tile, but the detection pass
// in front sends only the tiles that can hit there.  Staged indices are 16 bits.
constexpr int kMaxScanL = 10400;
constexpr int kScanLdsL = 3800;
constexpr int kScanPad = 8;   // thr_del / thr_dup carry this many unreachable entries (-inf / +inf) after index Lmax
// thr_del[L], thr_dup[L] (L = 1..Lmax, index L): a window of length L is a DEL hit iff
// sum <= thr_del[L], a DUP hit iff sum >= thr_dup[L] (host-derived, see scan_thresholds()).
// first_del / first_dup: smallest L that marks the bin, 0xffffffff when none.  counters[0] = trim
// escapes, counters[1] = values breaking the exact-sum precondition.
constexpr int kThrInline = 232;   // thresholds that fit the kernel arguments: Lmax + 1 + kScanPad <= kThrInline
struct ScanThr { double del[kThrInline]; double dup[kThrInline]; };
// inl != NULL: thresholds in the kernel arguments (thr_del / thr_dup unused)
// Two launches (kernels_bin.hip): a detection pass lists the tiles of 256 bins in which any lane can hit at any L (float
// prefixes against thresholds widened by the rounding bound: a superset), the exact sweep then runs on the listed tiles only,
// each tile's lengths split over several workgroups.  tiles: scratch for (nb / 256 + 1) tile indices; NULL = no detection
// pass, every tile through the exact sweep.  counters: the pass' work block (zero before): [0] trim escapes, [1] values
// breaking the exact-sum precondition, [8] tiles listed, [9] the exact sweep's task counter.
void launch_rsi_scan(const float* T, const int32_t* medint, const ScanParams& sp, const double* thr_del,
                     const double* thr_dup, const ScanThr* inl, uint32_t* first_del, uint32_t* first_dup, uint32_t* counters,
                     uint32_t* tiles, void* tile_ws /* scan_tile_workspace_bytes(Lmax) when that is not 0 */, hipStream_t stream);
size_t scan_tile_workspace_bytes(int Lmax);   // 0: the exact sweep's tile fits LDS
// Stop levels of the two sweeps (rsi.cpp:1225, 1255; DEL marks win, App. A Q14) in one launch.
// work: [16 uint32: escapes, inexact (the scan's), ldel, ldup, both-count, ...][hist_del][hist_dup] (scan_level_stride(Lmax) words each), zero
// before the scan; both: scratch for kBothCap (first_del, first_dup) pairs.  The last workgroup copies host_bytes of work to
// host_copy (mapped host memory).
constexpr int kMaxLevels = 10416;   // >= kMaxScanL + 1 + kScanPad, a multiple of 4
inline int scan_level_stride(int Lmax) { return (Lmax + 1 + kScanPad + 3) & ~3; }   // hist_dup sits this many words behind hist_del
// the words of that record the host reads (pipeline_steps.h: ScanRecord); [8] is the scan's own (tiles listed, launch_rsi_scan)
constexpr int kScanRecEscapes = 0, kScanRecInexact = 1, kScanRecStop = 2 /* ldel, ldup */, kScanRecTiles = 8, kScanRecLevels = 16;
constexpr size_t kScanWorkBytes = 64 + 2 * (size_t)kMaxLevels * 4;
void launch_level_stop(const uint32_t* first_del, const uint32_t* first_dup, int64_t nb, int32_t Lmax, uint32_t* work, void* both,
                       unsigned int* counter, void* host_copy, size_t host_bytes, hipStream_t stream);
// status[j] = -first_del[j] if first_del[j] <= levels[0]; else +first_dup[j] if <= levels[1]; else 0; copy (may be NULL)
// receives the same.  Run boundaries appended unordered to runs as (pos << 1 | is_end), *count entries (zero before);
// host_copy (may be NULL): [count, 0][first host_entries entries] written by the last workgroup.
void launch_resolve_runs(const uint32_t* first_del, const uint32_t* first_dup, const uint32_t* levels, int64_t nb, int32_t* status,
                         int32_t* copy, uint64_t* runs, uint32_t* count, uint32_t cap, unsigned int* counter, void* host_copy,
                         uint32_t host_entries, hipStream_t stream);

// ---- K9/K10: marked runs and max-score sub-segment (get_continuous_segments rsi.cpp:291;
//      get_rsi_segments rsi.cpp:1060) ----
struct BestSeg { double score; int32_t start; int32_t len; };
struct SegItem { int32_t run; int32_t len; int32_t Lbeg; int32_t Lend; };   // lengths [Lbeg, Lend) of one run
// Short run / item lists ride in the kernel arguments (the pointer forms are for longer ones).
constexpr int kRunsInline = 200, kItemsInline = 150;
constexpr int kBestLds = 6144;   // doubles of a run's prefix k_best_subsegment stages in LDS (48 KB); a longer prefix is read from global memory
struct RunsInline { int32_t se[2 * kRunsInline]; int32_t off[kRunsInline]; };     // (start, end) pairs; prefix offsets
struct ItemsInline { SegItem it[kItemsInline]; int32_t off[kRunsInline]; };
// exact double prefix of every run into scratch + poff[run] (len+1 entries), one workgroup per run
// status_out (may be NULL; may be mapped host memory): the runs' status values, run after run, value e of run r at poff[r] - r + e
void launch_run_prefix(const float* T, const int32_t* run_start, const int32_t* run_end, const RunsInline* inl, int nruns,
                       const int64_t* poff, double* scratch, const int32_t* status, int32_t* status_out, hipStream_t stream);
// one workgroup per work item; out[item] = best (score, offset, L) of that item under the
// reference's visiting order (larger score, then smaller L, then smaller offset); out may be mapped host memory
void launch_best_items(const void* items, const ItemsInline* inl, int nitems, const int64_t* poff, const double* scratch,
                       double tmedian, BestSeg* out, hipStream_t stream);
// edge trimming of filterstatus (rsi.cpp:1023-1044): one thread per run
void launch_trim_runs(const float* T, int32_t* status, const int32_t* run_start, const int32_t* run_end, const RunsInline* inl,
                      int nruns, double delthr, double addthr, hipStream_t stream);

// ---- filterstatus' per-level float sums on the device (kernels_fs.hip; rsi.cpp:967-976, App. A Q13) ----
// out: [2 Lmax + 1] float sums then [2 Lmax + 1] int32 counts, index = level + Lmax: the sum of T over the bins of each
// status level accumulated in FLOAT in index order, bit for bit what the sequential loop gives (an exact parallel form, see
// the file).  A count of -1 at level 0: the device declined (negative / non-finite values, or more than clist_cap marked
// bins) and the caller runs the loop itself.  ws: level_sums_workspace_bytes() laid out for scans up to Lmax_cap; its first
// level_sums_head_bytes(Lmax_cap) bytes zero before the launch.  counter: one arrival counter, zero before and after.
// host_copy: mapped host memory for `out` (2 (2 Lmax + 1) words).
size_t level_sums_head_bytes(int Lmax_cap);
size_t level_sums_workspace_bytes(int64_t nb, int32_t clist_cap, int Lmax_cap);
void launch_level_sums(const float* T, const int32_t* status, int64_t nb, int Lmax, void* ws, int Lmax_cap, int32_t clist_cap, float* out,
                       unsigned int* counter, void* host_copy, hipStream_t stream);

// Dynamic LDS beyond 48 KB has to be allowed per kernel and per device.  Done once per (kernel, device) and for all the CU
// has left next to the kernel's static use: a per-launch setting from several host threads (a pool) would race with the
// other threads' launches.  A failed attribute call is reported (stderr) -- the launch that needed it then fails and the
// pipeline's next wait returns the launch error.
constexpr int kMaxDevices = 16;
void report_attribute_failure(const char* kernel, const char* what);
#define RSI_ALLOW_FULL_LDS(kernel)                                                                                  \
  do {                                                                                                              \
    static std::once_flag once__[rsik::kMaxDevices];                                                                \
    int dev__ = 0;                                                                                                  \
    if (hipGetDevice(&dev__) != hipSuccess || dev__ < 0 || dev__ >= rsik::kMaxDevices) dev__ = 0;                   \
    std::call_once(once__[dev__], [dev__] {                                                                         \
      hipFuncAttributes a__;                                                                                        \
      int lds__ = 0;                                                                                                \
      if (hipFuncGetAttributes(&a__, reinterpret_cast<const void*>(kernel)) != hipSuccess) {                        \
        rsik::report_attribute_failure(#kernel, "hipFuncGetAttributes"); return;                                    \
      }                                                                                                             \
      if (hipDeviceGetAttribute(&lds__, hipDeviceAttributeMaxSharedMemoryPerBlock, dev__) != hipSuccess || lds__ <= 0) \
        lds__ = 160 * 1024;                                                                                         \
      if (hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,   \
                              lds__ - (int)a__.sharedSizeBytes) != hipSuccess)                                      \
        rsik::report_attribute_failure(#kernel, "hipFuncSetAttribute(MaxDynamicSharedMemorySize)");                 \
    });                                                                                                             \
  } while (0)

// ---- candidate stages on the device (kernels_cand.hip) ----
constexpr unsigned kCandHistBins = 16384;   // LDS counters of the per-test quantile histograms
struct EdgeJob {            // optimize_with_derivative for one candidate; start/end updated in place by each launch
  int32_t start, end, type, pad;
};
struct CandJob {            // one isitcnvwrap test, prepared on the host from the candidate list
  int32_t start, end;       // the candidate (compacted coordinates, inclusive)
  int32_t kind;             // 0 DEL, 1 DUP
  int32_t margin;           // int(len*buffer + 1)
  int32_t capacity;         // (int)(chklen*d*2): slots of the neighbourhood array
  int32_t top;              // slot the left side starts filling from (downwards)
  int32_t nleft, nright;    // neighbour intervals the walk may have to jump over, in pointer order
  int32_t left_off, right_off;   // offsets into the chain array (int2 start,end)
  int32_t budget;           // maxchkbp*10: thinning threshold
  int32_t cut;              // bit 0 / 1: the left / right chain was cut short by the host (the kernel reports when it runs out)
  double right_cap;         // 2*chklen*d (the right side appends while used < right_cap)
  int64_t iscratch_off;     // value scratch, in int32 units (a multiple of 4): the pieces of cand_scratch_bytes
  int64_t lscratch_off;     // int64 scratch (one-workgroup form only): capacity + 1 rounded up to a multiple of 4; offset even
};
struct CandOut {
  int32_t flags;            // 1: empty neighbourhood, 2: body value range beyond the LDS histogram, 4: same for the window means, 8: cut chain used up, 16: the left walk ran short where the host had vouched it would not (split form)
  int32_t nref, nbody, nwin, left_reach, right_reach, body_min, body_max;
  double body_q[3], body_s1, body_s2;   // lower quartile / median / upper quartile (partition_stat_tp), sum, sum of squares
  double ref_q[3], ref_s1, ref_s2;      // the same for the window means
};
// The capped, compacted depth as the candidate kernels see it: int32 (bytes = 4) or, behind K4', one byte per base (bytes = 1).
struct DepthRef { const void* p; int bytes; };
void launch_widen_u8(const uint8_t* src, int64_t n, int32_t* dst, hipStream_t stream);   // the int32 form of a byte array
void launch_patch_i32(int32_t* dst, const int32_t* pos, const int32_t* val, int64_t cnt, hipStream_t stream);   // dst[pos[k]] = val[k]
void launch_range_sums(DepthRef rdc, const void* ranges /* int2 lo,hi inclusive */, int nranges, long long* sums, hipStream_t stream);
// one launch = one call of optimize_with_derivative for every job; ws: sharpen_workspace_bytes(ws_jobs) bytes laid out for
// ws_jobs >= njobs jobs, whose first sharpen_workspace_zero_bytes(ws_jobs) are zero before the first launch (each launch
// leaves them zero again, so a workspace is cleared once, when it is allocated).  jobs may be mapped host memory.
void launch_sharpen_edges(DepthRef rdc, int64_t ncompact, EdgeJob* jobs, int njobs, void* ws, int ws_jobs, hipStream_t stream);
size_t sharpen_workspace_bytes(int njobs);
size_t sharpen_workspace_zero_bytes(int njobs);
// How the candidate kernels store the values they gather: one byte each where the depth is bytes (value_bytes = 1), else
// int32 (value_bytes = 4; also allowed for byte depth: RSI_HOT_CAND_BYTES=0).  The value scratch of one test, every piece
// on a 16-byte boundary: top + 1 values (left part), capacity floats (the window means; the one-workgroup form keeps the
// neighbourhood's values there first), min(capacity, budget) values (thinned copy) and, for the split form, capacity
// values more (the right walk's own slots).
inline size_t cand_scratch_bytes(int top, int capacity, int budget, int value_bytes, bool split) {
  auto up16 = [](size_t x) { return (x + 15) & ~size_t(15); };
  const size_t vb = (size_t)value_bytes;
  return up16((size_t)(top + 1 > 0 ? top + 1 : 0) * vb) + up16((size_t)capacity * 4) +
         up16((size_t)(capacity < budget ? capacity : budget) * vb) + (split ? up16((size_t)capacity * vb) : 0);
}
// The same test spread over several workgroups (three launches: the two walks side by side; chunked window means by sliding
// sums + the candidate's statistics; chunked histogram with a last-workgroup fold).  No int64 scratch.  mid: njobs CandMid records, `done`
// zero before the first launch (each launch leaves it zero); ghist: njobs x kCandHistBins counters, zero likewise.
constexpr int kCandChunks = 16;
struct CandMid {
  int32_t lcnt, lreach, lused, rcnt_max, rreach, rused;
  uint32_t done, body_flags;
  float flo[kCandChunks], fhi[kCandChunks];
  double m1[kCandChunks], m2[kCandChunks];
  int32_t body_min, body_max;
  double body_q[3], body_s1, body_s2;
};
void launch_candidate_test_split(DepthRef rdc, int64_t ncompact, const CandJob* jobs, int njobs, const void* chains,
                                 int32_t* iscratch, double RDmedian, CandMid* mid, uint32_t* ghist,
                                 CandOut* outs, int value_bytes, hipStream_t stream);
void launch_candidate_test(DepthRef rdc, int64_t ncompact, const CandJob* jobs, int njobs, const void* chains,
                           int32_t* iscratch, long long* lscratch, double RDmedian, CandOut* outs, int value_bytes, hipStream_t stream);

// ---- depth text ingestion (kernels_io.hip; load_data_from_text's parse loop, loaddata.cpp:496-517) ----
struct TextParseStats { unsigned long long lines, stored, beyond; unsigned int unsorted, pad; };
// One chunk of text that starts on a line start and ends on a line end (or the end of the file).  depth[size] must be
// zeroed before the first chunk.  wg_first / wg_max: text_parse_workgroups(nbytes) entries each (first counted position
// and running maximum per workgroup; -1 = none) for the caller's cross-workgroup order check; stats accumulates.
int text_parse_workgroups(long long nbytes);
void launch_parse_depth_text(const void* text, long long nbytes, long long size, int32_t* depth, long long* wg_first,
                             long long* wg_max, TextParseStats* stats, hipStream_t stream);

// ---- named lines: "RNAME pos depth", every chromosome of a genome in one file (kernels_io.hip) ----
// Boundary pass: every data line (not empty, first byte not '#', a name token after the leading blanks) whose name differs
// from the previous data line's within [0, nbytes) -- the chunk's first data line always -- is one entry, in no particular
// order: {line start, name start, name length}.  count (zeroed by the caller) receives how many there were, also beyond cap.
struct NameBound { long long line; int32_t name, len; };
// bedgraph: data lines are bedGraph ones ("RNAME start end d" whose name is not track / browser and whose end > start).
void launch_text_name_bounds(const void* text, long long nbytes, NameBound* bounds, unsigned int* count, unsigned int cap,
                             hipStream_t stream, bool bedgraph = false);
// Parse pass over [begin, end) of a chunk: the segments' starts ascend, segs[0].start <= begin, nseg <= kMaxGenomeSegs.  Every
// line belongs to the last segment that starts at or before it; a segment without a depth buffer (slot < 0) is skipped.  The
// rest of a line behind its name is read like a "pos depth" line; counts and the order proof go to slots[slot].
struct GenomeSeg { long long start, n; int32_t* depth; int32_t slot, pad; };
struct GenomeSlotStats { unsigned long long lines, stored, beyond; unsigned int unsorted, pad; long long last_pos; /* 0: none yet */ };
constexpr int kMaxGenomeSegs = 512;
// Cohort files, "RNAME pos d1 d2 ... dK": the same pass, storing the selected depth columns.  Sample j of a segment lives at
// depth + j * genome_sample_stride(n) (16-byte aligned starts); a line's column c is what `iss >> pos >> d1 >> ... >> dc`
// leaves in dc (0 once an extraction has failed).  cols: the selected 1-based columns in ascending order, j[i] the sample
// that column col[i] goes to.
constexpr int kMaxGenomeSamples = 64;
struct GenomeSampleCols { int32_t col[kMaxGenomeSamples], j[kMaxGenomeSamples]; int32_t n, pad; };
__host__ __device__ inline long long genome_sample_stride(long long n) { return (n + 4 + 3) & ~3ll; }
// bedGraph files, "RNAME start end d" (DESIGN.md 6d): the same pass over intervals.  A line stands for the lines "RNAME p d",
// p = start + 1 .. end; depth, counts and order proof are what the text format gives on those lines.  Runs longer than
// the parsing thread writes go to `runs` in pieces of at most kBedPiece bases, written by a fill kernel behind the parse;
// *nruns (8 bytes) must be zeroed before each launch.  run_cap: bedgraph_run_cap(chunk bytes, the sum of the chromosomes'
// lengths), enough for any sorted text; a chromosome whose pieces do not fit is marked unsorted (the host loop rebuilds it).
struct BedRun { int32_t* dst; uint32_t len; int32_t d; };
constexpr long long kBedPiece = 1ll << 20;
unsigned long long bedgraph_run_cap(long long text_bytes, long long sum_len);
// What a line behind its name holds: "pos d", "pos d1 ... dK" or "start end d".
enum class GenomeFormat { kText, kSamples, kBedgraph };
// Workgroups of the parse over nbytes of text; the most for kText and kBedgraph (the smaller tile).
int genome_parse_workgroups(GenomeFormat format, long long nbytes);
// The parse of `format`, the order fold behind it and, for kBedgraph, the fill.  wg: 4 * genome_parse_workgroups(format, end -
// begin) words of scratch (per workgroup: first segment, first position, last segment, last position) that the order fold
// reads.  cols is read for kSamples only; runs, nruns and run_cap for kBedgraph only.
void launch_parse_genome(GenomeFormat format, const void* text, long long begin, long long end, const GenomeSeg* segs, int nseg,
                         GenomeSlotStats* slots, long long* wg, const GenomeSampleCols* cols, BedRun* runs, unsigned long long* nruns,
                         unsigned int run_cap, hipStream_t stream);

// ---- BGZF members inflated on the device (kernels_inflate.hip, inflate_core.h) ----
// One member per entry: its deflate payload at comp[coff, coff + clen), its ISIZE bytes to text[out, out + isize) once ISIZE
// and the CRC32 are verified.  isize <= 65536.  last_nl: atomicMax of the offset of the last '\n' written (the caller sets its
// start value); status: atomicMin of (member index << 8 | rsinf::Err) over the bad members (the caller sets it to ~0).
struct InflateBlock { long long coff, out; uint32_t clen, isize, crc, pad; };
void launch_inflate_bgzf(const void* comp, const InflateBlock* blocks, int nblocks, void* text, int* last_nl,
                         unsigned long long* status, hipStream_t stream);
// ---- The reference sequence unfolded (kernels_ref.hip) ----
// span[0, span_len): text of a FASTA file in HBM, its first byte at text offset span_off; span is 16-byte aligned and its buffer
// readable up to span_len rounded up to 16.  L: one sequence's .fai layout (linebases >= 1, linewidth >= linebases, length <
// 2^31 - 4096).  The bases [k0, k1), 0 <= k0 < k1 <= length, whose bytes -- and, behind a base that ends a full line, the
// line's terminator -- lie inside the span (ref_host.h: contained_bases) go to out[k0 .. k1) unchanged, one byte each; out is 16-byte aligned.  flags[0] += the
// terminator positions that hold something other than '\n' or '\r', flags[1] += the base positions that hold '\n', '\r' or '>'
// (or lie outside the span): non-zero means the layout does not fit the text.  A terminator that would lie behind the span (the
// file's last line may lack it) is not looked at.  Launching twice writes the same bytes; no workgroup waits for another.
constexpr int kRefTileBases = 4096;      // bases per workgroup
constexpr int kRefStageBytes = 16896;    // LDS for a tile's text: lines of one base with "\r\n" and a byte to spare still fit
struct RefLayout { long long offset, length; int linebases, linewidth; };
bool ref_unfold_staged(const RefLayout& L);   // the tile's text goes through LDS (else it is picked from HBM byte by byte)
void launch_ref_unfold(const void* span, long long span_off, long long span_len, const RefLayout& L, long long k0, long long k1,
                       void* out, unsigned int* flags, hipStream_t stream);
// Name bytes of the boundary pass's entries bounds[k0, k1) into out[(i - k0) * 256 ...] (at most 255 bytes each).
void launch_gather_names(const void* text, const NameBound* bounds, unsigned k0, unsigned k1, char* out, hipStream_t stream);

// ---- BAM pileup -> depth (kernels_io.hip; load_data_from_bam, loaddata.cpp:277-333 + resolve_cigar_pos, samfunctions.cpp:38-100) ----
struct BamDepthStats { unsigned long long used, runs, malformed; };   // malformed: records whose fields overrun their block_size (skipped)
// One thread per record: data = inflated BAM bytes, rec_off[i] = offset of record i's block_size field.  diff: int32[n + 1], zeroed
// before the first chunk; launch_inclusive_scan_i32 over n turns it into the depth (tile_scratch: scan_tiles(n) ints).
void launch_bam_depth(const void* data, const uint32_t* rec_off, int nrec, int tid, int minq, int min_baseq, long long n, int32_t* diff,
                      BamDepthStats* stats, hipStream_t stream);
int scan_tiles(long long n);
void launch_inclusive_scan_i32(int32_t* x, long long n, int32_t* tile_scratch, hipStream_t stream);

// ---- BAM records found on the device (kernels_bam.hip, bam_walk_core.h) ----
// data[0, len): a chunk of inflated BAM bytes whose byte 0 starts a record, cut into segments of RSI_BAM_SEGMENT bytes.  The three launches, in this order on one stream, leave in rec_off[] the ascending offsets of the whole
// records of `tid` on the chain from 0 -- what launch_bam_depth takes -- and in *report their number and where and why the chain
// stopped.  guess: bam_segments(len) words; out: as many BamSegOut; lists: bam_segments(len) * kBamListCap words; reflen[nref]:
// the header's reference lengths.  The buffer behind data must be readable 3 bytes in front of data and 3 bytes behind data + len
// (the guess stages whole words).
#define RSI_BAM_SEGMENT 16384
constexpr int kBamMaxSegs = 3072;                           // 48 MB: what the loader's buffers (guess, out, lists, rec_off) are laid out for
constexpr int kBamListCap = RSI_BAM_SEGMENT / 36 + 1;       // a record has at least 36 bytes
using BamSegOut = rsibam::SegOut;
using BamFindReport = rsibam::Report;
int bam_segments(long long len);
void launch_bam_guess(const void* data, long long len, int nref, const int32_t* reflen, uint32_t* guess, hipStream_t stream);
void launch_bam_walk(const void* data, long long len, int tid, const uint32_t* guess, BamSegOut* out, uint32_t* lists, hipStream_t stream);
void launch_bam_stitch(const void* data, long long len, int tid, const uint32_t* guess, const BamSegOut* out, uint32_t* lists, uint32_t* rec_off,
                       BamFindReport* report, hipStream_t stream);

// ---- read-pair annotation on the device (kernels_pairs.hip, bam_pairs_core.h) ----
// The pair table: five int32 arrays, entry k = record k of the chromosome in file order (bam_pairs_core.h, Entry).
struct PairTable { int32_t *pos, *rend, *mpos, *isize; uint32_t* info; };
// words[4]: the largest rend - pos, the load flags (rsipairs::LoadFlag), and the last pos of the chunk before, kept in
// words[2 + parity] and left for the next launch in words[2 + (parity ^ 1)]: the launches of a load alternate parity.
constexpr int kPairWords = 4;
// One thread per entry of rec_off[] (what launch_bam_depth takes, same data): entry base + i of the table is written.
void launch_bam_pairs(const void* data, const uint32_t* rec_off, int nrec, int tid, long long base, PairTable t, int32_t* words, int parity,
                      hipStream_t stream);
// The insert-size sample over table[0, n).  ws: pair_sample_workspace_bytes(n) bytes.  out[4] (device, unsigned long long):
// count, sum |isize|, sum of the wrapped squares (two's complement), records kept up to and including the stopping one.
constexpr int kPairSampleTile = 1024;
size_t pair_sample_workspace_bytes(long long n);
void launch_pair_sample(PairTable t, long long n, long long tid_len, void* ws, unsigned long long* out, hipStream_t stream);
// One workgroup per call: calls[ncalls] (rsipairs::Call), out[4 * ncalls]: q0_all, q0_q0, rp, records examined.  The table is
// ascending in pos; maxspan: the largest rend - pos in it.
void launch_pairs_annotate(PairTable t, long long n, int maxspan, const void* calls, int ncalls, int isize_mean, int isize_sd, uint32_t* out,
                           hipStream_t stream);
// What launch_pair_sample leaves in its workspace for the kernels behind it: the stop word (the stopping record's table index,
// 0xffffffff: none) at its start, and every tile's prefix (rsipairs::Seg per tile).
const void* pair_sample_tile_pre(const void* ws, long long n);

// ---- `pin`: the kept CIGARs, the depth sample, one workgroup per breakpoint (kernels_pin.hip, bam_pin_core.h) ----
// Beside the pair table, entry for entry: lq = l_qseq, coff = the read's place in the pool (pool[coff] = n_cigar, then its words).
struct PinTable { int32_t* lq; uint32_t* coff; uint32_t* pool; };
// One thread per entry of rec_off[], beside launch_bam_pairs.  *cursor: the pool words taken so far; a wave takes its reads'
// words with one atomicAdd.  pool_cap: words the pool has room for -- the caller makes it cursor + nrec + (bytes of the chunk) / 4
// at least, which no chunk's CIGARs exceed; a read that would not fit all the same is not copied and *cursor still grows.
// A record whose name and CIGAR overrun its block_size gets n_cigar 0 (the pair kernel flags it; its CIGAR is not read).
void launch_bam_pin(const void* data, const uint32_t* rec_off, int nrec, long long base, PinTable t, unsigned int* cursor, unsigned int pool_cap,
                    hipStream_t stream);
// The depth sample behind launch_pair_sample (same table, n, tid_len and workspace ws).  rdc: kPinRdcWords int32, scan_scratch:
// scan_tiles(kPinRdcWords) ints.  Afterwards rdc[0, 1 001 000) holds the sample's rd, each read counted at its own stretch's
// offset, and *state (rsipin::SampleState, device) what the loop leaves behind.
constexpr int kPinRdcWords = 1001000 + 8;
void launch_pin_sample(PairTable t, PinTable p, long long n, long long tid_len, const void* ws, int32_t* rdc, int32_t* scan_scratch, void* state,
                       hipStream_t stream);
// drd[k] for k in [lo, hi) of the sample's last stretch (rsipin::sample_drd)
void launch_pin_sample_drd(const int32_t* rdc, int32_t* drd, int lo, int hi, int l_qseq, hipStream_t stream);
// One workgroup per breakpoint: bps[nbp] (rsipin::Bp), out[2 * nbp]: i_max (-1: none) and the clip count there.  3 (2 r_len + 1)
// counters in LDS: r_len <= kPinMaxRlen.
constexpr int kPinMaxRlen = 2559;
void launch_pin_windows(PairTable t, PinTable p, long long n, int maxspan, long long tid_len, const void* bps, int nbp, int r_len, int l_qseq,
                        double drd_sd, int32_t* out, hipStream_t stream);

// ---- `geno`: quantiles, count, sum, minimum and maximum of ranges of the compacted depth (kernels_geno.hip) ----
// A job is one statistic over the values of its tiles; a tile (rsigeno::Tile's layout, geno_host.h) is `len` consecutive values
// from `off` on, inside the array -- the caller checks that.  hist: geno_hist_bytes() bytes, all zero before the first launch.
// Bytes: launch_geno_hist8 (a workgroup per tile), then launch_geno_scan8 (a workgroup per job) writes out[job].
// int32: launch_geno_init32, _minmax32, _plan32 -- which finishes empty and all-equal jobs and leaves in *maxbits the widest
// max - min of the others, in bits -- then ceil(*maxbits / kGenoBits) times launch_geno_hist32 + launch_geno_scan32; the scan of
// a job's last pass writes out[job] and every scan leaves the job's histogram zero.
struct GenoTile { int32_t job, off, len, pad; };
struct GenoOut { int32_t n, vmin, vmax, q[3]; long long sum; };
struct GenoState { int32_t vmin, vmax; unsigned int n; int32_t shift; unsigned long long sum; uint32_t prefix[3], k[3]; };
constexpr int kGenoThreads = 256, kGenoBits = 11, kGenoBins = 1 << kGenoBits;
size_t geno_hist_bytes(int storage, int64_t njobs);
void launch_geno_hist8(const uint8_t* d, const GenoTile* tiles, int ntiles, unsigned int* hist, hipStream_t stream);
void launch_geno_scan8(const unsigned int* hist, int njobs, GenoOut* out, hipStream_t stream);
void launch_geno_init32(GenoState* st, int njobs, unsigned int* maxbits, hipStream_t stream);
void launch_geno_minmax32(const int32_t* d, const GenoTile* tiles, int ntiles, GenoState* st, hipStream_t stream);
void launch_geno_plan32(GenoState* st, int njobs, GenoOut* out, unsigned int* maxbits, hipStream_t stream);
void launch_geno_hist32(const int32_t* d, const GenoTile* tiles, int ntiles, const GenoState* st, unsigned int* hist, hipStream_t stream);
void launch_geno_scan32(GenoState* st, int njobs, unsigned int* hist, GenoOut* out, hipStream_t stream);

// ---- plot data: the running mean's window sums and the queried values of planned figures (kernels_plot.hip) ----
// A job is one figure's neighbourhood: la values from a0 on, then lb values from b0 on, all inside the array (the caller checks
// that), cut into tiles of `tile` values (1 <= tile <= kPlotMaxTile) of that concatenation; tile0 is the job's first tile in the
// batch's numbering (ascending over the jobs, every job has at least one value).  Its queries start at q0: nq0 rows of block 0, nq1
// of block 1, nq2 of block 2, the two of block 3.  qref[q]: neighbourhood index of the window's centre before the clamp, in
// [0, la + lb), or -1 for no window; inside blocks 0 and 2 it is never -1 and never descends.  Per batch: launch_plot_tile_sums
// (a workgroup per tile: tsum[tile]), launch_plot_tile_scan (a workgroup per job: tsum becomes the sum in front of each tile),
// launch_plot_window_ends (a workgroup per tile scans its values in LDS and writes the prefix sum at every window end that falls
// into the tile: ends[2 q] at the window's last value, ends[2 q + 1] at the value in front of its first; `ends` all zero before),
// launch_plot_gather (a thread per query: value[q] = d[qdepth[q]] or 0 for -1, wsum[q] = ends[2 q] - ends[2 q + 1]).  The kernel
// boundary is the only synchronisation between workgroups; all sums are exact in 64 bits.
struct PlotJob { int32_t a0, la, b0, lb, band, nq0, nq1, nq2; long long q0; int32_t tile0, pad; };
constexpr int kPlotThreads = 256, kPlotMaxTile = 4096, kPlotDefaultTile = 2048;
void launch_plot_tile_sums(const int32_t* d, const PlotJob* jobs, int njobs, int ntiles, int tile, long long* tsum, hipStream_t stream);
void launch_plot_tile_scan(const PlotJob* jobs, int njobs, int tile, long long* tsum, hipStream_t stream);
void launch_plot_window_ends(const int32_t* d, const PlotJob* jobs, int njobs, int ntiles, int tile, const long long* tsum, const int32_t* qref,
                             long long* ends, hipStream_t stream);
void launch_plot_gather(const int32_t* d, const int32_t* qdepth, const int32_t* qref, const long long* ends, long long nq, int32_t* value,
                        long long* wsum, hipStream_t stream);
// expand_data (loaddata.cpp:140-183) on the device: out[n] = the compacted array src (storage 1: bytes, 4: int32) with the removed
// regions back in as zeros.  starts / ends: npairs inclusive pairs, ascending and disjoint; before[k]: removed values in front of
// pair k.  The caller has checked that the pairs lie inside [0, n) and that n minus their lengths is the compacted length.
void launch_plot_expand(const void* src, int storage, const int32_t* starts, const int32_t* ends, const long long* before, int npairs, int32_t* out,
                        long long n, hipStream_t stream);

// ---- `depth`: a chromosome's per-base depth int32[n] summed up without a run (kernels_depth.hip) ----
// launch_depth_summary: one pass, a workgroup per `span` values.  acc: vmin = INT32_MAX, vmax = INT32_MIN and zeros before the
// launch; dist: kDepthBins zeros.  After it acc holds the exact sum, minimum and maximum of the non-negative depths, how many lie
// above 65535 (counted in bin 65535) and how many are negative (counted nowhere else: they index nothing).
struct DepthAcc { unsigned long long sum, over, negative; int32_t vmin, vmax; };
constexpr int kDepthThreads = 256, kDepthBins = 65536;
constexpr int kDepthSplit = 512, kDepthCopies = 16;   // depths below the split are counted in LDS, in so many counters per value
constexpr long long kDepthSpan = 1ll << 17;            // values per workgroup
void launch_depth_summary(const int32_t* d, long long n, long long span, DepthAcc* acc, unsigned int* dist, hipStream_t stream);
// Windows [k W, min((k + 1) W, n)) for k in [w0, w1), a slice: launch_depth_window_table writes start[k - w0], end[k - w0] and
// clears sum[k - w0]; launch_depth_windows adds every window's depths into sum[k - w0], exact in 64 bits, a workgroup per `span`
// bases of the slice (1 <= span <= kWindowSpan; W need not divide it, and may exceed it).  W >= 1, w1 <= ceil(n / W).
constexpr int kWindowSpan = 4096;
void launch_depth_window_table(long long w0, long long w1, long long W, long long n, long long* start, long long* end, unsigned long long* sum,
                               hipStream_t stream);
void launch_depth_windows(const int32_t* d, long long n, long long W, long long w0, long long w1, int span, unsigned long long* sum,
                          hipStream_t stream);

// ---- depth track: an int32 array as bedGraph text, run-length encoded and formatted on the device (kernels_track.hip) ----
// One line "NAME \t pos0+start \t pos0+end \t value \n" per maximal run of equal values of v[0, n), worked through in slices
// [b, e) of bases.  A run start is i == 0 or v[i] != v[i - 1] -- read from the whole array, so slicing moves no start.  A line is
// written by the slice that sees its END: the start of the last run seen so far stays open in TrackState::carry and becomes the
// first entry of the next slice's start list; the last slice (e == n) closes it with n.  Per slice: launch_track_starts, then
// launch_track_line_bytes, then -- once the host has read the state's nlines / nbytes and checked them against its buffers --
// launch_track_format.
struct TrackState {
  long long carry;     // start of the open run (index into v), -1 before the first slice
  long long nstarts;   // entries of starts[] for this slice, the carried one included (the closing n not)
  long long nlines;    // lines this slice writes
  long long nbytes;    // their bytes
  long long packed;    // BGZF: bytes of the last slice's packed members (k_bgzf_pack; read with the next slice's numbers)
  long long stored;    // BGZF: how many of them are one stored block
};
struct TrackName { char s[256]; int len; };   // the chromosome name, at most 255 bytes, travels with the kernel arguments
constexpr int kTrackTile = 256;               // bases (passes 1-3) or lines (passes 4-5) per workgroup
__host__ __device__ inline int track_tiles(long long count) { return (int)((count + kTrackTile - 1) / kTrackTile); }
// Passes 1-3: run starts of [b, e) flagged and counted per tile, the tile counts scanned (one workgroup), the starts
// scattered to starts[] behind the carried one.  tiles: track_tiles(e - b) + 1 words; starts: e - b + 2 entries; e - b > 0.
void launch_track_starts(const int32_t* v, long long b, long long e, long long n, unsigned int* tiles, long long* starts, TrackState* st,
                         hipStream_t stream);
// Pass 4: every line's byte length from digit counts, summed per tile of lines and scanned (one workgroup): st->nbytes, and
// st->carry for the next slice.  max_lines: e - b + 1 (the grid; workgroups beyond st->nlines leave at once); ltiles:
// track_tiles(max_lines) + 1 words.
void launch_track_line_bytes(const int32_t* v, const long long* starts, TrackState* st, long long pos0, int name_len, long long max_lines,
                             unsigned int* ltiles, hipStream_t stream);
// Pass 5: line j of nlines at its byte offset in text[0, cap); a line that would pass cap is not written.
void launch_track_format(const int32_t* v, const long long* starts, const unsigned int* ltiles, long long nlines, long long pos0,
                         const TrackName& name, char* text, long long cap, hipStream_t stream);

// ---- per-bin track: one value per bin as bedGraph text, a line per piece of a bin (kernels_track.hip) ----
// Bin b holds the compacted positions [b m, (b + 1) m), mapped back through the removed-region table (cbreak[nreg], cum[nreg + 1],
// in HBM); it is cut where a removed region lies strictly inside it.  Slices are ranges of bins [b0, b1); a piece belongs to the
// slice of its bin, so no state passes from slice to slice.  pieces: one 8-byte word per piece, (bin - b0) << 16 | region index.
struct BinTrackSource {
  const int32_t* v;                 // value of every bin of the chromosome
  const unsigned long long* pieces;
  const long long* cbreak; const long long* cum;
  int nreg, m;
  long long b0;                     // the slice's first bin
  int which;                        // 0: the value as %d; 1: value / (median2 / 2) with three decimals, rounded half up
  long long median2;                // > 0 when which == 1
};
// Passes 1-3: pieces counted per tile of bins, the tile counts scanned, the pieces scattered (none at or beyond cap); st->nlines.
// tiles: track_tiles(b1 - b0) + 1 words; b1 - b0 > 0.
void launch_bintrack_pieces(const long long* cbreak, const long long* cum, int nreg, int m, long long b0, long long b1, unsigned int* tiles,
                            unsigned long long* pieces, long long cap, TrackState* st, hipStream_t stream);
// Passes 4 and 5 of the depth track on the pieces: max_lines bounds the grid as there; ltiles: track_tiles(max_lines) + 1 words.
void launch_bintrack_line_bytes(const BinTrackSource& src, TrackState* st, int name_len, long long max_lines, unsigned int* ltiles,
                                hipStream_t stream);
void launch_bintrack_format(const BinTrackSource& src, const unsigned int* ltiles, long long nlines, const TrackName& name, char* text,
                            long long cap, hipStream_t stream);

// ---- region lines: "NAME \t pos0+start \t pos0+end \t mean \n" from (start, end, sum) triples in HBM (kernels_track.hip) ----
// One line per triple of a slice, in order; windows (-by W) and BED regions (-by FILE) both come as triples.  The mean is
// sum / (end - start) with two decimals, rounded half up in integers: a = S / L, r = S mod L, hundredths (200 r + L) / (2 L), a
// hundred of them carrying into a; 0.00 when end <= start or the sum is not positive.  No state passes from slice to slice.
struct RegionTrackSource { const long long* start; const long long* end; const long long* sum; };
// st for a slice of nlines lines, then passes 4 and 5 of the depth track on the triples (ltiles: track_tiles(nlines) + 1 words)
void launch_regiontrack_line_bytes(const RegionTrackSource& src, TrackState* st, long long nlines, long long pos0, int name_len,
                                   unsigned int* ltiles, hipStream_t stream);
void launch_regiontrack_format(const RegionTrackSource& src, const unsigned int* ltiles, long long nlines, long long pos0, const TrackName& name,
                               char* text, long long cap, hipStream_t stream);


// ---- BGZF tracks: a slice's text deflated member by member (kernels_deflate.hip, deflate_core.h) ----
constexpr unsigned int kDeflateMemberText = 65280;   // text bytes of a member (the last of a slice may hold fewer)
constexpr unsigned int kDeflateSlotBytes = 65536;    // where a member is left: header, payload, footer from the slot's start
inline int deflate_members(long long nbytes) { return nbytes <= 0 ? 0 : (int)((nbytes + kDeflateMemberText - 1) / kDeflateMemberText); }
// text[0, nbytes) (256-byte aligned) -> member k, a whole BGZF member of text[k * 65280 ...], at slots[k * 65536 ...]; sizes[k]: its
// bytes, bit 31 set when it is one stored block.  The bytes are a function of the text alone.
void launch_deflate_bgzf(const void* text, long long nbytes, void* slots, unsigned int* sizes, hipStream_t stream);
// The members back to back in packed[0, cap); st->packed: their bytes (nothing is copied past cap; the sum says so), st->stored.
void launch_bgzf_pack(const void* slots, const unsigned int* sizes, int nmembers, void* packed, long long cap, TrackState* st,
                      hipStream_t stream);

// ---- the tabix index of a BGZF track: a slice's chunk starts and window starts (kernels_track.hip) ----
// Run behind a slice's deflate and pack launches.  Line j of the slice (0-based half-open [s, e), e' = e - 1) lies at text offset t
// (the ltiles prefix plus the scan of the line lengths, as in the format pass); its virtual offset, relative to the slice's first
// packed byte, is (sum of sizes[0, t / 65280)) << 16 | t % 65280.  Two record lists, each gathered workgroup by workgroup behind an
// atomic counter (in line order inside a workgroup; the host sorts by voff, which is unique per line):
//   chunk starts  {voff, a = reg2bin(s, e)}:       j == 0 or the bin differs from line j - 1's
//   window starts {voff, a = w_first, b = w_last}: j == 0 (w_first = s >> 14: the host knows how far the slices before reached) or
//                                                  e'_j >> 14 > e'_(j-1) >> 14, w_first = max(s_j >> 14, (e'_(j-1) >> 14) + 1)
// with w_last = e'_j >> 14.  A count above its capacity says that records are missing: nothing is written past a capacity.
struct TrackIndexRec { unsigned long long voff; unsigned int a, b; };
struct TrackIndexHead { unsigned int nchunk, nwin, bad, pad; };   // bad: more members than the kernel's LDS table holds
constexpr int kTrackIndexMembers = 515;                            // members of a slice at most (track_host.h: kMaxMembers)
// One allocation per slice: the head, chunk_cap chunk records, win_cap window records
struct TrackIndexOut { TrackIndexHead* head; TrackIndexRec* chunks; unsigned int chunk_cap; TrackIndexRec* wins; unsigned int win_cap; };
inline size_t track_index_bytes(unsigned int chunk_cap, unsigned int win_cap) {
  return sizeof(TrackIndexHead) + ((size_t)chunk_cap + win_cap) * sizeof(TrackIndexRec);
}
inline TrackIndexOut track_index_out(void* base, unsigned int chunk_cap, unsigned int win_cap) {
  TrackIndexRec* r = reinterpret_cast<TrackIndexRec*>(static_cast<char*>(base) + sizeof(TrackIndexHead));
  return TrackIndexOut{static_cast<TrackIndexHead*>(base), r, chunk_cap, r + chunk_cap, win_cap};
}
// out.head zeroed by the caller on the same stream; nlines > 0; pos0 >= 0
void launch_track_index(const int32_t* v, const long long* starts, const unsigned int* ltiles, long long nlines, long long pos0, int name_len,
                        const unsigned int* sizes, int nmembers, const TrackIndexOut& out, hipStream_t stream);
void launch_bintrack_index(const BinTrackSource& src, const unsigned int* ltiles, long long nlines, int name_len, const unsigned int* sizes,
                           int nmembers, const TrackIndexOut& out, hipStream_t stream);

}  // namespace rsik
