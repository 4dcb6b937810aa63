// kernels_io.hip -- depth text ingestion on the device.  The reference's loader
// (load_data_from_text, loaddata.cpp:496-517) reads "pos depth" lines with getline + istringstream:
// about 65 % of its wall time on the -d path.  Here the file's bytes are streamed to HBM in pinned
// chunks and parsed by one kernel at memory speed.
//
// Reference semantics kept: empty lines and lines starting with '#' are skipped; `iss >> pos >> d` with libstdc++'s
// extraction (text_rules.h: leading blanks, optional sign, digits; no digit gives 0, a value outside int the clamped
// bound, and either failure leaves d at 0; an overflowing pos is therefore INT_MIN, skipped, or INT_MAX, beyond the
// end); pos < 1 skipped; reading
// STOPS at the first pos >= size (the last base is never set, App. A Q7); RD[pos-1] = d, later lines
// overwrite earlier ones.  The last two rules are order-dependent, so the kernel also proves that
// positions are strictly increasing through the file (true for any samtools-depth style file): then
// "stop at the first pos >= size" equals "ignore every pos >= size" and no position is written twice.
// When the proof fails the caller falls back to the sequential host parser (same semantics, slower).
#include "kernels.h"
#include "text_rules.h"

namespace rsik {

namespace {

constexpr int kThreads = 256;
constexpr int kSpan = 32;                      // bytes of text per thread: the lines that START in them are the thread's
constexpr int kTile = kThreads * kSpan;        // 8 KB of text per workgroup

using rsitxt::is_blank;
using rsitxt::extract_i32;   // `iss >> v` into an int: pos, d and the cohort columns
using rsitxt::extract_i64;   // into a long long: bedGraph start and end

__global__ __launch_bounds__(kThreads) void k_parse_depth_text(const unsigned char* __restrict__ text, long long nbytes,
                                                              long long size, int32_t* __restrict__ depth,
                                                              long long* __restrict__ wg_first, long long* __restrict__ wg_max,
                                                              TextParseStats* __restrict__ stats) {
  __shared__ long long s_first[kThreads], s_max[kThreads];
  __shared__ int s_bad;
  if (threadIdx.x == 0) s_bad = 0;
  const long long b0 = ((long long)blockIdx.x * kThreads + threadIdx.x) * kSpan;
  long long first = -1, last = -1;     // positions of the thread's first / latest counted line (pos >= 1)
  unsigned lines = 0, stored = 0, beyond = 0;
  bool sorted = true;
  if (b0 < nbytes) {
    const long long b1 = b0 + kSpan < nbytes ? b0 + kSpan : nbytes;
    for (long long s = b0; s < b1; ++s) {
      if (s != 0 && text[s - 1] != '\n') continue;          // not a line start (the chunk itself starts on one)
      long long e = s;
      while (e < nbytes && text[e] != '\n') ++e;              // lines are short; they may run past the span
      if (e == s || text[s] == '#') continue;
      long long q = s, pos = 0, d = 0;
      if (extract_i32(text, q, e, pos)) extract_i32(text, q, e, d);   // a failed pos (0 or clamped) leaves d at 0
      if (pos < 1) continue;
      ++lines;
      if (last >= 0 && pos <= last) sorted = false;
      if (first < 0) first = pos;
      last = pos;
      if (pos >= size) { ++beyond; continue; }
      depth[pos - 1] = (int32_t)d;
      ++stored;
    }
  }
  // ---- strictly increasing across the threads of the workgroup: running maximum of `last` ----
  s_first[threadIdx.x] = first;
  s_max[threadIdx.x] = last;
  __syncthreads();
  if (threadIdx.x == 0) {
    long long run = -1, wfirst = -1;
    bool ok = true;
    for (int t = 0; t < kThreads; ++t) {
      if (s_first[t] < 0) continue;
      if (wfirst < 0) wfirst = s_first[t];
      if (run >= 0 && s_first[t] <= run) ok = false;
      run = s_max[t] > run ? s_max[t] : run;
    }
    wg_first[blockIdx.x] = wfirst;
    wg_max[blockIdx.x] = run;
    if (!ok) s_bad = 1;
  }
  if (!sorted) atomicOr(&s_bad, 1);
  __syncthreads();
  // ---- totals ----
  for (int d = 32; d >= 1; d >>= 1) { lines += __shfl_xor(lines, d); stored += __shfl_xor(stored, d); beyond += __shfl_xor(beyond, d); }
  // one set of atomics per workgroup (they all land on the same three words and serialise there)
  __shared__ int s_tot[kThreads / 64][3];
  if ((threadIdx.x & 63) == 0) { s_tot[threadIdx.x >> 6][0] = (int)lines; s_tot[threadIdx.x >> 6][1] = (int)stored; s_tot[threadIdx.x >> 6][2] = (int)beyond; }
  __syncthreads();
  if (threadIdx.x == 0) {
    long long t0 = 0, t1 = 0, t2 = 0;
    for (int w = 0; w < kThreads / 64; ++w) { t0 += s_tot[w][0]; t1 += s_tot[w][1]; t2 += s_tot[w][2]; }
    if (t0) atomicAdd(&stats->lines, (unsigned long long)t0);
    if (t1) atomicAdd(&stats->stored, (unsigned long long)t1);
    if (t2) atomicAdd(&stats->beyond, (unsigned long long)t2);
    if (s_bad) atomicOr(&stats->unsorted, 1u);
  }
}

// ---- named lines (whole-genome files): "RNAME pos depth" ----
// A data line is a line that is not empty, does not start with '#' and has a name token: leading blanks, then the bytes up to
// the next blank.  What follows the name is read exactly like a "pos depth" line above, so that every chromosome's lines give
// what its slice (the same lines without the name) gives through k_parse_depth_text.

// The line that starts at s: its end e (a '\n' or `lim`) and its name token [ns, ne); ns == ne when it is no data line.
__device__ inline void line_name(const unsigned char* __restrict__ t, long long s, long long lim, long long& e, long long& ns, long long& ne) {
  e = s;
  while (e < lim && t[e] != '\n') ++e;
  ns = ne = s;
  if (e == s || t[s] == '#') return;
  long long q = s;
  while (q < e && is_blank(t[q])) ++q;
  ns = q;
  while (q < e && !is_blank(t[q])) ++q;
  ne = q;
}

// bedGraph files, "RNAME start end depth": a line is a data line when its name token is not "track" or "browser"
// (the format's header lines) and it stands for at least one "RNAME p depth" line, i.e. start and end parse and end > start.
// The lines that stand for none are no lines of the expanded file, so they neither open nor interrupt a chromosome.
__device__ inline bool is_word(const unsigned char* __restrict__ t, long long ns, long long ne, const char* w, int wl) {
  if (ne - ns != wl) return false;
  for (int k = 0; k < wl; ++k) if (t[ns + k] != (unsigned char)w[k]) return false;
  return true;
}
template <bool kBed>
__device__ inline void data_line(const unsigned char* __restrict__ t, long long s, long long lim, long long& e, long long& ns, long long& ne) {
  line_name(t, s, lim, e, ns, ne);
  if (!kBed || ns == ne) return;
  long long q = ne, a = 0, b = 0;
  if (is_word(t, ns, ne, "track", 5) || is_word(t, ns, ne, "browser", 7) || !extract_i64(t, q, e, a) || !extract_i64(t, q, e, b) || b <= a) ne = ns;
}

__device__ inline bool same_name(const unsigned char* __restrict__ t, long long a, long long alen, long long b, long long blen) {
  if (alen != blen) return false;
  for (long long k = 0; k < alen; ++k) if (t[a + k] != t[b + k]) return false;
  return true;
}

// Boundary pass: one entry per data line whose name is not the previous data line's.  A thread compares the first data line
// of its span with the data line before it (walking back over comment and empty lines: each such stretch is walked by one
// thread only), the others with the thread's own previous one.
// kBed: bedGraph data lines (data_line above); the text files' instantiation is kBed = false.
template <bool kBed>
__global__ __launch_bounds__(kThreads) void k_text_name_bounds(const unsigned char* __restrict__ text, long long nbytes,
                                                               NameBound* __restrict__ bounds, unsigned int* __restrict__ count,
                                                               unsigned int cap) {
  const long long b0 = ((long long)blockIdx.x * kThreads + threadIdx.x) * kSpan;
  if (b0 >= nbytes) return;
  const long long b1 = b0 + kSpan < nbytes ? b0 + kSpan : nbytes;
  long long pns = -1, pne = -1;   // name of the previous data line, once known
  for (long long s = b0; s < b1; ++s) {
    if (s != 0 && text[s - 1] != '\n') continue;
    long long e, ns, ne;
    data_line<kBed>(text, s, nbytes, e, ns, ne);
    if (ns == ne) continue;
    if (pns < 0) {   // first data line of the span: find the data line in front of it
      long long p = s;
      while (p > 0) {
        long long ls = p - 1;                              // text[p - 1] is the '\n' that ends the line before
        while (ls > 0 && text[ls - 1] != '\n') --ls;
        long long e2, ns2, ne2;
        data_line<kBed>(text, ls, p - 1, e2, ns2, ne2);
        if (ns2 != ne2) { pns = ns2; pne = ne2; break; }
        p = ls;
      }
    }
    if (pns < 0 || !same_name(text, pns, pne - pns, ns, ne - ns)) {
      const unsigned int k = atomicAdd(count, 1u);
      if (k < cap) bounds[k] = NameBound{s, (int32_t)ns, (int32_t)(ne - ns)};
    }
    pns = ns; pne = ne;
  }
}

// Across the workgroups of one parse launch: a workgroup's first counted line against the last one of the nearest workgroup
// before it that counted any (same segment only); the launch's first counted line against its chromosome's last position so
// far; the launch's last counted line becomes its chromosome's last position.  One workgroup.
__global__ __launch_bounds__(kThreads) void k_genome_order_fold(const long long* __restrict__ wg, int nwg, const GenomeSeg* __restrict__ segs,
                                                                GenomeSlotStats* __restrict__ slots) {
  __shared__ int s_first, s_last;
  if (threadIdx.x == 0) { s_first = 0x7fffffff; s_last = -1; }
  __syncthreads();
  for (int w = threadIdx.x; w < nwg; w += kThreads) {
    if (wg[4 * (long long)w] < 0) continue;
    atomicMin(&s_first, w); atomicMax(&s_last, w);
    int p = w - 1;
    while (p >= 0 && wg[4 * (long long)p] < 0) --p;
    if (p >= 0 && wg[4 * (long long)p + 2] == wg[4 * (long long)w] && wg[4 * (long long)w + 1] <= wg[4 * (long long)p + 3])
      atomicOr(&slots[segs[wg[4 * (long long)w]].slot].unsorted, 1u);
  }
  __syncthreads();
  if (threadIdx.x == 0 && s_last >= 0) {
    GenomeSlotStats* F = &slots[segs[wg[4 * (long long)s_first]].slot];
    if (F->last_pos > 0 && wg[4 * (long long)s_first + 1] <= F->last_pos) F->unsorted = 1u;
    slots[segs[wg[4 * (long long)s_last + 2]].slot].last_pos = wg[4 * (long long)s_last + 3];
  }
}

// ---- parse pass: one skeleton, k_parse_genome<Format>, and per format what one data line means ----
// A Format gives kSpan (bytes of text per thread: the lines that START in them are the thread's), Count (the type of the
// per-thread and per-workgroup counters), Args (its own kernel arguments, by value), Shared (its LDS, filled by stage() before
// the first barrier), header() (name tokens that name no chromosome; tested before the segment lookup) and the line rule:
//   counted(): is the line's tail [ne, e) a counted line?  Then L holds its first and last position (the order record; it
//              counts last - first + 1 positions) and what store() needs of the line.
//   store():   the writes; it returns how many of the counted positions are stored, the others lie beyond the chromosome's end.
// Between the two the skeleton moves the counters to the line's segment and extends the order record.

// "NAME pos d", read like k_parse_depth_text's "pos d".
struct TextLines {
  static constexpr int kSpan = rsik::kSpan;
  using Count = unsigned;
  struct Args {};
  struct Shared {};
  struct Line { long long first, last, d; };
  static __device__ void stage(const Args&, Shared&) {}
  static __device__ bool header(const unsigned char*, long long, long long) { return false; }
  static __device__ __forceinline__ bool counted(const unsigned char* __restrict__ t, long long ne, long long e, Line& L) {
    long long q = ne, pos = 0;
    L.d = 0;
    if (extract_i32(t, q, e, pos)) extract_i32(t, q, e, L.d);
    L.first = L.last = pos;
    return pos >= 1;
  }
  static __device__ __forceinline__ Count store(const unsigned char* __restrict__, long long, const GenomeSeg& G, const Line& L, const Args&,
                                                const Shared&, bool&) {
    if (L.first >= G.n) return 0;
    G.depth[L.first - 1] = (int32_t)L.d;
    return 1;
  }
};

// Cohort files, "NAME pos d1 ... dK": per counted line below the chromosome's end, the depth tokens are read in
// order up to the largest selected column and every selected one is stored to its sample's array.  A line is 15-20 bytes plus
// 3-4 per sample, so a thread takes 128 bytes of text: with 32-byte spans most threads of a wave would find no line start
// while a few walk a whole line.
struct SampleLines {
  static constexpr int kSpan = 128;
  using Count = unsigned;
  using Args = GenomeSampleCols;
  struct Shared { int col[kMaxGenomeSamples], j[kMaxGenomeSamples]; };
  struct Line { long long first, last, q; bool ok; };
  static __device__ void stage(const Args& cols, Shared& sh) {
    if (threadIdx.x < kMaxGenomeSamples) { sh.col[threadIdx.x] = cols.col[threadIdx.x]; sh.j[threadIdx.x] = cols.j[threadIdx.x]; }
  }
  static __device__ bool header(const unsigned char*, long long, long long) { return false; }
  static __device__ __forceinline__ bool counted(const unsigned char* __restrict__ t, long long ne, long long e, Line& L) {
    long long pos = 0;
    L.q = ne;
    L.ok = extract_i32(t, L.q, e, pos);
    L.first = L.last = pos;
    return pos >= 1;
  }
  static __device__ __forceinline__ Count store(const unsigned char* __restrict__ t, long long e, const GenomeSeg& G, const Line& L,
                                                const Args& cols, const Shared& sh, bool&) {
    if (L.first >= G.n) return 0;
    int32_t* out = G.depth + (L.first - 1);
    const long long stride = genome_sample_stride(G.n);
    // Column c is what its own extraction gives (the clamped bound included) while every extraction before it succeeded,
    // 0 after a failed one.  (pos < n here, so pos did not overflow and ok holds.)
    long long q = L.q, v = 0;
    bool ok = L.ok;
    int col = 1;                     // the next depth column to extract
    for (int i = 0; i < cols.n; ++i) {
      const int want = sh.col[i];
      while (col <= want) { v = 0; if (ok) ok = extract_i32(t, q, e, v); ++col; }
      out[(long long)sh.j[i] * stride] = (int32_t)v;
    }
    return 1;
  }
};

// bedGraph files: a line "NAME start end d" stands for "NAME p d", p = start + 1 .. end; with a = max(start, 0)
// and b = end its counted positions are a + 1 .. b: lines += b - a, those >= n are beyond, the others are stored at indices
// [a, min(b, n - 1)).  The proof is the text one with first = a + 1 and last = b per line.  One line may stand for 2^31
// positions, so the counters are 64-bit.
// Writes: a run of at most kBedInline bases is written by the thread that parsed it, a longer one goes to the run list in
// pieces of at most kBedPiece bases that k_bedgraph_fill writes, one workgroup per piece.  d == 0 writes nothing: the buffer
// was cleared when the chromosome opened and, once the order proof holds, no base is written twice (a chromosome whose proof
// fails, or whose pieces do not fit the list, is rebuilt on the host from a cleared buffer).
constexpr int kBedInline = 128;

struct BedLines {
  static constexpr int kSpan = rsik::kSpan;
  using Count = unsigned long long;
  struct Args { BedRun* __restrict__ runs; unsigned long long* __restrict__ nruns; unsigned int run_cap; };
  struct Shared {};
  struct Line { long long first, last, d; };
  static __device__ void stage(const Args&, Shared&) {}
  static __device__ bool header(const unsigned char* __restrict__ t, long long ns, long long ne) {
    return is_word(t, ns, ne, "track", 5) || is_word(t, ns, ne, "browser", 7);
  }
  static __device__ __forceinline__ bool counted(const unsigned char* __restrict__ t, long long ne, long long e, Line& L) {
    long long q = ne, start = 0, stop = 0;
    if (!extract_i64(t, q, e, start) || !extract_i64(t, q, e, stop)) return false;   // overflow included: no line
    L.d = 0;
    extract_i32(t, q, e, L.d);
    const long long a = start > 0 ? start : 0;
    L.first = a + 1; L.last = stop;
    return stop > a;                   // else no position >= 1
  }
  static __device__ __forceinline__ Count store(const unsigned char* __restrict__, long long, const GenomeSeg& G, const Line& L, const Args& A,
                                                const Shared&, bool& bad) {
    const long long a = L.first - 1, b = L.last;
    const long long edge = G.n - 1;  // positions >= n: beyond; the last base is never set
    const long long hi = b < edge ? b : edge;
    if (hi <= a) return 0;
    const Count stored = (Count)(hi - a);
    if (L.d == 0) return stored;
    const int32_t v = (int32_t)L.d;
    if (hi - a <= kBedInline) {
      for (long long i = a; i < hi; ++i) G.depth[i] = v;
      return stored;
    }
    const long long np = (hi - a + kBedPiece - 1) / kBedPiece;   // <= 2^31 / kBedPiece
    const unsigned long long k = atomicAdd(A.nruns, (unsigned long long)np);
    if (k + (unsigned long long)np > A.run_cap) {
      // No room: the chromosome goes to the host loop.  The entries of [k, k + np) below run_cap are this thread's alone
      // (the reservations are disjoint) and k_bedgraph_fill reads every entry below min(*nruns, run_cap), so each of them
      // gets an empty piece: the fill never sees an entry nobody wrote in this launch.
      bad = true;
      for (unsigned long long r = k; r < A.run_cap && r < k + (unsigned long long)np; ++r) A.runs[r] = BedRun{nullptr, 0u, 0};
      return stored;
    }
    for (long long j = 0; j < np; ++j) {
      const long long p0 = a + j * kBedPiece, len = hi - p0 < kBedPiece ? hi - p0 : kBedPiece;
      A.runs[k + (unsigned long long)j] = BedRun{G.depth + p0, (uint32_t)len, v};
    }
    return stored;
  }
};

// The skeleton.  The order proof of k_parse_depth_text, per chromosome: within a thread, within a workgroup (thread 0 over the
// threads' first and last counted lines), then k_genome_order_fold across the workgroups and against the chromosome's last
// position in the chunks before.  Counts go out with one set of atomics per workgroup when the workgroup's lines end in one
// segment (the common case: a chromosome is millions of lines), per thread otherwise.
template <class F>
__global__ __launch_bounds__(kThreads) void k_parse_genome(const unsigned char* __restrict__ text, long long begin, long long end,
                                                           const GenomeSeg* __restrict__ segs, int nseg,
                                                           GenomeSlotStats* __restrict__ slots, long long* __restrict__ wg,
                                                           typename F::Args args) {
  using Count = typename F::Count;
  __shared__ long long s_start[kMaxGenomeSegs];
  __shared__ int s_segA[kThreads], s_segB[kThreads];
  __shared__ long long s_firstA[kThreads], s_lastB[kThreads];
  __shared__ typename F::Shared s_fmt;
  __shared__ int s_lo, s_hi;
  for (int i = threadIdx.x; i < nseg; i += kThreads) s_start[i] = segs[i].start;
  F::stage(args, s_fmt);
  if (threadIdx.x == 0) { s_lo = 0x7fffffff; s_hi = -1; }
  __syncthreads();
  const long long b0 = begin + ((long long)blockIdx.x * kThreads + threadIdx.x) * F::kSpan;
  int segA = -1, segB = -1;            // segments of the thread's first / last counted line
  long long firstA = -1, lastB = -1;   // the first position of the one, the last of the other
  int cseg = -1;                       // segment the counters below belong to
  Count lines = 0, stored = 0, beyond = 0;
  bool bad = false;
  auto flush = [&]() {
    if (cseg >= 0 && (lines || bad)) {
      GenomeSlotStats* S = &slots[segs[cseg].slot];
      if (lines) atomicAdd(&S->lines, (unsigned long long)lines);
      if (stored) atomicAdd(&S->stored, (unsigned long long)stored);
      if (beyond) atomicAdd(&S->beyond, (unsigned long long)beyond);
      if (bad) atomicOr(&S->unsorted, 1u);
    }
    lines = stored = beyond = 0; bad = false;
  };
  if (b0 < end) {
    const long long b1 = b0 + F::kSpan < end ? b0 + F::kSpan : end;
    int g = -1;
    for (long long s = b0; s < b1; ++s) {
      if (s != 0 && text[s - 1] != '\n') continue;
      long long e, ns, ne;
      line_name(text, s, end, e, ns, ne);
      if (ns == ne || F::header(text, ns, ne)) continue;
      if (g < 0) {   // last segment starting at or before s
        int lo = 0, hi = nseg - 1;
        while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (s_start[mid] <= s) lo = mid; else hi = mid - 1; }
        g = lo;
      }
      while (g + 1 < nseg && s_start[g + 1] <= s) ++g;
      const GenomeSeg& G = segs[g];
      if (G.slot < 0) continue;
      typename F::Line L;
      if (!F::counted(text, ne, e, L)) continue;
      if (g != cseg) { flush(); cseg = g; }
      const Count n = (Count)(L.last - L.first + 1);
      lines += n;
      if (segB == g && L.first <= lastB) bad = true;
      if (segA < 0) { segA = g; firstA = L.first; }
      segB = g; lastB = L.last;
      const Count st = F::store(text, e, G, L, args, s_fmt, bad);
      stored += st; beyond += n - st;
    }
  }
  s_segA[threadIdx.x] = segA; s_segB[threadIdx.x] = segB;
  s_firstA[threadIdx.x] = firstA; s_lastB[threadIdx.x] = lastB;
  if (cseg >= 0 && (lines || bad)) { atomicMin(&s_lo, cseg); atomicMax(&s_hi, cseg); }
  __syncthreads();
  if (threadIdx.x == 0) {   // the threads in order: a counted line must lie beyond the previous one of its segment
    int run_seg = -1, wseg = -1;
    long long run_last = -1, wfirst = -1;
    for (int t = 0; t < kThreads; ++t) {
      if (s_segA[t] < 0) continue;
      if (wseg < 0) { wseg = s_segA[t]; wfirst = s_firstA[t]; }
      if (s_segA[t] == run_seg && s_firstA[t] <= run_last) atomicOr(&slots[segs[run_seg].slot].unsorted, 1u);
      run_seg = s_segB[t]; run_last = s_lastB[t];
    }
    long long* r = wg + 4 * (long long)blockIdx.x;
    r[0] = wseg; r[1] = wfirst; r[2] = run_seg; r[3] = run_last;
  }
  if (s_lo == s_hi) {   // every thread's remaining counts are one segment's: one set of atomics for the workgroup
    const bool mine = cseg == s_lo && (lines || bad);
    Count l = mine ? lines : 0, st = mine ? stored : 0, bd = mine ? beyond : 0;
    unsigned bb = mine && bad ? 1u : 0u;
    for (int d = 32; d >= 1; d >>= 1) { l += __shfl_xor(l, d); st += __shfl_xor(st, d); bd += __shfl_xor(bd, d); bb |= __shfl_xor(bb, d); }
    __shared__ Count s_tot[kThreads / 64][3];
    __shared__ unsigned s_bad[kThreads / 64];
    if ((threadIdx.x & 63) == 0) { s_tot[threadIdx.x >> 6][0] = l; s_tot[threadIdx.x >> 6][1] = st; s_tot[threadIdx.x >> 6][2] = bd; s_bad[threadIdx.x >> 6] = bb; }
    __syncthreads();
    if (threadIdx.x == 0) {
      unsigned long long t0 = 0, t1 = 0, t2 = 0; unsigned t3 = 0;
      for (int w = 0; w < kThreads / 64; ++w) { t0 += s_tot[w][0]; t1 += s_tot[w][1]; t2 += s_tot[w][2]; t3 |= s_bad[w]; }
      GenomeSlotStats* S = &slots[segs[s_lo].slot];
      if (t0) atomicAdd(&S->lines, t0);
      if (t1) atomicAdd(&S->stored, t1);
      if (t2) atomicAdd(&S->beyond, t2);
      if (t3) atomicOr(&S->unsorted, 1u);
    }
  } else {
    flush();
  }
}

// The run list's pieces, one workgroup per piece (grid-stride over the list): 4-byte stores up to the first 16-byte boundary,
// 16-byte stores through the body, 4-byte stores for the tail.  Every entry below min(*nruns, run_cap) was written by this launch's
// parse, as a piece or (its line did not fit, its chromosome goes to the host loop) as an empty one, len = 0, that stores nothing.
constexpr int kBedFillGrid = 512;

__global__ __launch_bounds__(kThreads) void k_bedgraph_fill(const BedRun* __restrict__ runs, const unsigned long long* __restrict__ nruns,
                                                            unsigned int run_cap) {
  const unsigned long long cnt = *nruns;
  const unsigned long long m = cnt < run_cap ? cnt : run_cap;
  for (unsigned long long r = blockIdx.x; r < m; r += gridDim.x) {
    const BedRun R = runs[r];
    int32_t* p = R.dst;
    const int len = (int)R.len, v = R.d;
    int head = (int)(((16 - ((uintptr_t)p & 15)) & 15) >> 2);
    head = head < len ? head : len;
    if ((int)threadIdx.x < head) p[threadIdx.x] = v;
    const int nv = (len - head) >> 2;
    int4* body = reinterpret_cast<int4*>(p + head);
    const int4 vv = make_int4(v, v, v, v);
    for (int i = threadIdx.x; i < nv; i += kThreads) body[i] = vv;
    const int t0 = head + 4 * nv;
    if (t0 + (int)threadIdx.x < len) p[t0 + threadIdx.x] = v;
  }
}

}  // namespace

int genome_parse_workgroups(GenomeFormat format, long long nbytes) {
  const long long tile = (long long)kThreads * (format == GenomeFormat::kSamples ? SampleLines::kSpan : kSpan);
  return (int)((nbytes + tile - 1) / tile);
}

unsigned long long bedgraph_run_cap(long long text_bytes, long long sum_len) {
  return (unsigned long long)(text_bytes / 8 + 2 + sum_len / kBedPiece);
}

void launch_parse_genome(GenomeFormat format, const void* text, long long begin, long long end, const GenomeSeg* segs, int nseg,
                         GenomeSlotStats* slots, long long* wg, const GenomeSampleCols* cols, BedRun* runs, unsigned long long* nruns,
                         unsigned int run_cap, hipStream_t stream) {
  const int grid = genome_parse_workgroups(format, end - begin);
  if (grid <= 0 || nseg <= 0 || (format == GenomeFormat::kSamples && cols->n <= 0)) return;
  const unsigned char* t = static_cast<const unsigned char*>(text);
  const BedLines::Args bed{runs, nruns, run_cap};
  switch (format) {
    case GenomeFormat::kText: RSI_LAUNCH(k_parse_genome<TextLines>, dim3(grid), dim3(kThreads), 0, stream, t, begin, end, segs, nseg, slots, wg, TextLines::Args()); break;
    case GenomeFormat::kSamples: RSI_LAUNCH(k_parse_genome<SampleLines>, dim3(grid), dim3(kThreads), 0, stream, t, begin, end, segs, nseg, slots, wg, *cols); break;
    case GenomeFormat::kBedgraph: RSI_LAUNCH(k_parse_genome<BedLines>, dim3(grid), dim3(kThreads), 0, stream, t, begin, end, segs, nseg, slots, wg, bed); break;
  }
  RSI_LAUNCH(k_genome_order_fold, dim3(1), dim3(kThreads), 0, stream, wg, grid, segs, slots);
  if (format == GenomeFormat::kBedgraph) RSI_LAUNCH(k_bedgraph_fill, dim3(kBedFillGrid), dim3(kThreads), 0, stream, runs, nruns, run_cap);
}

void launch_text_name_bounds(const void* text, long long nbytes, NameBound* bounds, unsigned int* count, unsigned int cap, hipStream_t stream,
                             bool bedgraph) {
  const int grid = (int)((nbytes + kTile - 1) / kTile);
  if (grid <= 0) return;
  if (bedgraph) RSI_LAUNCH(k_text_name_bounds<true>, dim3(grid), dim3(kThreads), 0, stream, static_cast<const unsigned char*>(text), nbytes, bounds, count, cap);
  else RSI_LAUNCH(k_text_name_bounds<false>, dim3(grid), dim3(kThreads), 0, stream, static_cast<const unsigned char*>(text), nbytes, bounds, count, cap);
}

int text_parse_workgroups(long long nbytes) { return (int)((nbytes + kTile - 1) / kTile); }

void launch_parse_depth_text(const void* text, long long nbytes, long long size, int32_t* depth, long long* wg_first,
                             long long* wg_max, TextParseStats* stats, hipStream_t stream) {
  const int grid = text_parse_workgroups(nbytes);
  if (grid <= 0) return;
  RSI_LAUNCH(k_parse_depth_text, dim3(grid), dim3(kThreads), 0, stream, static_cast<const unsigned char*>(text), nbytes, size,
                     depth, wg_first, wg_max, stats);
}

}  // namespace rsik

// ------------------------------------------------------------------------------------------
// BAM pileup -> per-base depth.  The host inflates the BGZF blocks and finds the
// record boundaries; everything the reference does per read -- the filters of load_data_from_bam
// (loaddata.cpp:313-320), the CIGAR positions of resolve_cigar_pos (samfunctions.cpp:38-100) and the
// per-base quality test (loaddata.cpp:328-331) -- runs here, one thread per record, on the inflated
// bytes in HBM.  A run of counted bases becomes +1 / -1 in a difference array; an inclusive scan turns
// that into the depth.
namespace rsik {

namespace {

__device__ inline uint32_t ld_u32(const unsigned char* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
__device__ inline uint32_t ld_u16(const unsigned char* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }

enum { kCigM = 0, kCigI = 1, kCigD = 2, kCigN = 3, kCigS = 4, kCigEq = 7, kCigX = 8 };

__global__ __launch_bounds__(256) void k_bam_depth(const unsigned char* __restrict__ data, const uint32_t* __restrict__ rec_off,
                                                   int nrec, int tid, int minq, int min_baseq, long long n,
                                                   int32_t* __restrict__ diff, BamDepthStats* __restrict__ stats) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  unsigned used = 0, runs = 0, bad = 0;
  if (i < nrec) {
    const long long bsize = (long long)ld_u32(data + rec_off[i]);   // block_size: bytes of the record behind this field
    const unsigned char* b = data + rec_off[i] + 4;       // past block_size
    const int rtid = (int)ld_u32(b), pos0 = (int)ld_u32(b + 4);
    const int l_name = b[8], mapq = b[9];
    const int n_cig = (int)ld_u16(b + 12), flag = (int)ld_u16(b + 14);
    const int l_seq = (int)ld_u32(b + 16);
    // A record whose variable-length fields do not fit its block_size (corrupt or crafted file) is counted and skipped:
    // nothing below may read past the record or write outside the depth array.  pos < 0 (an unplaced read that carries a
    // reference id) is never yielded by the reference's region iterator: skipped like the other filtered reads.
    const bool fits = l_seq >= 0 && 32ll + l_name + 4ll * n_cig + ((long long)l_seq + 1) / 2 + (long long)l_seq <= bsize;
    if (!fits) bad = 1;
    // loaddata.cpp:315-319: pos == 0, tid < 0, mapq, secondary, duplicate (the iterator only yields this tid)
    const bool keep = fits && rtid == tid && pos0 > 0 && mapq >= minq && !(flag & 0x100) && !(flag & 0x400);
    if (keep) {
      const unsigned char* cig = b + 32 + l_name;
      const unsigned char* qual = cig + 4 * n_cig + (l_seq + 1) / 2;
      // anchor: the first M / D / = / X (samfunctions.cpp:75-78); without one the read contributes nothing
      int anchor = -1;
      for (int k = 0; k < n_cig && anchor < 0; ++k) { const int op = cig[4 * k] & 0xf; if (op == kCigM || op == kCigD || op == kCigEq || op == kCigX) anchor = k; }
      if (anchor >= 0) {
        used = 1;
        long long ref_end = (long long)pos0 + 1;     // 1-based position of op `anchor` (samfunctions.cpp:85-92)
        // The query position is 64 bits wide because it goes on growing behind the read's end: an op adds less than 2^28
        // and there are fewer than 2^16 ops, so q stays below 2^44 and never wraps, whatever a crafted CIGAR says (as an
        // int it could turn negative and pass the `q + t >= l_seq` cut below).  qual[] is read at 0 <= q + t < l_seq only.
        long long q = 0;
        for (int k = 0; k < n_cig; ++k) {
          const uint32_t c = ld_u32(cig + 4 * k);
          const int op = (int)(c & 0xf), len = (int)(c >> 4);
          if (k >= anchor && (op == kCigM || op == kCigEq)) {
            const long long p1 = ref_end - 1;        // 0-based reference position of the op's first base
            // bases with quality >= min_baseq, in runs (loaddata.cpp:328-331)
            long long run_start = -1;
            for (int t = 0; t < len; ++t) {
              const long long p = p1 + t;
              if (p >= n || q + t >= l_seq) break;   // the second: a CIGAR longer than the read (malformed)
              const bool ok = qual[q + t] >= min_baseq;
              if (ok && run_start < 0) run_start = p;
              if (!ok && run_start >= 0) { atomicAdd(&diff[run_start], 1); atomicAdd(&diff[p], -1); run_start = -1; ++runs; }
            }
            if (run_start >= 0) {
              long long e = p1 + len; if (e > n) e = n;
              if (q + len > l_seq) { const long long eq = p1 + (l_seq - q); e = eq < e ? eq : e; }
              if (e > run_start) { atomicAdd(&diff[run_start], 1); atomicAdd(&diff[e], -1); ++runs; }
            }
          }
          // ops before the anchor never match (they are I / S / H / N / P); their positions are not needed
          if (k >= anchor && (op == kCigM || op == kCigD || op == kCigN || op == kCigS)) ref_end += len;   // '=' and 'X' do not advance: reference quirk
          if (op == kCigM || op == kCigI || op == kCigS || op == kCigEq || op == kCigX) q += len;          // samfunctions.cpp:67-71
        }
      }
    }
  }
  for (int d = 32; d >= 1; d >>= 1) { used += __shfl_xor(used, d); runs += __shfl_xor(runs, d); bad += __shfl_xor(bad, d); }
  if ((threadIdx.x & 63) == 0) {
    if (used) atomicAdd(&stats->used, (unsigned long long)used);
    if (runs) atomicAdd(&stats->runs, (unsigned long long)runs);
    if (bad) atomicAdd(&stats->malformed, (unsigned long long)bad);
  }
}

// ---- inclusive scan of int32 in place: tile sums, scan of the tile sums, tile scan + offset ----
constexpr int kScanThreads = 256, kScanPer = 16, kScanTileElems = kScanThreads * kScanPer;

__device__ inline int wg_exscan_i32(int v, int* s_w /* 4 */, int* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int incl = v;
  for (int d = 1; d < 64; d <<= 1) { const int up = __shfl_up(incl, d); if (lane >= d) incl += up; }
  __syncthreads();
  if (lane == 63) s_w[wave] = incl;
  __syncthreads();
  int base = 0, tot = 0;
  for (int w = 0; w < kScanThreads / 64; ++w) { if (w < wave) base += s_w[w]; tot += s_w[w]; }
  __syncthreads();
  *total = tot;
  return base + incl - v;
}

__global__ __launch_bounds__(kScanThreads) void k_scan_tile_sums(const int32_t* __restrict__ x, long long n, int32_t* __restrict__ tile_sum) {
  __shared__ int s_w[kScanThreads / 64];
  const long long e0 = (long long)blockIdx.x * kScanTileElems + (long long)threadIdx.x * kScanPer;
  int s = 0;
  for (int k = 0; k < kScanPer; ++k) if (e0 + k < n) s += x[e0 + k];
  int total;
  (void)wg_exscan_i32(s, s_w, &total);
  if (threadIdx.x == 0) tile_sum[blockIdx.x] = total;
}
__global__ __launch_bounds__(kScanThreads) void k_scan_tile_offsets(int32_t* __restrict__ tile_sum, int ntiles) {   // exclusive, in place, one workgroup
  __shared__ int s_w[kScanThreads / 64];
  int carry = 0;
  for (int t0 = 0; t0 < ntiles; t0 += kScanThreads) {
    const int t = t0 + (int)threadIdx.x;
    const int v = t < ntiles ? tile_sum[t] : 0;
    int total;
    const int ex = wg_exscan_i32(v, s_w, &total);
    if (t < ntiles) tile_sum[t] = carry + ex;
    carry += total;
  }
}
__global__ __launch_bounds__(kScanThreads) void k_scan_apply(int32_t* __restrict__ x, long long n, const int32_t* __restrict__ tile_off) {
  __shared__ int s_w[kScanThreads / 64];
  const long long e0 = (long long)blockIdx.x * kScanTileElems + (long long)threadIdx.x * kScanPer;
  int v[kScanPer];
  int s = 0;
#pragma unroll
  for (int k = 0; k < kScanPer; ++k) { v[k] = e0 + k < n ? x[e0 + k] : 0; s += v[k]; v[k] = s; }
  int total;
  const int base = tile_off[blockIdx.x] + wg_exscan_i32(s, s_w, &total);
#pragma unroll
  for (int k = 0; k < kScanPer; ++k) if (e0 + k < n) x[e0 + k] = base + v[k];
}

}  // namespace

void launch_bam_depth(const void* data, const uint32_t* rec_off, int nrec, int tid, int minq, int min_baseq, long long n, int32_t* diff,
                      BamDepthStats* stats, hipStream_t stream) {
  if (nrec <= 0) return;
  RSI_LAUNCH(k_bam_depth, dim3((nrec + 255) / 256), dim3(256), 0, stream, static_cast<const unsigned char*>(data), rec_off, nrec, tid,
                     minq, min_baseq, n, diff, stats);
}
int scan_tiles(long long n) { return (int)((n + kScanTileElems - 1) / kScanTileElems); }
void launch_inclusive_scan_i32(int32_t* x, long long n, int32_t* tile_scratch, hipStream_t stream) {
  const int ntiles = scan_tiles(n);
  if (ntiles <= 0) return;
  RSI_LAUNCH(k_scan_tile_sums, dim3(ntiles), dim3(kScanThreads), 0, stream, x, n, tile_scratch);
  RSI_LAUNCH(k_scan_tile_offsets, dim3(1), dim3(kScanThreads), 0, stream, tile_scratch, ntiles);
  RSI_LAUNCH(k_scan_apply, dim3(ntiles), dim3(kScanThreads), 0, stream, x, n, tile_scratch);
}

}  // namespace rsik
