// bam_pin_core.h -- the per-read logic of `rsicnv pin`, for the pin kernels (kernels_pin.hip) and for plain host
// C++ (tests/pin_harness.cpp).  The same functions run in both builds.  Three parts: a read's CIGAR as the reference's
// resolve_cigar_pos places it (counted_runs), the depth sample of bam_rd_pr_stats over the pair table plus the CIGAR pool
// (which reads add where), and one breakpoint's window (get_rds_stats and the scoring loop of optimize_resolution).  The serial
// forms at the end are the kernels' oracle.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "bam_pairs_core.h"

#if defined(__HIPCC__) || defined(__HIP__)
#define RSI_PIN_HD __host__ __device__ inline
#else
#define RSI_PIN_HD inline
#endif

namespace rsipin {

// ---- the kept CIGARs ----
// Per read of the pair table: lq = l_qseq, coff = where its CIGAR lies in the pool of uint32 words: pool[coff] = n_cigar,
// pool[coff + 1 ...] the operations as the record holds them (length << 4 | op).  8 bytes per read and 4 + 4 n_cigar in the pool.
struct Tab { const int32_t* lq; const uint32_t* coff; const uint32_t* pool; };

RSI_PIN_HD bool op_anchors(uint32_t op) { return op == 0 || op == 2 || op == 7 || op == 8; }   // M, D, =, X
// The stretches of counted bases of a read at `pos` (0-based): f(first 0-based reference position, length) per M or '=' op, with
// resolve_cigar_pos's positions (samfunctions.cpp:38): from the first M / D / = / X on, M, D, N and S advance; = and X do not.
template <class F> RSI_PIN_HD void counted_runs(const uint32_t* cig, uint32_t n, int32_t pos, F&& f) {
  uint32_t a = 0;
  while (a < n && !op_anchors(cig[a] & 0xf)) ++a;
  int64_t at = pos;
  for (uint32_t k = a; k < n; ++k) {
    const uint32_t op = cig[k] & 0xf, l = cig[k] >> 4;
    if (op == 0 || op == 7) f(at, (int64_t)l);
    if (op == 0 || op == 2 || op == 3 || op == 4) at += l;
  }
}
// bam_calend as the loops use it: of a read without CIGAR it is its pos (the table's rend is pos + 1 there)
RSI_PIN_HD int32_t calend_of(int32_t pos, int32_t rend, uint32_t info) { return rsipairs::cigar_class(info) ? rend : pos; }

// ---- the depth sample (bam_rd_pr_stats) ----
constexpr int32_t kRdcSize = rsipairs::kSampleLen + 1000;      // RDC.resize(sample_len + 1000)
constexpr int32_t kRdcLimit = kRdcSize - 100;                  // beyond it the reference grows the array by copies of its last element
enum SampleFlag : uint32_t { kGrows = 1 };
// What the sample leaves behind: the last stretch's start and the pos of the last read counted, how many reads that stretch
// has and the sum of their l_qseq; flags: SampleFlag.  count == 0: no read was accepted.
struct SampleState { int32_t pos_start, pos_end, count, flags; int64_t lq_sum; };
// Does the stopping read S end the loop before it is counted (pos or calend at the chromosome's end), or behind count++?
RSI_PIN_HD bool stops_uncounted(int32_t pos, int32_t rend, uint32_t info, int64_t tid_len) {
  return (int64_t)pos >= tid_len || (int64_t)calend_of(pos, rend, info) >= tid_len;
}
// One accepted read's bases into a difference array of kRdcSize + 1 words at its own stretch's offset: add(index, +1 / -1).
template <class A> RSI_PIN_HD void sample_add(const uint32_t* cig, uint32_t n, int32_t pos, int32_t offset, int64_t tid_len, A&& add) {
  counted_runs(cig, n, pos, [&](int64_t p1, int64_t l) {
    int64_t a = p1 - offset, b = (p1 + l < tid_len ? p1 + l : tid_len) - offset;
    if (a < 0) a = 0;
    if (b > kRdcSize) b = kRdcSize;
    if (a < b) { add(a, 1); add(b, -1); }
  });
}
// drd of the sample at index k of the last stretch: q = l_qseq / 4 bases on each side, int arithmetic
RSI_PIN_HD int32_t sample_drd(const int32_t* rd, int32_t k, int32_t l_qseq) {
  const int32_t q = l_qseq / 4;
  int32_t d0 = 0, d1 = 0;
  for (int32_t i = k - q; i < k; ++i) d0 += rd[i];
  for (int32_t i = k; i < k + q; ++i) d1 += rd[i];
  return (d1 - d0) * 4 / l_qseq;
}

// ---- one breakpoint's window (get_rds_stats) ----
constexpr int32_t kMinRlen = 50;
RSI_PIN_HD int32_t r_len_of(int32_t m, int32_t l_qseq) { const int32_t r = m > l_qseq ? m : l_qseq; return r > kMinRlen ? r : kMinRlen; }
// Is the read one the iterator yields for [beg, end) (beg below 0 queries from 0) and none of the filters passes over?
RSI_PIN_HD bool window_kept(int32_t pos, int32_t rend, uint32_t info, int64_t tid_len, int64_t beg, int64_t end) {
  const int64_t qbeg = beg < 0 ? 0 : beg;
  if (!((int64_t)pos < end && (int64_t)rend > qbeg)) return false;
  if (info & rsipairs::kMateElsewhere) return false;
  const uint32_t flag = rsipairs::flag_of(info);
  if ((flag & 0x100u) || (flag & 0x400u)) return false;
  return !stops_uncounted(pos, rend, info, tid_len);
}
enum Counter { kRd = 0, kSBeg = 1, kSEnd = 2 };
// What one kept read adds to the window's counters: inc(counter, ipos), ipos in [0, 2 r_len].
template <class I> RSI_PIN_HD void window_add(const uint32_t* cig, uint32_t n, int32_t pos, int32_t rend, int64_t beg, int32_t r_len, I&& inc) {
  const int64_t w = 2 * (int64_t)r_len;
  if (n >= 2) {
    const int64_t ib = (int64_t)pos + 1 - beg, ie = (int64_t)rend + 1 - beg;
    if (!op_anchors(cig[0] & 0xf) && ib >= 0 && ib <= w) inc(kSBeg, (int32_t)ib);
    if (!op_anchors(cig[n - 1] & 0xf) && ie >= 0 && ie <= w) inc(kSEnd, (int32_t)ie);
  }
  counted_runs(cig, n, pos, [&](int64_t p1, int64_t l) {
    int64_t a = p1 + 1 - beg, b = a + l;
    if (a < 0) a = 0;
    if (b > w + 1) b = w + 1;
    for (int64_t i = a; i < b; ++i) inc(kRd, (int32_t)i);
  });
}
// drd at index k of a window of `size` entries; 0 outside [q, size - q)
RSI_PIN_HD int32_t window_drd(const int32_t* rd, int32_t size, int32_t k, int32_t l_qseq) {
  const int32_t q = l_qseq / 4;
  if (k < q || k >= size - q) return 0;
  int64_t d0 = 0, d1 = 0;
  for (int32_t i = k - q > 0 ? k - q : 0; i < k; ++i) d0 += rd[i];
  for (int32_t i = k; i < (k + q < size ? k + q : size); ++i) d1 += rd[i];
  return (int32_t)((d1 - d0) * 4 / l_qseq);
}
// score5 (five) or score3 of one index, as IEEE doubles
RSI_PIN_HD double score_of(int32_t drd, int32_t clips, double drd_sd, bool five) {
  return five ? (double)(-drd) / drd_sd + 3.0 * (double)clips : (double)drd / drd_sd + 3.0 * (double)clips;
}
// The serial loop takes index i when its score is above the best so far (0.0 at first).  Of two candidates (score, index) the
// loop's final choice is the higher score, the lower index among equals; a NaN never wins.
struct Best { double score; int32_t i; };
RSI_PIN_HD Best best_none() { return Best{0.0, -1}; }
RSI_PIN_HD Best best_of(const Best& a, const Best& b) {
  if (b.i < 0) return a;
  if (a.i < 0) return b;
  if (b.score > a.score) return b;
  if (a.score > b.score) return a;
  return a.i < b.i ? a : b;
}
RSI_PIN_HD Best best_take(const Best& a, double score, int32_t i) { return score > 0.0 ? best_of(a, Best{score, i}) : a; }

// A breakpoint as the kernel gets it: its position (1-based, as the list has it) and which score it uses.
struct Bp { int32_t bp, five; };
// The two breakpoints of a call (type 0 DEL, 1 DUP): a DEL scores its start with score5 and its end with score3, a DUP the
// other way round.
RSI_PIN_HD void bps_of(int32_t start, int32_t end, int32_t type, Bp out[2]) {
  out[0] = Bp{start, type == 0}; out[1] = Bp{end, type != 0};
}
// Where a breakpoint goes: to index i_max of its window (bp - RDC.size() / 2 + i_max) if at least two clipped reads end there
RSI_PIN_HD int32_t moved(int32_t bp, int32_t r_len, int32_t i_max, int32_t clips) {
  return clips >= 2 ? (int32_t)((int64_t)bp - r_len + i_max) : bp;
}
// Is the call looked at at all?  (short ones and unknown types are left as they are)
RSI_PIN_HD bool call_pinned(int32_t start, int32_t end, int32_t type) {
  const int64_t d = (int64_t)end - start;
  return (d < 0 ? -d : d) >= 800 && (type == 0 || type == 1);
}

// ---- serial forms over a table (the oracle of the kernels) ----
// The sample: rd[kRdcSize] (zeroed here) gets the counts of the reads before the stop read, each at its stretch's offset.
inline SampleState sample_serial(int64_t n, const int32_t* pos, const int32_t* rend, const uint32_t* info, const Tab& t, int64_t tid_len, int32_t* rd) {
  for (int32_t i = 0; i < kRdcSize; ++i) rd[i] = 0;
  SampleState st{0, -10000, 0, 0, 0};
  int32_t offset = 0;
  for (int64_t i = 0; i < n; ++i) {
    if (!rsipairs::sample_kept(pos[i], rend[i], info[i])) continue;
    if (stops_uncounted(pos[i], rend[i], info[i], tid_len)) break;
    if ((int64_t)pos[i] > (int64_t)st.pos_end + rsipairs::kSampleGap) { st.count = 0; st.pos_start = offset = pos[i]; st.lq_sum = 0; }
    if ((int64_t)calend_of(pos[i], rend[i], info[i]) - offset > kRdcLimit) st.flags |= kGrows;
    st.pos_end = pos[i];
    st.lq_sum += t.lq[i];
    st.count += 1;
    if (st.count > rsipairs::kSampleCount || (int64_t)st.pos_end - st.pos_start > rsipairs::kSampleLen) break;
    const uint32_t* c = t.pool + t.coff[i];
    sample_add(c + 1, c[0], pos[i], offset, tid_len, [&](int64_t at, int d) { if (at < kRdcSize) rd[at] += d; });
  }
  // the difference array summed in place (index kRdcSize is never stored: sample_add's -1 there falls off the end)
  int32_t run = 0;
  for (int32_t i = 0; i < kRdcSize; ++i) { run += rd[i]; rd[i] = run; }
  return st;
}
// One breakpoint: out = i_max (-1: none), the clip count at it (0 then).  w: 3 * (2 r_len + 1) words of scratch.
inline void window_serial(int64_t n, const int32_t* pos, const int32_t* rend, const uint32_t* info, const Tab& t, int64_t tid_len, Bp b, int32_t r_len,
                          int32_t l_qseq, double drd_sd, int32_t* w, int32_t out[2]) {
  const int32_t size = 2 * r_len + 1;
  for (int32_t i = 0; i < 3 * size; ++i) w[i] = 0;
  const int64_t beg = (int64_t)b.bp - r_len, end = (int64_t)b.bp + r_len;
  for (int64_t i = 0; i < n; ++i) {
    if (!window_kept(pos[i], rend[i], info[i], tid_len, beg, end)) continue;
    const uint32_t* c = t.pool + t.coff[i];
    window_add(c + 1, c[0], pos[i], rend[i], beg, r_len, [&](int which, int32_t ipos) { w[which * size + ipos] += 1; });
  }
  Best best = best_none();
  const int32_t* clips = w + (b.five ? kSEnd : kSBeg) * size;
  for (int32_t i = 0; i < size; ++i) best = best_take(best, score_of(window_drd(w, size, i, l_qseq), clips[i], drd_sd, b.five != 0), i);
  out[0] = best.i; out[1] = best.i >= 0 ? clips[best.i] : 0;
}

}  // namespace rsipin
