// bam_pairs_core.h -- the read-pair annotation's per-record logic, for the pair kernels (kernels_pairs.hip) and
// for plain host C++ (tests/pairs_harness.cpp).  The same functions run in both builds.  Three parts: the fields a record
// leaves in the pair table (extract), the insert-size sample's rules as an associative element over the table's records
// (Seg, compose: what bam_pair_sample's serial loop keeps between two reads), and the decision for one (call, record) pair
// (decide: bam_annotate_calls' visitor, line for line).  The serial forms at the end are the kernels' oracle.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define RSI_PAIRS_HD __host__ __device__ inline
#else
#define RSI_PAIRS_HD inline
#endif

namespace rsipairs {

// ---- the table entry ----
// info: mapq (bits 0-7) | flag << 8 (bits 8-23) | cigar class << 24 (0: no op, 1: one op, 2: two or more) |
// mate elsewhere (mtid != tid && mtid > 0) << 26 | (mtid == tid) << 27
struct Entry { int32_t pos, rend, mpos, isize; uint32_t info; };
constexpr uint32_t kMateElsewhere = 1u << 26, kMateSame = 1u << 27;
RSI_PAIRS_HD uint32_t mapq_of(uint32_t info) { return info & 0xffu; }
RSI_PAIRS_HD uint32_t flag_of(uint32_t info) { return (info >> 8) & 0xffffu; }
RSI_PAIRS_HD uint32_t cigar_class(uint32_t info) { return (info >> 24) & 3u; }
RSI_PAIRS_HD uint32_t pack_info(uint32_t mapq, uint32_t flag, uint32_t n_cigar, int32_t tid, int32_t mtid) {
  return (mapq & 0xffu) | ((flag & 0xffffu) << 8) | ((n_cigar >= 2 ? 2u : n_cigar) << 24) | ((mtid != tid && mtid > 0) ? kMateElsewhere : 0u) |
         (mtid == tid ? kMateSame : 0u);
}

enum LoadFlag : uint32_t { kUnsorted = 1, kOverrun = 2 };   // a pos below its predecessor's / name and CIGAR do not fit block_size

template <class B> RSI_PAIRS_HD uint32_t rd32(const B& d, uint64_t off) {
  return (uint32_t)d.at(off) | ((uint32_t)d.at(off + 1) << 8) | ((uint32_t)d.at(off + 2) << 16) | ((uint32_t)d.at(off + 3) << 24);
}
template <class B> RSI_PAIRS_HD uint32_t rd16(const B& d, uint64_t off) { return (uint32_t)d.at(off) | ((uint32_t)d.at(off + 1) << 8); }

// The entry of the record whose block_size field is at `off` (a whole record: off + 4 + block_size bytes are readable, and
// block_size >= 32).  rend = n_cigar ? bam_calend : pos + 1, calend = pos + lengths of M / D / N as BamReader::next sums them
// (kept as int32, the cast bam_annotate_calls makes).  overrun: 32 + l_name + 4 n_cigar > block_size -- BamReader::next's
// "name / CIGAR overrun the record"; the CIGAR is not read then, and rend is pos + 1.
template <class B> RSI_PAIRS_HD Entry extract(const B& d, uint64_t off, int32_t tid, bool& overrun) {
  const uint32_t bs = rd32(d, off);
  const uint64_t b = off + 4;
  Entry e;
  e.pos = (int32_t)rd32(d, b + 4);
  const uint32_t l_name = d.at(b + 8), mapq = d.at(b + 9), n_cigar = rd16(d, b + 12), flag = rd16(d, b + 14);
  const int32_t mtid = (int32_t)rd32(d, b + 20);
  e.mpos = (int32_t)rd32(d, b + 24);
  e.isize = (int32_t)rd32(d, b + 28);
  e.info = pack_info(mapq, flag, n_cigar, tid, mtid);
  overrun = 32ull + l_name + 4ull * n_cigar > (uint64_t)bs;
  int64_t end = e.pos;
  if (!overrun) {
    const uint64_t cig = b + 32 + l_name;
    for (uint32_t k = 0; k < n_cigar; ++k) {
      const uint32_t c = rd32(d, cig + 4ull * k);
      const uint32_t op = c & 0xf;
      if (op == 0 || op == 2 || op == 3) end += c >> 4;     // M, D, N (bam.c:23)
    }
  }
  e.rend = (n_cigar && !overrun) ? (int32_t)end : (int32_t)((int64_t)e.pos + 1);
  return e;
}

// ---- the insert-size sample (bam_pair_sample, the part of bam_rd_pr_stats cnv_stat uses) ----
constexpr int32_t kSampleBeg = 10000000, kSampleEnd = 349250621;   // cnv_stat's window (pairrd.cpp:636)
constexpr int32_t kSampleGap = 1000, kSampleLen = 1000000, kSampleCount = 1000000, kSampleNoPrev = -10000;

// the records for_reads_in(beg, end) yields and the visitor does not pass over, in table order: j = 0, 1, ...
RSI_PAIRS_HD bool sample_kept(int32_t pos, int32_t rend, uint32_t info) {
  if (!(rend > kSampleBeg && pos < kSampleEnd)) return false;
  if (info & kMateElsewhere) return false;
  const uint32_t flag = flag_of(info);
  return !(flag & 0x100u) && !(flag & 0x400u);
}
// ... and those whose isize goes into the sums: flag 0x2 and mtid == tid
RSI_PAIRS_HD bool sample_summed(uint32_t info) { return (flag_of(info) & 0x2u) && (info & kMateSame); }
// int * int as the reference computes it: the product wrapped to 32 bits
RSI_PAIRS_HD int32_t isize_square(int32_t isize) { return (int32_t)((uint32_t)isize * (uint32_t)isize); }
RSI_PAIRS_HD int64_t isize_abs(int32_t isize) { return isize < 0 ? -(int64_t)isize : (int64_t)isize; }

// What a run of consecutive kept records leaves behind, and how two runs join.  n: its records (0: none, the identity);
// first / last: the pos of its first and last; hasb: a boundary (pos > predecessor's pos + 1000) lies at a record other
// than its first; then bpos is the pos at the last such boundary and tail the records from it on; without one tail == n.
// compose is associative: the scan over the table may bracket it any way.
struct Seg { int32_t n, first, last, hasb, bpos, tail; };
RSI_PAIRS_HD Seg seg_none() { return Seg{0, 0, 0, 0, 0, 0}; }
RSI_PAIRS_HD Seg seg_one(int32_t pos) { return Seg{1, pos, pos, 0, 0, 1}; }
RSI_PAIRS_HD Seg compose(const Seg& a, const Seg& b) {
  if (b.n == 0) return a;
  if (a.n == 0) return b;
  Seg r;
  r.n = a.n + b.n; r.first = a.first; r.last = b.last;
  if (b.hasb) { r.hasb = 1; r.bpos = b.bpos; r.tail = b.tail; }
  else if ((int64_t)b.first > (int64_t)a.last + kSampleGap) { r.hasb = 1; r.bpos = b.first; r.tail = b.n; }
  else { r.hasb = a.hasb; r.bpos = a.bpos; r.tail = a.tail + b.n; }
  return r;
}
// For p = the records 0 .. j joined: pos_start and count as the serial loop holds them behind record j (the predecessor of
// record 0 is at -10000; pos_start begins as 0).  The count saturates in int32 only beyond 2^31 records.
RSI_PAIRS_HD void sample_state(const Seg& p, int32_t& seg_start, int32_t& count) {
  if (p.hasb) { seg_start = p.bpos; count = p.tail; }
  else if ((int64_t)p.first > (int64_t)kSampleNoPrev + kSampleGap) { seg_start = p.first; count = p.n; }
  else { seg_start = 0; count = p.n; }
}
// Does record j stop the sample?  p as above (record j included).
RSI_PAIRS_HD bool sample_stops(const Seg& p, int32_t pos, int32_t rend, uint32_t info, int64_t tid_len) {
  if ((int64_t)pos >= tid_len) return true;
  if (cigar_class(info) > 0 && (int64_t)rend >= tid_len) return true;   // a record without CIGAR: calend == pos
  int32_t seg_start, count;
  sample_state(p, seg_start, count);
  return count > kSampleCount || (int64_t)pos - (int64_t)seg_start > kSampleLen;
}

// ---- the annotation of one call ----
struct Call { int32_t beg, end, type, len, p1e, p2e; };   // beg <= end; len = end - beg + 1; [p1e, p2e): the window read
// The windows of a list of calls: DIS carries over from call to call (bam_annotate_calls).
struct Windows {
  int32_t dis = 1000;
  Call next(int32_t start, int32_t end, int32_t type) {
    Call c;
    if (start > end) { const int32_t t = start; start = end; end = t; }
    c.beg = start; c.end = end; c.type = type;
    c.len = end - start + 1;
    dis = dis > c.len ? dis : c.len;
    dis = dis < 5000 ? dis : 5000;
    const int64_t p1 = (int64_t)start - dis, p2 = (int64_t)end + dis;
    c.p1e = p1 < 1 ? 1 : (int32_t)p1;
    c.p2e = p2 > INT32_MAX ? INT32_MAX : (int32_t)p2;
    return c;
  }
};

enum Vote : uint32_t { kQ0All = 1, kQ0Q0 = 2, kRp = 4 };
RSI_PAIRS_HD int64_t iabs64(int64_t v) { return v < 0 ? -v : v; }
// What one record adds to one call's counts: bam_annotate_calls' visitor behind for_reads_in's filter, its tests in its order.
// 64-bit integers throughout: equal to the host's int arithmetic wherever that does not overflow, and `overlap < x * 0.5` is
// `2 overlap < x` exactly.
RSI_PAIRS_HD uint32_t decide(const Call& c, int32_t pos, int32_t rend32, int32_t mpos, uint32_t info, int32_t isize_mean, int32_t isize_sd) {
  if (!(rend32 > c.p1e && pos < c.p2e)) return 0;          // for_reads_in: overlapping [p1e, p2e)
  if (cigar_class(info) < 2) return 0;                     // n_cigar <= 1
  uint32_t v = 0;
  const int64_t beg = c.beg, end = c.end, LEN = c.len;
  if (rend32 > c.beg && pos < c.end) { v |= kQ0All; if (mapq_of(info) == 0) v |= kQ0Q0; }
  if (info & kMateElsewhere) return v;
  const uint32_t flag = flag_of(info);
  const bool rev = (flag & 0x10u) != 0, mrev = (flag & 0x20u) != 0;
  if (rev == mrev) return v;                               // both forward, or both reverse
  int64_t r1 = rend32, r2 = mpos;
  const int64_t far = (int64_t)isize_mean + (int64_t)isize_sd * 3;
  if (c.type == 0) {
    if (r2 - r1 < far) return v;
    const int64_t overlap = (r2 < end ? r2 : end) - (r1 > beg ? r1 : beg);
    if (overlap < 0) return v;
    if (iabs64(r1 - beg) + iabs64(r2 - end) < far) return v | kRp;
    if (2 * overlap < LEN) return v;
    if (2 * overlap < r2 - r1) return v;
    return v | kRp;
  }
  if (c.type == 1) {
    if (r2 - r1 > (int64_t)isize_mean - (int64_t)isize_sd * 3) return v;
    if (iabs64(r1 - beg) + iabs64(r2 - end) < far) return v | kRp;
    if (r1 > r2) { const int64_t t = r1; r1 = r2; r2 = t; }
    const int64_t overlap = (r2 < end ? r2 : end) - (r1 > beg ? r1 : beg);
    if (2 * overlap < LEN) return v;
    if (2 * overlap < r2 - r1) return v;
    return v | kRp;
  }
  return v;
}

// ---- serial forms over a table (the oracle of the kernels) ----
// out: count, sum |isize|, sum of the wrapped squares, S (the stopping j, or the last j; -1: no record).  The integer sums
// equal bam_pair_sample's double sums wherever those are exact (|sum| < 2^53).
inline void sample_serial(int64_t n, const int32_t* pos, const int32_t* rend, const int32_t* isize, const uint32_t* info, int64_t tid_len,
                          int64_t out[4]) {
  Seg p = seg_none();
  out[0] = out[1] = out[2] = 0; out[3] = -1;
  for (int64_t i = 0; i < n; ++i) {
    if (!sample_kept(pos[i], rend[i], info[i])) continue;
    p = compose(p, seg_one(pos[i]));
    out[3] = (int64_t)p.n - 1;
    if (sample_summed(info[i])) { out[0] += 1; out[1] += isize_abs(isize[i]); out[2] += isize_square(isize[i]); }
    if (sample_stops(p, pos[i], rend[i], info[i], tid_len)) break;
  }
}
inline void annotate_serial(int64_t n, const int32_t* pos, const int32_t* rend, const int32_t* mpos, const uint32_t* info, const Call& c,
                            int32_t isize_mean, int32_t isize_sd, uint32_t out[3]) {
  out[0] = out[1] = out[2] = 0;
  for (int64_t i = 0; i < n; ++i) {
    const uint32_t v = decide(c, pos[i], rend[i], mpos[i], info[i], isize_mean, isize_sd);
    out[0] += (v & kQ0All) != 0; out[1] += (v & kQ0Q0) != 0; out[2] += (v & kRp) != 0;
  }
}

}  // namespace rsipairs
