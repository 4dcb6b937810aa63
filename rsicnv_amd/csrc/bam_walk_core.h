// bam_walk_core.h -- the record chain of inflated BAM bytes, found segment by segment, for the record-finder
// kernels (kernels_bam.hip) and for plain host C++ (tests/sanitize/bam_walk_harness.cpp).  The same functions run in both
// builds.  A chunk is `len` bytes behind a byte source B (B::at(i), 0 <= i < len); record starts are offsets into it.
//
// The chain is serial -- a record starts where the one before ends -- so the parallel form guesses a start in every
// segment (guess_segment), walks every segment from its guess (walk_segment), and goes through the segments in order with
// the true entry (stitch): only a walk that began at the true entry is kept, every other segment is walked again from it.
// The result is the serial chain's for every input; the guess decides the speed alone.
//
// Memory safety on arbitrary input: every at(i) has i < len (checked before each read), a list takes at most `cap`
// entries, and every loop advances by at least 36 bytes per trip or ends.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define RSI_BAM_HD __host__ __device__ inline
#else
#define RSI_BAM_HD inline
#endif

namespace rsibam {

constexpr uint32_t kNone = 0xffffffffu;            // no guess / no exit
constexpr uint32_t kMaxBlockSize = 8u << 20;       // plausibility: a record longer than this is never guessed
constexpr uint32_t kMinBlockSize = 32;             // the fixed fields behind block_size
enum Flag : uint32_t { kBeyond = 1, kBad = 2, kOpen = 4 };

// list entries a segment of `seg` bytes can need: a record has at least 36 bytes
RSI_BAM_HD uint32_t list_cap(uint32_t seg) { return seg / 36 + 1; }

struct Span {                                      // plain bytes
  const uint8_t* p;
  RSI_BAM_HD uint8_t at(uint64_t i) const { return p[i]; }
};

template <class B> RSI_BAM_HD uint32_t le32(const B& d, uint64_t off) {
  return (uint32_t)d.at(off) | ((uint32_t)d.at(off + 1) << 8) | ((uint32_t)d.at(off + 2) << 16) | ((uint32_t)d.at(off + 3) << 24);
}
template <class B> RSI_BAM_HD uint32_t le16(const B& d, uint64_t off) { return (uint32_t)d.at(off) | ((uint32_t)d.at(off + 1) << 8); }

// Could a record start at p?  Needs p + 4 <= len; the fixed fields are tested when the chunk holds them (p + 36 <= len), the
// name's last byte when the chunk holds it.  reflen[nref]: the header's reference lengths.
template <class B> RSI_BAM_HD bool plausible(const B& d, uint64_t len, uint64_t p, int32_t nref, const int32_t* reflen) {
  if (p + 4 > len) return false;
  const uint32_t bs = le32(d, p);
  if (bs < kMinBlockSize || bs > kMaxBlockSize) return false;
  if (p + 36 > len) return true;
  const int32_t refid = (int32_t)le32(d, p + 4), pos = (int32_t)le32(d, p + 8);
  if (refid < -1 || refid >= nref) return false;
  const uint32_t l_name = d.at(p + 12);
  if (l_name < 1) return false;
  const uint32_t n_cig = le16(d, p + 16);
  const int32_t l_seq = (int32_t)le32(d, p + 20);
  if (l_seq < 0) return false;
  if (32ull + l_name + 4ull * n_cig + ((uint64_t)l_seq + 1) / 2 + (uint64_t)l_seq > bs) return false;
  const int32_t next_refid = (int32_t)le32(d, p + 24);
  if (next_refid < -1 || next_refid >= nref) return false;
  if (pos < -1 || (refid >= 0 && pos >= reflen[refid])) return false;
  const uint64_t nul = p + 36 + l_name - 1;
  if (nul < len && d.at(nul) != 0) return false;
  return true;
}

// One hop of the chain from p: 0 and next / refid set for a whole record, else kBad (block_size < 32) or kOpen (the chunk
// ends inside the record, or inside its length field).
template <class B> RSI_BAM_HD uint32_t hop(const B& d, uint64_t len, uint64_t p, uint64_t& next, int32_t& refid) {
  if (p + 4 > len) return kOpen;
  const uint32_t bs = le32(d, p);
  if (bs < kMinBlockSize) return kBad;
  if (p + 4 + (uint64_t)bs > len) return kOpen;
  refid = (int32_t)le32(d, p + 4);
  next = p + 4 + (uint64_t)bs;
  return 0;
}

// The segment's guess: the lowest offset of [a, b) that is plausible and whose next two hops, as far as the chunk reaches,
// are plausible too (guess_chain tests one offset: the kernel shares a segment's offsets among its threads).
template <class B> RSI_BAM_HD bool guess_chain(const B& d, uint64_t len, uint64_t p, int32_t nref, const int32_t* reflen) {
  if (!plausible(d, len, p, nref, reflen)) return false;
  uint64_t q = p;
  for (int h = 0; h < 2; ++h) {
    q += 4 + (uint64_t)le32(d, q);
    if (q + 4 > len) return true;                  // the chunk reaches no further
    if (!plausible(d, len, q, nref, reflen)) return false;
  }
  return true;
}
template <class B> RSI_BAM_HD uint32_t guess_segment(const B& d, uint64_t len, uint64_t a, uint64_t b, int32_t nref, const int32_t* reflen) {
  for (uint64_t p = a; p < b; ++p) if (guess_chain(d, len, p, nref, reflen)) return (uint32_t)p;
  return kNone;
}

struct SegOut { uint32_t exit, listed, seen, flags; };

// The walk of a segment: from p, a record start, to the first record start at or beyond seg_end (<= len), the exit.  The
// starts of the records of `tid` go to list[0, cap); every whole record met counts as seen, the one that ends the file's
// part of `tid` (refid > tid or < 0: kBeyond, the walk stops AT it) included.  kBad and kOpen stop at the record they name.
template <class B> RSI_BAM_HD SegOut walk_segment(const B& d, uint64_t len, uint64_t p, uint64_t seg_end, int32_t tid, uint32_t* list, uint32_t cap) {
  SegOut o{0, 0, 0, 0};
  while (p < seg_end) {
    uint64_t next = 0;
    int32_t refid = 0;
    const uint32_t f = hop(d, len, p, next, refid);
    if (f) { o.flags |= f; break; }
    ++o.seen;
    if (refid == tid) { if (o.listed < cap) list[o.listed] = (uint32_t)p; ++o.listed; }
    else if (refid > tid || refid < 0) { o.flags |= kBeyond; break; }
    p = next;
  }
  o.exit = (uint32_t)p;
  return o;
}

struct Report {
  uint32_t listed;      // records of tid, whole, in rec_off[]
  uint32_t seen;        // whole records on the chain, the one that flagged kBeyond included
  uint32_t end;         // where the chain stopped: the end of the last whole record (the start of the kBeyond one)
  uint32_t flags;       // Flag bits of the segment the chain stopped in
  uint32_t guessed;     // segments accepted as guessed
  uint32_t rewalked;    // segments walked again from the true entry
  uint32_t passed;      // segments a long record covers: no record starts in them
  uint32_t pad;
};

// The ordered pass: segment s is [s * seg, min((s + 1) * seg, len)), nseg = ceil(len / seg); guess[s] and out[s] are what
// guess_segment and walk_segment(guess[s]) left, lists + s * cap the segment's list.  On return acc[s] is the number of list
// entries of segment s that belong to the chain (0 for a segment passed over, or behind the stop); out[s] and the list of
// a segment walked again are overwritten.  The pass may be taken in tiles of consecutive segments, the state carried from
// tile to tile: stitch_tile takes the segments [s0, s1), with guess, out and acc indexed from s0 (a tile's copies) and lists
// from segment 0.  acc may be guess itself (guess[s] is read before acc[s] is written).  One thread.
struct StitchState { uint64_t entry; uint32_t stopped; Report r; };
RSI_BAM_HD StitchState stitch_begin(uint64_t start) { return StitchState{start, 0, Report{0, 0, (uint32_t)start, 0, 0, 0, 0, 0}}; }
template <class B> RSI_BAM_HD void stitch_tile(const B& d, uint64_t len, uint32_t seg, uint32_t s0, uint32_t s1, int32_t tid, const uint32_t* guess,
                                               SegOut* out, uint32_t* lists, uint32_t cap, uint32_t* acc, StitchState& st) {
  for (uint32_t s = s0; s < s1; ++s) {
    const uint32_t k = s - s0;
    const uint32_t g = guess[k];
    acc[k] = 0;
    if (st.stopped) continue;
    const uint64_t b = ((uint64_t)s + 1) * seg < len ? ((uint64_t)s + 1) * seg : len;
    if (st.entry >= b) { ++st.r.passed; continue; }
    if (g == (uint32_t)st.entry) ++st.r.guessed;
    else { out[k] = walk_segment(d, len, st.entry, b, tid, lists + (size_t)s * cap, cap); ++st.r.rewalked; }
    const SegOut o = out[k];
    acc[k] = o.listed < cap ? o.listed : cap;
    st.r.listed += acc[k]; st.r.seen += o.seen;
    st.entry = o.exit;
    if (o.flags) { st.r.flags = o.flags; st.stopped = 1; }
  }
  st.r.end = (uint32_t)st.entry;
}
template <class B> RSI_BAM_HD Report stitch(const B& d, uint64_t len, uint64_t start, uint32_t seg, uint32_t nseg, int32_t tid, const uint32_t* guess,
                                            SegOut* out, uint32_t* lists, uint32_t cap, uint32_t* acc) {
  StitchState st = stitch_begin(start);
  stitch_tile(d, len, seg, 0, nseg, tid, guess, out, lists, cap, acc, st);
  return st.r;
}

}  // namespace rsibam
