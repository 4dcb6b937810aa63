// per_base_device.h -- small device-side helpers shared by the per-base kernel files (kernels_base.hip, kernels_k4s.hip):
// byte tests, quad sums without the LDS pipeline, window GC counts on staged mask words, the float form of the GC rescale,
// and what the K4 forms (K4, K4', K4w, K4j, K4s, K4m) have in common: the removed-region table and its staging, the tile
// geometry, the per-element walk over the source segments between removed regions, the value K3 would have left at a source
// index, and the packed counting medians.  Each translation unit gets its own copy (anonymous namespace).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kernels.h"
#include "device_util.h"

#if defined(__HIPCC__)
namespace rsik {
namespace {

constexpr int kFixShift = 22;   // fraction bits of the fixed-point ratios K2j verifies and K4j / K4s rescale with

__device__ inline int lane_id() { return threadIdx.x & 63; }
__device__ inline bool has_escape(uint32_t w) {   // any byte of w equal to 0xff
  const uint32_t x = ~w;                          // a zero byte of x
  return ((x - 0x01010101u) & ~x & 0x80808080u) != 0;
}


// Sum over the 2, 4, 8 or 16 consecutive lanes that share a bin (the median phases of K4' / K4j): neighbours at distance 1 and 2
// through DPP quad permutes -- one VALU instruction each -- instead of ds_bpermute, which goes through the LDS pipeline and whose
// latency sat seven times two deep in every bin's bisection.
__device__ inline int dpp_xor1(int x) { return __builtin_amdgcn_update_dpp(0, x, 0xB1, 0xF, 0xF, true); }   // quad_perm [1, 0, 3, 2]
__device__ inline int dpp_xor2(int x) { return __builtin_amdgcn_update_dpp(0, x, 0x4E, 0xF, 0xF, true); }   // quad_perm [2, 3, 0, 1]
__device__ inline int parts_sum(int x, int parts) {
  x += dpp_xor1(x);
  if (parts > 2) x += dpp_xor2(x);
  for (int d = 4; d < parts; d <<= 1) x += __shfl_xor(x, d);
  return x;
}
__device__ inline uint64_t dpp_xor1_u64(uint64_t x) { return (uint64_t)(uint32_t)dpp_xor1((int)(uint32_t)x) | ((uint64_t)(uint32_t)dpp_xor1((int)(uint32_t)(x >> 32)) << 32); }
__device__ inline uint64_t dpp_xor2_u64(uint64_t x) { return (uint64_t)(uint32_t)dpp_xor2((int)(uint32_t)x) | ((uint64_t)(uint32_t)dpp_xor2((int)(uint32_t)(x >> 32)) << 32); }

// the same two queries on a plain array of staged words (a workgroup's tile in K4j)
__device__ inline uint32_t gcw_window(const uint64_t* __restrict__ word, uint32_t rel) {
  const uint32_t k = rel >> 6, b = rel & 63;
  const uint64_t w0 = word[k], w1 = word[k + 1], w2 = word[k + 2], w3 = word[k + 3], w4 = word[k + 4];
  const uint32_t rem = 9 + b;
  const uint64_t m3 = rem >= 64 ? ~0ull : ((1ull << rem) - 1);
  const uint64_t m4 = rem > 64 ? ((1ull << (rem - 64)) - 1) : 0ull;
  return (uint32_t)(__popcll(w0 >> b) + __popcll(w1) + __popcll(w2) + __popcll(w3 & m3) + __popcll(w4 & m4));
}
__device__ inline uint32_t gcw_field16(const uint64_t* __restrict__ word, uint32_t rel) {
  const uint32_t k = rel >> 6, b = rel & 63;
  uint64_t v = word[k] >> b;
  if (b > 48) v |= word[k + 1] << (64 - b);
  return (uint32_t)v & 0xffffu;
}

// The GC rescale without a division -- or any double arithmetic -- per base (f64 runs at half rate on gfx950, its
// conversions at a quarter).  The reference's expression is (int)((double)d * rdmean / table[g] + 0.5) (gccontent.cpp:89:
// product, IEEE division, truncation).  With ratio = (float)(rdmean / table[g]), f = fma((float)d, ratio, 0.5f) is within
// 2^-23 (t + 0.5) of the reference's t + 0.5 (one rounding in the ratio, one in the fma; d < 2^24 is exact), so
// floor(f) equals the reference's result unless f lies within tol = 2.5e-7 f + 1e-6 (twice that bound) of an integer.
// Those bases raise `unsure` and the caller redoes them with the reference's own double expression: the result is the
// reference's in every case; only one base in ten thousand takes the slow way.
__device__ inline float rescale_f32(float d, float ratio, bool& unsure) {
  const float f = __fmaf_rn(d, ratio, 0.5f);
  const float fl = floorf(f);
  const float fr = f - fl;
  const float tol = __fmaf_rn(f, 2.5e-7f, 1.0e-6f);
  unsure |= fabsf(fr - 0.5f) > 0.5f - tol;
  return fl;
}

constexpr int kRegLds = 128;   // removed regions mirrored in LDS (the list is short; more stay in HBM; 128: K4j keeps four workgroups per CU with its 24 KB histogram)

struct RegionTable {
  const int64_t* cbreak; const int64_t* cum; int nreg;
  int64_t* s_break; int64_t* s_cum;   // LDS mirror of the first kRegLds entries (+1 for cum)
  __device__ int64_t brk(int k) const { return k < kRegLds ? s_break[k] : cbreak[k]; }
  __device__ int64_t shift(int k) const { return k <= kRegLds ? s_cum[k] : cum[k]; }
};

// #GC in [lo, lo + 201) straight from the mask in HBM (per-element path only)
__device__ inline int gc_count201(const uint64_t* __restrict__ gcbits, int64_t lo) {
  int c = 0;
  int64_t p = lo;
  const int64_t end = lo + 201;
  while (p < end) {
    const int64_t w = p >> 6;
    const int b = (int)(p & 63);
    int take = 64 - b;
    if (p + take > end) take = (int)(end - p);
    uint64_t x = gcbits[w] >> b;
    if (take < 64) x &= (1ull << take) - 1;
    c += __popcll(x);
    p += take;
  }
  return c;
}

struct __attribute__((packed, aligned(1))) Bytes16 { uint32_t x, y, z, w; };   // 16 bytes at any byte address (gfx950 loads them in one go)

// ------------------------------------------------------------------------------------------
// What the K4 forms share.  Everything below is forced inline: a kernel that calls it compiles to what it did with the
// code written out in its body (profiles/r7_k4_resources_*.txt).
#define RSI_K4_INLINE __device__ __forceinline__

// The removed-region list into its LDS mirror (s_break[kRegLds], s_cum[kRegLds + 1]; the caller's barrier completes it).
// A list of up to kRegInline entries travels with the kernel arguments -- no upload in front of the launch -- unless the
// launch was queued before the host knew the list (`use_inline` false: K4j / K4s behind K2j); a longer one comes from device
// memory, its first kRegLds entries mirrored.
RSI_K4_INLINE void stage_regions(int64_t* s_break, int64_t* s_cum, int nreg, const K4Regions inl /* by value: the kernel's argument block itself once inlined, no generic pointer to it */,
                                 const int64_t* __restrict__ cbreak, const int64_t* __restrict__ cum, bool use_inline, int nthreads) {
  if (nreg <= kRegInline && use_inline) {
    for (int e = threadIdx.x; e < nreg; e += nthreads) s_break[e] = inl.brk[e];
    for (int e = threadIdx.x; e <= nreg; e += nthreads) s_cum[e] = inl.cum[e];
  } else {
    for (int e = threadIdx.x; e < kRegLds && e < nreg; e += nthreads) s_break[e] = cbreak[e];
    for (int e = threadIdx.x; e <= kRegLds && e <= nreg; e += nthreads) s_cum[e] = cum[e];
  }
}

// Tile geometry.  Compaction is a piecewise shift: compacted index p maps to source index p + shift(k), k = number of removed
// regions with brk <= p.  The tile [P0, P1) of `tile_elems` compacted positions is `plain` when no region cuts it -- one
// contiguous source range that begins at soff; k (the caller's, kept between calls: tiles are visited in increasing order)
// moves past the breaks at or before P0.
template <typename Regions>
RSI_K4_INLINE void tile_geometry(const Regions& R, int nreg, int& k, int64_t tile, int tile_elems, int64_t ncompact, int64_t& P0, int64_t& P1,
                                 bool& plain, int64_t& soff) {
  P0 = tile * tile_elems;
  P1 = (P0 + tile_elems < ncompact) ? P0 + tile_elems : ncompact;
  while (k < nreg && R.brk(k) <= P0) ++k;
  plain = (k >= nreg) || (R.brk(k) >= P1);
  soff = P0 + R.shift(k);
}

// The per-element path of a tile that a region cuts (or that a form's fast path does not take): the contiguous source segments
// between the removed regions, their elements dealt out to the workgroup's threads.  f(source index, compacted index, index
// within the tile), k as tile_geometry left it.
template <typename Regions, typename F>
RSI_K4_INLINE void for_each_tile_element(const Regions& R, int k, int nreg, int64_t P0, int64_t P1, int nthreads, F f) {
  int kk = k;
  int64_t seg = P0;
  while (seg < P1) {
    const int64_t nxt = (kk < nreg && R.brk(kk) < P1) ? R.brk(kk) : P1;
    const int64_t len = nxt - seg;
    if (len > 0) {
      const int64_t so = seg + R.shift(kk);
      const int dst = (int)(seg - P0);
      for (int64_t e = threadIdx.x; e < len; e += nthreads) f(so + e, seg + e, dst + e);
    }
    seg = nxt;
    if (kk < nreg && R.brk(kk) == nxt) ++kk;
  }
}

// The value K3 and its tail fix-up would have left at source index i, for the byte forms' per-element paths (K4', K4j), from
// the int32 depth with the reference's own expression (gccontent.cpp:89: product, IEEE division, truncation): clamped windows
// at the chromosome's ends (App. A Q1), and the 20-slice write-back's tail (App. A Q2/Q3) -- cells n-201 .. n-201+r-1 carry the
// rescaled depth of the last r bases, computed with the fresh edge window [n-201, n-1]; the last r bases keep their raw depth.
// raw: the bytes are the raw depth (-NOGC), no rescale and no quirks.
struct SlowSource {
  const int32_t* depth; const uint64_t* gcbits; int64_t n, S20, r20;   // S20 = n / 20, r20 = n - 20 S20
  const double* table /* [kGcLevels], in LDS */; double rdmean;
  __device__ int rescale(int d, uint32_t g) const { return (int)((double)d * rdmean / table[g] + 0.5); }
};
RSI_K4_INLINE int slow_value(const SlowSource& S, int64_t i, bool raw) {
  if (raw) return S.depth[i];
  if (S.r20 >= 2 && i >= S.n - 201 && i < S.n - 201 + S.r20) return S.rescale(S.depth[20 * S.S20 + (i - (S.n - 201))], (uint32_t)gc_count201(S.gcbits, S.n - 201));
  if (i >= 20 * S.S20) return S.depth[i];
  int64_t lo = i - 100;
  if (lo < 0) lo = 0;
  if (lo > S.n - 202) lo = S.n - 202;
  return S.rescale(S.depth[i], (uint32_t)gc_count201(S.gcbits, lo));
}

// ---- the packed counting median ----
// The median of a bin is its order statistic kth = (m + 1) / 2 (m odd, rsi.cpp:2061): the smallest t with #{x <= t} >= kth,
// found by bisection on t with a count over the bin's values held several to a register.  The guard-bit trick: with the top
// bit of every field set, (x | guard) - (t + 1) keeps that bit exactly where x > t, and no field borrows from its neighbour --
// #{x > t} of a register is one subtraction and one popcount.  Slots outside the bin hold all ones, above every t, and are
// taken off the count as a constant.
//
// bisect_kth: `count_le(t)` = #{x <= t} of the lane's bin, summed over the bin's lanes; every value is in 0 .. capval.
// Without BRACKET: STEPS steps from [0, capval], the same for every bin.  With it: the median of a bin lies next to its mean, so
// the 2 HALF + 2 values around `est` = sum / m bracket it on all but a handful of bins (event edges); the two counts that prove
// it (the median is not below the bracket, nor above it) and STEPS_IN steps inside replace the STEPS.  A wave with a bin outside
// its bracket takes the STEPS from [0, capval]: the result is the same either way, whatever the guess.  TOP: the largest t the
// fields can be asked about.
template <bool BRACKET, int HALF, int TOP, int STEPS, int STEPS_IN, typename F>
RSI_K4_INLINE int bisect_kth(F count_le, int est, int kth, int capval, bool active) {
  int lo = 0, hi = capval, steps = STEPS;
  if (BRACKET) {
    int lo0 = est - HALF;
    lo0 = lo0 < 0 ? 0 : lo0;
    int hi0 = lo0 + 2 * HALF + 1;
    hi0 = hi0 > capval ? capval : hi0;
    lo0 = lo0 > hi0 ? hi0 : lo0;
    const bool below = count_le(lo0 - 1) < kth;
    const bool above = hi0 >= capval || count_le(hi0 > TOP ? TOP : hi0) >= kth;   // (every value is <= capval)
    if (__all((below && above) || !active)) { lo = lo0; hi = hi0; steps = STEPS_IN; }
  }
#pragma unroll 1
  for (int it = 0; it < steps; ++it) {
    const int mid = (lo + hi) >> 1;
    const int le = count_le(mid);
    if (lo < hi) { if (le >= kth) hi = mid; else lo = mid + 1; }
  }
  return lo;
}

// Bytes (caps below kByteSat; K4', K4j, K4m): a lane holds seven dwords of its bin.  SW7 (cap <= 127, a byte has a spare bit):
// four values to a register, bit 7 of every byte as the guard.  Else (caps of 128 .. 253): the same scheme on 16-bit fields, two
// values to a register -- bytes 0 and 2 of a dword in xa, bytes 1 and 3 in xc, bit 15 of every field as the guard; #{x > t} of
// four values is then two subtractions and two popcounts.
template <bool SW7> struct BinBytes {
  uint32_t xa[7], xc[SW7 ? 1 : 7];
  // dword i of the lane; xb: its four bytes, those outside the bin set to 0xff
  RSI_K4_INLINE void set(int i, uint32_t xb) {
    if (SW7) xa[i] = xb | 0x80808080u;
    else { xa[i] = (xb & 0x00ff00ffu) | 0x80008000u; xc[i] = ((xb >> 8) & 0x00ff00ffu) | 0x80008000u; }
  }
  // #{x <= t} of the bin, t = -1 .. 126 (252): masked bytes always count as "> t" -- 28 byte slots per lane, minus the bin's m, over the bin's lanes
  RSI_K4_INLINE int count_le(int t, int parts) const {
    int gt = 0;
    if (SW7) {
      const uint32_t sub = (uint32_t)(t + 1) * 0x01010101u;
#pragma unroll
      for (int i = 0; i < 7; ++i) gt += __popc((xa[i] - sub) & 0x80808080u);
    } else {
      const uint32_t sub = (uint32_t)(t + 1) * 0x00010001u;
#pragma unroll
      for (int i = 0; i < 7; ++i) gt += __popc((xa[i] - sub) & 0x80008000u) + __popc((xc[i] - sub) & 0x80008000u);
    }
    return 4 * 7 * parts - parts_sum(gt, parts);
  }
  // The bin's median.  Bracket of eight (sixteen: deeper coverage, wider bins of values) around the mean, three (four) steps
  // inside it, seven (eight) from [0, cap].  inv_m = 1 / m is read with BRACKET only.
  template <bool BRACKET>
  RSI_K4_INLINE int median(uint32_t ssum, float inv_m, int kth, int capval, bool active, int parts) const {
    return bisect_kth<BRACKET, SW7 ? 3 : 7, SW7 ? 126 : 252, SW7 ? 7 : 8, SW7 ? 3 : 4>([&](int t) { return count_le(t, parts); },
                                                                                  BRACKET ? (int)((float)ssum * inv_m) : 0, kth, capval, active);
  }
};

// The bin [B, B + m) of a tile of bytes in LDS (K4', K4j) into X: its (up to 27) dwords go round robin to the bin's `parts`
// threads, bytes outside the bin masked -- to 0 for the sum (v_sad_u8 adds four bytes in one instruction), to 0xff for the
// counts.  Returns the bin's sum (every lane of the bin has it).
template <bool SW7>
RSI_K4_INLINE uint32_t load_bin_bytes(const unsigned char* s_val, int B, int m, int part, int parts, bool active, BinBytes<SW7>& X) {
  const int d0 = B >> 2, d1 = (B + m - 1) >> 2;
  const uint32_t* w = reinterpret_cast<const uint32_t*>(s_val);
  uint32_t ssum = 0;
#pragma unroll
  for (int i = 0; i < 7; ++i) {
    const int d = d0 + part + parts * i;
    const uint32_t v = w[d <= d1 ? d : d1];
    const int lo_cut = B - 4 * d, hi_cut = 4 * d + 4 - (B + m);          // bytes of the dword before / after the bin
    uint32_t keep = 0xffffffffu;
    keep = lo_cut > 0 ? keep << (8 * lo_cut) : keep;
    keep = hi_cut > 0 ? keep & (0xffffffffu >> (8 * hi_cut)) : keep;
    keep = (d <= d1 && active) ? keep : 0u;
    ssum = __builtin_amdgcn_sad_u8(v & keep, 0u, ssum);
    X.set(i, v | ~keep);
  }
  return (uint32_t)parts_sum((int)ssum, parts);
}

// 16-bit fields (caps below 2^15; K4's registers from an int32 tile, K4w's masked dwords of a 16-bit tile): N registers of two
// values per lane, bit 15 of each field as the guard, slots outside the bin 0xffff.  #{x <= t} of the bin, t = -1 .. 32766.
template <int N>
RSI_K4_INLINE int count_le16(const uint32_t (&x)[N], int t, int parts) {
  const uint32_t sub = (uint32_t)(t + 1) * 0x00010001u;
  int gt = 0;
#pragma unroll
  for (int i = 0; i < N; ++i) gt += __popc((x[i] - sub) & 0x80008000u);
  return 2 * N * parts - parts_sum(gt, parts);
}
// The bin's median: 64 values around the bin's mean bracket it, six steps inside, fifteen from [0, cap].  32-bit sums: m * cap
// stays below 2^31.
template <int N>
RSI_K4_INLINE int median16(const uint32_t (&x)[N], uint32_t ssum, int m, int kth, int capval, bool active, int parts) {
  return bisect_kth<true, 31, 32766, 15, 6>([&](int t) { return count_le16(x, t, parts); }, (int)((float)ssum / (float)m), kth, capval, active);
}

}  // namespace
}  // namespace rsik
#endif
