// pairs_scan_device.h -- the tile scan of the insert-size sample, shared by the kernels that walk the pair table
// tile by tile: kernels_pairs.hip (the sample's stop and sums) and kernels_pin.hip (the sample's depth counts, 6m).
#pragma once
#include "kernels.h"
#include "bam_pairs_core.h"

namespace rsik {

constexpr int kPairThreads = 256;
constexpr int kPairItems = kPairSampleTile / kPairThreads;     // consecutive records per thread of a sample tile
static_assert(kPairItems * kPairThreads == kPairSampleTile, "a tile is whole threads");

// Inclusive scan of one Seg per thread under rsipairs::compose (not commutative: the left operand is the lower thread).  On
// return s[t] holds thread t's result too.
__device__ inline rsipairs::Seg pair_block_scan(rsipairs::Seg v, rsipairs::Seg* s) {
  const int t = threadIdx.x;
  s[t] = v;
  __syncthreads();
  for (int d = 1; d < kPairThreads; d <<= 1) {
    const rsipairs::Seg a = t >= d ? s[t - d] : rsipairs::seg_none();
    __syncthreads();
    if (t >= d) { v = rsipairs::compose(a, v); s[t] = v; }
    __syncthreads();
  }
  return v;
}

// the kept records among a thread's kPairItems, joined
__device__ inline rsipairs::Seg pair_thread_seg(const PairTable& t, long long i0, long long n) {
  rsipairs::Seg v = rsipairs::seg_none();
  for (int k = 0; k < kPairItems; ++k) {
    const long long i = i0 + k;
    if (i < n && rsipairs::sample_kept(t.pos[i], t.rend[i], t.info[i])) v = rsipairs::compose(v, rsipairs::seg_one(t.pos[i]));
  }
  return v;
}

// the first entry of the table (ascending in pos) whose pos is not below key
__device__ inline uint32_t lower_bound_pos(const int32_t* __restrict__ pos, uint32_t n, long long key) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if ((long long)pos[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

}  // namespace rsik
