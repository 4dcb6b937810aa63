// kernels_depth.hip -- `rsicnv depth` on the device: what a chromosome's per-base depth int32[n] in HBM says about
// itself, without a run.
//   k_depth_summary       one pass: exact sum, minimum, maximum, the count of depths above 65535, the count of negative ones and
//                         the 65536-bin distribution.  Depths below kDepthSplit are counted in LDS, kDepthCopies counters per value
//                         (at 30x nearly all bases carry a few dozen values: one counter per value would serialise the wave on
//                         them); the others go to the global bins with integer atomicAdd.  A workgroup takes one span of the array
//                         and folds its non-zero LDS bins into the global ones at its end.
//   k_depth_window_table  the (start, end, 0) triples of a slice of consecutive windows of W bases
//   k_depth_windows       their sums: a workgroup stages its span of the slice in LDS, every thread walks a chunk of it and adds
//                         a partial sum wherever a window ends; windows that span workgroups meet in the slice's sum array.
// Everything that counts is an integer atomic, so a result does not depend on the order of arrival: the same input gives the same
// bytes.  The kernel boundary is the only synchronisation between workgroups.  The explicit regions of `-by FILE` take geno's
// k_geno_init32 / k_geno_minmax32 (kernels_geno.hip); the lines of both are formatted by kernels_track.hip's third mode.
#include <algorithm>
#include "kernels.h"

namespace rsik {

namespace {

constexpr int kT = kDepthThreads;
constexpr int kWaves = kT / 64;
constexpr int kStride = kDepthSplit + 1;   // a copy's counters: copy c of value v lies in bank (c + v) mod 32, so the copies of one
                                           // value -- what a flat stretch of depth hits -- spread over kDepthCopies banks
static_assert((kDepthCopies & (kDepthCopies - 1)) == 0 && kDepthCopies <= 32, "a thread finds its copy with a mask");
static_assert(kDepthSplit % kT == 0, "the fold gives every thread whole bins");

__global__ __launch_bounds__(kT) void k_depth_summary(const int32_t* __restrict__ d, long long n, long long span, DepthAcc* __restrict__ acc,
                                                      unsigned int* __restrict__ dist) {
  __shared__ unsigned int h[kDepthCopies * kStride];
  __shared__ long long s_sum[kWaves];
  __shared__ int32_t s_min[kWaves], s_max[kWaves];
  __shared__ unsigned int s_over[kWaves], s_neg[kWaves];
  const long long b0 = (long long)blockIdx.x * span;
  if (b0 >= n) return;
  const long long len = min(span, n - b0);
  for (int i = threadIdx.x; i < kDepthCopies * kStride; i += kT) h[i] = 0;
  __syncthreads();
  unsigned int* mine = h + (threadIdx.x & (kDepthCopies - 1)) * kStride;
  long long sum = 0;
  int32_t lo = 0x7fffffff, hi = (int32_t)0x80000000;
  unsigned int over = 0, neg = 0;
  // k bases of depth v.  A negative depth indexes nothing and enters nothing but its own count
  auto count = [&](int32_t v, unsigned int k) {
    if (v < 0) { neg += k; return; }
    sum += (long long)v * k;
    lo = min(lo, v); hi = max(hi, v);
    if (v < kDepthSplit) { atomicAdd(&mine[v], k); return; }
    if (v >= kDepthBins) { over += k; v = kDepthBins - 1; }
    atomicAdd(&dist[v], k);
  };
  const int32_t* p = d + b0;
  const long long head = min(len, (long long)(((16 - ((uintptr_t)p & 15)) & 15) >> 2));   // values in front of the first aligned 16 bytes
  const long long nq = (len - head) >> 2, tail = len - head - 4 * nq;
  if ((long long)threadIdx.x < head) count(p[threadIdx.x], 1u);
  const int4* w = reinterpret_cast<const int4*>(p + head);
  for (long long i = threadIdx.x; i < nq; i += kT) {
    const int4 x = w[i];
    if (x.x == x.y && x.y == x.z && x.z == x.w) count(x.x, 4u);   // flat depth is the common case: one add for the four
    else { count(x.x, 1u); count(x.y, 1u); count(x.z, 1u); count(x.w, 1u); }
  }
  if ((long long)threadIdx.x < tail) count(p[head + 4 * nq + threadIdx.x], 1u);

  for (int k = 32; k > 0; k >>= 1) {
    sum += __shfl_down(sum, k, 64);
    lo = min(lo, __shfl_down(lo, k, 64)); hi = max(hi, __shfl_down(hi, k, 64));
    over += __shfl_down(over, k, 64); neg += __shfl_down(neg, k, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    const int wv = threadIdx.x >> 6;
    s_sum[wv] = sum; s_min[wv] = lo; s_max[wv] = hi; s_over[wv] = over; s_neg[wv] = neg;
  }
  __syncthreads();   // the waves' partial results, and every count in h
  for (int b = threadIdx.x; b < kDepthSplit; b += kT) {
    unsigned int c = 0;
    for (int k = 0; k < kDepthCopies; ++k) c += h[k * kStride + b];
    if (c) atomicAdd(&dist[b], c);
  }
  if (threadIdx.x == 0) {
    for (int k = 1; k < kWaves; ++k) { sum += s_sum[k]; lo = min(lo, s_min[k]); hi = max(hi, s_max[k]); over += s_over[k]; neg += s_neg[k]; }
    if (sum) atomicAdd(&acc->sum, (unsigned long long)sum);
    if (lo <= hi) { atomicMin(&acc->vmin, lo); atomicMax(&acc->vmax, hi); }   // (a span of negative depths alone has none)
    if (over) atomicAdd(&acc->over, (unsigned long long)over);
    if (neg) atomicAdd(&acc->negative, (unsigned long long)neg);
  }
}

__global__ __launch_bounds__(kT) void k_depth_window_table(long long w0, long long w1, long long W, long long n, long long* __restrict__ start,
                                                           long long* __restrict__ end, unsigned long long* __restrict__ sum) {
  const long long k = w0 + (long long)blockIdx.x * kT + threadIdx.x;
  if (k >= w1) return;
  start[k - w0] = k * W;
  end[k - w0] = min(n, (k + 1) * W);
  sum[k - w0] = 0ull;
}

constexpr int kLdsWindows = 512;                      // windows a workgroup sums in LDS; a span that meets more adds straight to HBM
__device__ inline int staged(int i) { return i + (i >> 5); }   // a pad word per 32: the threads' chunks start in different banks

__global__ __launch_bounds__(kT) void k_depth_windows(const int32_t* __restrict__ d, long long n, long long W, long long w0, long long w1, int span,
                                                      unsigned long long* __restrict__ sum) {
  __shared__ int32_t tile[kWindowSpan + kWindowSpan / 32 + 1];
  __shared__ unsigned long long ws[kLdsWindows];
  const long long stop = min(n, w1 * W);
  const long long b0 = w0 * W + (long long)blockIdx.x * span;
  if (b0 >= stop) return;
  const int len = (int)min((long long)span, stop - b0);
  const long long kf = b0 / W, kl = (b0 + len - 1) / W;   // the first and the last window this span meets
  const long long nw = kl - kf + 1;
  const bool local = nw <= kLdsWindows;
  if (local) for (int j = threadIdx.x; j < (int)nw; j += kT) ws[j] = 0ull;
  for (int i = threadIdx.x; i < len; i += kT) tile[staged(i)] = d[b0 + i];
  __syncthreads();
  const int chunk = (span + kT - 1) / kT;
  const int i0 = min(len, (int)threadIdx.x * chunk), i1 = min(len, i0 + chunk);
  if (nw == 1) {   // one window over the whole span: one add per wave
    long long s = 0;
    for (int i = i0; i < i1; ++i) s += tile[staged(i)];
    for (int k = 32; k > 0; k >>= 1) s += __shfl_down(s, k, 64);
    if ((threadIdx.x & 63) == 0 && s) atomicAdd(&ws[0], (unsigned long long)s);
  } else if (i0 < i1) {
    long long k = (b0 + i0) / W;
    long long next = (k + 1) * W - b0;   // where window k ends, as an index into the span
    long long s = 0;
    auto flush = [&]() {
      if (!s) return;
      if (local) atomicAdd(&ws[k - kf], (unsigned long long)s);   // two's complement: exact for any signs
      else atomicAdd(&sum[k - w0], (unsigned long long)s);
    };
    for (int i = i0; i < i1; ++i) {
      if (i == next) { flush(); s = 0; ++k; next += W; }
      s += tile[staged(i)];
    }
    flush();
  }
  if (!local) return;
  __syncthreads();
  for (int j = threadIdx.x; j < (int)nw; j += kT) { const unsigned long long v = ws[j]; if (v) atomicAdd(&sum[kf - w0 + j], v); }
}

}  // namespace

void launch_depth_summary(const int32_t* d, long long n, long long span, DepthAcc* acc, unsigned int* dist, hipStream_t stream) {
  if (n <= 0 || span <= 0) return;
  RSI_LAUNCH(k_depth_summary, dim3((unsigned)((n + span - 1) / span)), dim3(kT), 0, stream, d, n, span, acc, dist);
}

void launch_depth_window_table(long long w0, long long w1, long long W, long long n, long long* start, long long* end, unsigned long long* sum,
                               hipStream_t stream) {
  if (w1 <= w0) return;
  RSI_LAUNCH(k_depth_window_table, dim3((unsigned)((w1 - w0 + kT - 1) / kT)), dim3(kT), 0, stream, w0, w1, W, n, start, end, sum);
}

void launch_depth_windows(const int32_t* d, long long n, long long W, long long w0, long long w1, int span, unsigned long long* sum,
                          hipStream_t stream) {
  const long long bases = std::min(n, w1 * W) - w0 * W;
  if (bases <= 0 || span < 1 || span > kWindowSpan) return;
  RSI_LAUNCH(k_depth_windows, dim3((unsigned)((bases + span - 1) / span)), dim3(kT), 0, stream, d, n, W, w0, w1, span, sum);
}

}  // namespace rsik
