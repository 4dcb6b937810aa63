// kernels_pairs.hip -- the RP / Q0 annotation of a BAM run on the device.  k_bam_pairs keeps, beside the pileup,
// the few words per read the annotation looks at (the pair table); the k_pair_sample_* kernels compute the insert-size sample
// over it as a segmented scan (tile summaries, one workgroup over the summaries, first stop per tile, masked sum);
// k_pairs_annotate counts, one workgroup per call, the reads of the call's window.  The per-record logic is
// bam_pairs_core.h's, the host harness's own.
#include "kernels.h"
#include "bam_pairs_core.h"
#include "pairs_scan_device.h"

namespace rsik {

namespace {

using rsipairs::Seg;

__global__ __launch_bounds__(kPairThreads) void k_bam_pairs(const uint8_t* __restrict__ data, const uint32_t* __restrict__ rec_off, int nrec, int tid,
                                                            long long base, PairTable t, int32_t* __restrict__ words, int parity) {
  const int i = blockIdx.x * kPairThreads + threadIdx.x;
  if (i >= nrec) return;
  const rsibam::Span d{data};
  const uint64_t off = rec_off[i];
  bool overrun = false;
  const rsipairs::Entry e = rsipairs::extract(d, off, tid, overrun);
  const long long k = base + i;
  t.pos[k] = e.pos; t.rend[k] = e.rend; t.mpos[k] = e.mpos; t.isize[k] = e.isize; t.info[k] = e.info;
  // the predecessor's pos: the record before in this chunk, or the one the launch before left
  const int32_t prev = i > 0 ? (int32_t)rsipairs::rd32(d, (uint64_t)rec_off[i - 1] + 8) : words[2 + parity];
  uint32_t f = 0;
  if (e.pos < prev) f |= rsipairs::kUnsorted;
  if (overrun) f |= rsipairs::kOverrun;
  if (f) atomicOr(reinterpret_cast<unsigned int*>(words + 1), f);
  const int32_t span = (int32_t)min((long long)e.rend - (long long)e.pos, (long long)INT32_MAX);
  if (span > *(volatile int32_t*)words) atomicMax(words, span);      // (the plain read only spares atomics: the word only grows)
  if (i == nrec - 1) words[2 + (parity ^ 1)] = e.pos;
}

__global__ __launch_bounds__(kPairThreads) void k_pair_sample_tiles(PairTable t, long long n, Seg* __restrict__ tile_sum) {
  __shared__ Seg s[kPairThreads];
  const long long i0 = (long long)blockIdx.x * kPairSampleTile + (long long)threadIdx.x * kPairItems;
  const Seg v = pair_block_scan(pair_thread_seg(t, i0, n), s);
  if (threadIdx.x == kPairThreads - 1) tile_sum[blockIdx.x] = v;
}

// One workgroup: tile_pre[b] = the tiles before b joined.  Also clears the stop word and the sums.
__global__ __launch_bounds__(kPairThreads) void k_pair_sample_scan(const Seg* __restrict__ tile_sum, long long ntiles, Seg* __restrict__ tile_pre,
                                                                   unsigned int* __restrict__ stop, unsigned long long* __restrict__ out) {
  __shared__ Seg s[kPairThreads];
  const int t = threadIdx.x;
  if (t == 0) *stop = 0xffffffffu;
  if (t < 4) out[t] = 0;
  Seg carry = rsipairs::seg_none();
  for (long long c0 = 0; c0 < ntiles; c0 += kPairThreads) {
    const long long b = c0 + t;
    pair_block_scan(b < ntiles ? tile_sum[b] : rsipairs::seg_none(), s);
    if (b < ntiles) tile_pre[b] = rsipairs::compose(carry, t ? s[t - 1] : rsipairs::seg_none());
    carry = rsipairs::compose(carry, s[kPairThreads - 1]);
    __syncthreads();
  }
}

// The first stopping record of every tile; the lowest table index of all goes to *stop.
__global__ __launch_bounds__(kPairThreads) void k_pair_sample_stop(PairTable t, long long n, long long tid_len, const Seg* __restrict__ tile_pre,
                                                                   unsigned int* __restrict__ stop) {
  __shared__ Seg s[kPairThreads];
  const long long i0 = (long long)blockIdx.x * kPairSampleTile + (long long)threadIdx.x * kPairItems;
  pair_block_scan(pair_thread_seg(t, i0, n), s);
  Seg p = rsipairs::compose(tile_pre[blockIdx.x], threadIdx.x ? s[threadIdx.x - 1] : rsipairs::seg_none());
  for (int k = 0; k < kPairItems; ++k) {
    const long long i = i0 + k;
    if (i >= n) break;
    const int32_t pos = t.pos[i], rend = t.rend[i];
    const uint32_t info = t.info[i];
    if (!rsipairs::sample_kept(pos, rend, info)) continue;
    p = rsipairs::compose(p, rsipairs::seg_one(pos));
    if (rsipairs::sample_stops(p, pos, rend, info, tid_len)) { atomicMin(stop, (unsigned int)i); break; }
  }
}

__device__ inline unsigned long long wave_sum(unsigned long long v) {
  for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
  return v;
}

// The sums over the kept records up to and including *stop.  Integer sums: equal to bam_pair_sample's double sums wherever
// those are exact (|sum| < 2^53), and the same from run to run.
__global__ __launch_bounds__(kPairThreads) void k_pair_sample_sum(PairTable t, long long n, const unsigned int* __restrict__ stop,
                                                                  unsigned long long* __restrict__ out) {
  __shared__ unsigned long long s_part[kPairThreads / 64][4];
  const unsigned int st = *stop;
  const long long last = st == 0xffffffffu ? n - 1 : (long long)st;
  unsigned long long acc[4] = {0, 0, 0, 0};
  for (long long i = (long long)blockIdx.x * kPairThreads + threadIdx.x; i <= last; i += (long long)gridDim.x * kPairThreads) {
    const uint32_t info = t.info[i];
    if (!rsipairs::sample_kept(t.pos[i], t.rend[i], info)) continue;
    acc[3] += 1;
    if (rsipairs::sample_summed(info)) {
      const int32_t is = t.isize[i];
      acc[0] += 1;
      acc[1] += (unsigned long long)rsipairs::isize_abs(is);
      acc[2] += (unsigned long long)(long long)rsipairs::isize_square(is);
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int k = 0; k < 4; ++k) { const unsigned long long v = wave_sum(acc[k]); if (lane == 0) s_part[wave][k] = v; }
  __syncthreads();
  if (threadIdx.x < 4) {
    unsigned long long v = 0;
    for (int w = 0; w < kPairThreads / 64; ++w) v += s_part[w][threadIdx.x];
    if (v) atomicAdd(out + threadIdx.x, v);
  }
}

__global__ __launch_bounds__(kPairThreads) void k_pairs_annotate(PairTable t, uint32_t n, int maxspan, const rsipairs::Call* __restrict__ calls,
                                                                 int isize_mean, int isize_sd, uint32_t* __restrict__ out) {
  __shared__ uint32_t s_part[kPairThreads / 64][3];
  const rsipairs::Call c = calls[blockIdx.x];
  // a read that reaches p1e begins above p1e - maxspan; one that begins at p2e or later is not read
  const uint32_t lo = lower_bound_pos(t.pos, n, (long long)c.p1e - (long long)maxspan);
  const uint32_t hi = lower_bound_pos(t.pos, n, (long long)c.p2e);
  uint32_t q0_all = 0, q0_q0 = 0, rp = 0;
#pragma unroll 1   // (unrolled, even twice, the branchy body takes all 256 VGPRs -- one wave per SIMD; as it stands 66)
  for (uint32_t i = lo + threadIdx.x; i < hi; i += kPairThreads) {
    const uint32_t v = rsipairs::decide(c, t.pos[i], t.rend[i], t.mpos[i], t.info[i], isize_mean, isize_sd);
    q0_all += (v & rsipairs::kQ0All) != 0; q0_q0 += (v & rsipairs::kQ0Q0) != 0; rp += (v & rsipairs::kRp) != 0;
  }
  for (int d = 32; d > 0; d >>= 1) { q0_all += __shfl_down(q0_all, d, 64); q0_q0 += __shfl_down(q0_q0, d, 64); rp += __shfl_down(rp, d, 64); }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { s_part[wave][0] = q0_all; s_part[wave][1] = q0_q0; s_part[wave][2] = rp; }
  __syncthreads();
  if (threadIdx.x < 3) {
    uint32_t v = 0;
    for (int w = 0; w < kPairThreads / 64; ++w) v += s_part[w][threadIdx.x];
    out[4 * blockIdx.x + threadIdx.x] = v;
  }
  if (threadIdx.x == 3) out[4 * blockIdx.x + 3] = hi > lo ? hi - lo : 0;
}

long long sample_tiles(long long n) { return (n + kPairSampleTile - 1) / kPairSampleTile; }

}  // namespace

void launch_bam_pairs(const void* data, const uint32_t* rec_off, int nrec, int tid, long long base, PairTable t, int32_t* words, int parity,
                      hipStream_t stream) {
  if (nrec <= 0) return;
  RSI_LAUNCH(k_bam_pairs, dim3((nrec + kPairThreads - 1) / kPairThreads), dim3(kPairThreads), 0, stream, static_cast<const uint8_t*>(data), rec_off,
             nrec, tid, base, t, words, parity);
}

size_t pair_sample_workspace_bytes(long long n) { return 256 + 2 * (size_t)(sample_tiles(n) + 1) * sizeof(Seg); }

const void* pair_sample_tile_pre(const void* ws, long long n) {
  return reinterpret_cast<const Seg*>(static_cast<const char*>(ws) + 256) + sample_tiles(n) + 1;
}

void launch_pair_sample(PairTable t, long long n, long long tid_len, void* ws, unsigned long long* out, hipStream_t stream) {
  const long long ntiles = sample_tiles(n);
  unsigned int* stop = static_cast<unsigned int*>(ws);
  Seg* tile_sum = reinterpret_cast<Seg*>(static_cast<char*>(ws) + 256);
  Seg* tile_pre = tile_sum + ntiles + 1;
  if (ntiles > 0) RSI_LAUNCH(k_pair_sample_tiles, dim3((unsigned)ntiles), dim3(kPairThreads), 0, stream, t, n, tile_sum);
  RSI_LAUNCH(k_pair_sample_scan, dim3(1), dim3(kPairThreads), 0, stream, tile_sum, ntiles, tile_pre, stop, out);
  if (ntiles <= 0) return;
  RSI_LAUNCH(k_pair_sample_stop, dim3((unsigned)ntiles), dim3(kPairThreads), 0, stream, t, n, tid_len, tile_pre, stop);
  const long long blocks = (n + kPairThreads - 1) / kPairThreads;
  RSI_LAUNCH(k_pair_sample_sum, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(kPairThreads), 0, stream, t, n, stop, out);
}

void launch_pairs_annotate(PairTable t, long long n, int maxspan, const void* calls, int ncalls, int isize_mean, int isize_sd, uint32_t* out,
                           hipStream_t stream) {
  if (ncalls <= 0) return;
  RSI_LAUNCH(k_pairs_annotate, dim3(ncalls), dim3(kPairThreads), 0, stream, t, (uint32_t)n, maxspan, static_cast<const rsipairs::Call*>(calls),
             isize_mean, isize_sd, out);
}

}  // namespace rsik
