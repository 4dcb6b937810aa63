// kernels_geno.hip -- `rsicnv geno` on the device: the quantile triple, count, sum, minimum and maximum of arbitrary
// ranges of the compacted depth.  A job is one statistic over up to two pieces of the array; the host cuts every piece into tiles
// (geno_host.h).  One workgroup per tile counts its values into a histogram in LDS and adds the non-zero bins to its job's
// histogram in HBM with integer atomicAdd (order-independent, so results are reproducible); one workgroup per job then scans that
// histogram.  The kernel boundary is the only synchronisation between workgroups.
//   bytes:  k_geno_hist8, k_geno_scan8 -- the 256 bins are the values.
//   int32:  k_geno_init32, k_geno_minmax32, k_geno_plan32, then per pass k_geno_hist32 + k_geno_scan32: a radix select of
//           kGenoBits bits per pass over v - min, digits aligned at bit 0, from the one that holds the top bit of max - min down;
//           a span below 2^kGenoBits takes one pass.
#include "kernels.h"

namespace rsik {

namespace {

constexpr int kT = kGenoThreads;
constexpr int kWaves = kT / 64;

__device__ inline long long rank1(long long n, int q) {
  const long long r = q == 0 ? n / 4 : q == 1 ? n / 2 : n * 3 / 4;
  return r < 1 ? 1 : r;
}

// inclusive scan of one value per thread over the workgroup; ws: kWaves words of LDS.  Begins with a barrier.
__device__ inline unsigned int block_scan_incl(unsigned int v, unsigned int* ws) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int s = 1; s < 64; s <<= 1) { const unsigned int o = __shfl_up(v, s, 64); if (lane >= s) v += o; }
  __syncthreads();   // ws may still be read from the scan before
  if (lane == 63) ws[wave] = v;
  __syncthreads();
  for (int w = 0; w < wave; ++w) v += ws[w];
  return v;
}

__global__ __launch_bounds__(kT) void k_geno_hist8(const uint8_t* __restrict__ d, const GenoTile* __restrict__ tiles, unsigned int* __restrict__ hist) {
  __shared__ unsigned int sub[kWaves][256];   // a sub-histogram per wave: a fourth of the lanes contend for a counter
  const GenoTile t = tiles[blockIdx.x];
  for (int i = threadIdx.x; i < kWaves * 256; i += kT) (&sub[0][0])[i] = 0;
  __syncthreads();
  unsigned int* mine = sub[threadIdx.x >> 6];
  const uint8_t* p = d + t.off;
  const int head = min(t.len, (int)((4 - ((uintptr_t)p & 3)) & 3));   // bytes in front of the first aligned word
  const int nw = (t.len - head) >> 2, tail = t.len - head - 4 * nw;
  if ((int)threadIdx.x < head) atomicAdd(&mine[p[threadIdx.x]], 1u);
  const uint32_t* w = reinterpret_cast<const uint32_t*>(p + head);
  for (int i = threadIdx.x; i < nw; i += kT) {
    const uint32_t x = w[i];
    const uint32_t b0 = x & 255, b1 = (x >> 8) & 255, b2 = (x >> 16) & 255, b3 = x >> 24;
    if (b0 == b1 && b1 == b2 && b2 == b3) atomicAdd(&mine[b0], 4u);   // flat depth is the common case: one add for the word
    else { atomicAdd(&mine[b0], 1u); atomicAdd(&mine[b1], 1u); atomicAdd(&mine[b2], 1u); atomicAdd(&mine[b3], 1u); }
  }
  if ((int)threadIdx.x < tail) atomicAdd(&mine[p[head + 4 * nw + threadIdx.x]], 1u);
  __syncthreads();
  for (int b = threadIdx.x; b < 256; b += kT) {
    unsigned int c = 0;
    for (int k = 0; k < kWaves; ++k) c += sub[k][b];
    if (c) atomicAdd(&hist[(size_t)t.job * 256 + b], c);
  }
}

__global__ __launch_bounds__(kT) void k_geno_scan8(const unsigned int* __restrict__ hist, GenoOut* __restrict__ out) {
  __shared__ unsigned int ws[kWaves];
  __shared__ unsigned long long wsum[kWaves];
  __shared__ GenoOut r;
  const int job = blockIdx.x, b = threadIdx.x;   // kT == 256: a bin per thread
  if (b == 0) { r.n = 0; r.vmin = 0; r.vmax = 0; r.q[0] = r.q[1] = r.q[2] = 0; r.sum = 0; }
  const unsigned int c = hist[(size_t)job * 256 + b];
  const unsigned int cum = block_scan_incl(c, ws);
  __shared__ unsigned int total;
  if (b == kT - 1) total = cum;
  unsigned long long s = (unsigned long long)c * (unsigned long long)b;
  for (int k = 32; k > 0; k >>= 1) s += __shfl_down(s, k, 64);
  if ((b & 63) == 0) wsum[b >> 6] = s;
  __syncthreads();
  const long long n = total;
  const unsigned int excl = cum - c;
  if (c) {
    if (excl == 0) r.vmin = b;
    if (cum == total) r.vmax = b;
    for (int q = 0; q < 3; ++q) { const long long k = rank1(n, q); if ((long long)excl < k && (long long)cum >= k) r.q[q] = b; }
  }
  __syncthreads();
  if (b == 0) {
    r.n = (int32_t)total;
    unsigned long long a = 0;
    for (int k = 0; k < kWaves; ++k) a += wsum[k];
    r.sum = (long long)a;
    out[job] = r;
  }
}

__global__ __launch_bounds__(kT) void k_geno_init32(GenoState* __restrict__ st, int njobs, unsigned int* __restrict__ maxbits) {
  const int j = blockIdx.x * kT + threadIdx.x;
  if (j == 0) *maxbits = 0;
  if (j >= njobs) return;
  GenoState s;
  s.vmin = 0x7fffffff; s.vmax = (int32_t)0x80000000; s.n = 0; s.shift = -1; s.sum = 0;
  for (int q = 0; q < 3; ++q) { s.prefix[q] = 0; s.k[q] = 0; }
  st[j] = s;
}

__global__ __launch_bounds__(kT) void k_geno_minmax32(const int32_t* __restrict__ d, const GenoTile* __restrict__ tiles, GenoState* __restrict__ st) {
  __shared__ int32_t smin[kWaves], smax[kWaves];
  __shared__ long long ssum[kWaves];
  const GenoTile t = tiles[blockIdx.x];
  const int32_t* p = d + t.off;
  int32_t lo = 0x7fffffff, hi = (int32_t)0x80000000;
  long long sum = 0;
  for (int i = threadIdx.x; i < t.len; i += kT) { const int32_t v = p[i]; lo = min(lo, v); hi = max(hi, v); sum += v; }
  for (int k = 32; k > 0; k >>= 1) { lo = min(lo, __shfl_down(lo, k, 64)); hi = max(hi, __shfl_down(hi, k, 64)); sum += __shfl_down(sum, k, 64); }
  if ((threadIdx.x & 63) == 0) { smin[threadIdx.x >> 6] = lo; smax[threadIdx.x >> 6] = hi; ssum[threadIdx.x >> 6] = sum; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < kWaves; ++k) { lo = min(lo, smin[k]); hi = max(hi, smax[k]); sum += ssum[k]; }
    GenoState* s = st + t.job;
    atomicMin(&s->vmin, lo);
    atomicMax(&s->vmax, hi);
    atomicAdd(&s->n, (unsigned int)t.len);
    atomicAdd(&s->sum, (unsigned long long)sum);   // two's complement: exact for any signs
  }
}

// One thread per job: an empty or all-equal job is finished here; the others get their first shift and their ranks.
__global__ __launch_bounds__(kT) void k_geno_plan32(GenoState* __restrict__ st, int njobs, GenoOut* __restrict__ out, unsigned int* __restrict__ maxbits) {
  const int j = blockIdx.x * kT + threadIdx.x;
  if (j >= njobs) return;
  GenoState s = st[j];
  GenoOut r;
  r.n = (int32_t)s.n; r.sum = (long long)s.sum;
  if (s.n == 0) { r.vmin = r.vmax = r.q[0] = r.q[1] = r.q[2] = 0; r.sum = 0; out[j] = r; return; }
  r.vmin = s.vmin; r.vmax = s.vmax;
  const uint32_t span = (uint32_t)s.vmax - (uint32_t)s.vmin;
  if (span == 0) { r.q[0] = r.q[1] = r.q[2] = s.vmin; out[j] = r; return; }
  const int bits = 32 - __clz(span);
  st[j].shift = (bits - 1) / kGenoBits * kGenoBits;   // whole digits from bit 0 up: the first pass takes the short one at the top
  for (int q = 0; q < 3; ++q) st[j].k[q] = (uint32_t)rank1((long long)s.n, q);
  atomicMax(maxbits, (unsigned int)bits);
}

// which of the three histograms rank q counts into: ranks whose prefixes agree above this pass's digit share one
__device__ inline void geno_slots(const GenoState& s, int slot[3]) {
  const int up = s.shift + kGenoBits;
  const unsigned long long h0 = (unsigned long long)s.prefix[0] >> up, h1 = (unsigned long long)s.prefix[1] >> up, h2 = (unsigned long long)s.prefix[2] >> up;
  slot[0] = 0;
  slot[1] = h1 == h0 ? 0 : 1;
  slot[2] = h2 == h0 ? 0 : h2 == h1 ? slot[1] : 2;
}

__global__ __launch_bounds__(kT) void k_geno_hist32(const int32_t* __restrict__ d, const GenoTile* __restrict__ tiles, const GenoState* __restrict__ st,
                                                    unsigned int* __restrict__ hist) {
  __shared__ unsigned int h[3][kGenoBins];
  const GenoTile t = tiles[blockIdx.x];
  const GenoState s = st[t.job];
  if (s.shift < 0) return;   // finished in an earlier pass (the whole workgroup leaves)
  int slot[3];
  geno_slots(s, slot);
  const int nslot = max(slot[1], slot[2]) + 1;
  for (int i = threadIdx.x; i < nslot * kGenoBins; i += kT) (&h[0][0])[i] = 0;
  __syncthreads();
  const int up = s.shift + kGenoBits;
  unsigned long long hi[3];
  for (int q = 0; q < 3; ++q) hi[q] = (unsigned long long)s.prefix[q] >> up;
  const int32_t* p = d + t.off;
  for (int i = threadIdx.x; i < t.len; i += kT) {
    const uint32_t u = (uint32_t)p[i] - (uint32_t)s.vmin;
    const unsigned long long uh = (unsigned long long)u >> up;
    const uint32_t bin = (u >> s.shift) & (kGenoBins - 1);
    if (uh == hi[0]) atomicAdd(&h[0][bin], 1u);
    if (slot[1] == 1 && uh == hi[1]) atomicAdd(&h[1][bin], 1u);
    if (slot[2] == 2 && uh == hi[2]) atomicAdd(&h[2][bin], 1u);
  }
  __syncthreads();
  unsigned int* g = hist + (size_t)t.job * 3 * kGenoBins;
  for (int i = threadIdx.x; i < nslot * kGenoBins; i += kT) { const unsigned int c = (&h[0][0])[i]; if (c) atomicAdd(&g[i], c); }
}

__global__ __launch_bounds__(kT) void k_geno_scan32(GenoState* __restrict__ st, unsigned int* __restrict__ hist, GenoOut* __restrict__ out) {
  constexpr int kPer = kGenoBins / kT;
  __shared__ unsigned int ws[kWaves];
  __shared__ uint32_t npre[3], nk[3];
  const int job = blockIdx.x;
  const GenoState s = st[job];
  if (s.shift < 0) return;
  int slot[3];
  geno_slots(s, slot);
  unsigned int* g = hist + (size_t)job * 3 * kGenoBins;
  for (int q = 0; q < 3; ++q) {
    const unsigned int* hq = g + (size_t)slot[q] * kGenoBins + threadIdx.x * kPer;
    unsigned int c[kPer], mine = 0;
    for (int i = 0; i < kPer; ++i) { c[i] = hq[i]; mine += c[i]; }
    unsigned int seen = block_scan_incl(mine, ws) - mine;
    const unsigned int k = s.k[q];
    for (int i = 0; i < kPer; ++i) {
      if (seen < k && seen + c[i] >= k) { npre[q] = s.prefix[q] | ((uint32_t)(threadIdx.x * kPer + i) << s.shift); nk[q] = k - seen; }
      seen += c[i];
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 3 * kGenoBins; i += kT) g[i] = 0;   // the next pass, and the next batch, start from zero
  if (threadIdx.x != 0) return;
  GenoState* d = st + job;
  for (int q = 0; q < 3; ++q) { d->prefix[q] = npre[q]; d->k[q] = nk[q]; }
  if (s.shift > 0) { d->shift = s.shift - kGenoBits; return; }
  d->shift = -1;
  GenoOut r;
  r.n = (int32_t)s.n; r.vmin = s.vmin; r.vmax = s.vmax; r.sum = (long long)s.sum;
  for (int q = 0; q < 3; ++q) r.q[q] = (int32_t)((uint32_t)s.vmin + npre[q]);
  out[job] = r;
}

}  // namespace

size_t geno_hist_bytes(int storage, int64_t njobs) { return (size_t)njobs * (storage == 1 ? 256 : 3 * kGenoBins) * 4; }

void launch_geno_hist8(const uint8_t* d, const GenoTile* tiles, int ntiles, unsigned int* hist, hipStream_t stream) {
  if (ntiles > 0) RSI_LAUNCH(k_geno_hist8, dim3((unsigned)ntiles), dim3(kT), 0, stream, d, tiles, hist);
}
void launch_geno_scan8(const unsigned int* hist, int njobs, GenoOut* out, hipStream_t stream) {
  RSI_LAUNCH(k_geno_scan8, dim3((unsigned)njobs), dim3(kT), 0, stream, hist, out);
}
void launch_geno_init32(GenoState* st, int njobs, unsigned int* maxbits, hipStream_t stream) {
  RSI_LAUNCH(k_geno_init32, dim3((unsigned)((njobs + kT - 1) / kT)), dim3(kT), 0, stream, st, njobs, maxbits);
}
void launch_geno_minmax32(const int32_t* d, const GenoTile* tiles, int ntiles, GenoState* st, hipStream_t stream) {
  if (ntiles > 0) RSI_LAUNCH(k_geno_minmax32, dim3((unsigned)ntiles), dim3(kT), 0, stream, d, tiles, st);
}
void launch_geno_plan32(GenoState* st, int njobs, GenoOut* out, unsigned int* maxbits, hipStream_t stream) {
  RSI_LAUNCH(k_geno_plan32, dim3((unsigned)((njobs + kT - 1) / kT)), dim3(kT), 0, stream, st, njobs, out, maxbits);
}
void launch_geno_hist32(const int32_t* d, const GenoTile* tiles, int ntiles, const GenoState* st, unsigned int* hist, hipStream_t stream) {
  if (ntiles > 0) RSI_LAUNCH(k_geno_hist32, dim3((unsigned)ntiles), dim3(kT), 0, stream, d, tiles, st, hist);
}
void launch_geno_scan32(GenoState* st, int njobs, unsigned int* hist, GenoOut* out, hipStream_t stream) {
  RSI_LAUNCH(k_geno_scan32, dim3((unsigned)njobs), dim3(kT), 0, stream, st, hist, out);
}

}  // namespace rsik
