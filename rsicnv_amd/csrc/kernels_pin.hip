// kernels_pin.hip -- `rsicnv pin` on the device.  k_bam_pin keeps, beside the pair table, every read's l_qseq and
// CIGAR (a pool of words, the space taken by one atomicAdd per wave); k_pin_sample_rd piles up the depth sample of
// bam_rd_pr_stats from the reads the pair sample's scan accepts, each at its own stretch's offset, k_pin_sample_state finds what
// the serial loop leaves behind, k_pin_sample_drd the depth steps; k_pin_windows counts, one workgroup per breakpoint, depth and
// clipped read ends of the breakpoint's window in LDS and picks the best-scoring base.  The per-read logic is bam_pin_core.h's,
// the host harness's own.
#include "kernels.h"
#include "bam_pin_core.h"
#include "pairs_scan_device.h"

namespace rsik {

namespace {

using rsipairs::Seg;

__global__ __launch_bounds__(kPairThreads) void k_bam_pin(const uint8_t* __restrict__ data, const uint32_t* __restrict__ rec_off, int nrec, long long base,
                                                          PinTable t, unsigned int* __restrict__ cursor, unsigned int pool_cap) {
  const int i = blockIdx.x * kPairThreads + threadIdx.x;
  const bool live = i < nrec;
  const rsibam::Span d{data};
  uint32_t ncig = 0;
  uint64_t cig = 0;
  int32_t lq = 0;
  if (live) {
    const uint64_t off = rec_off[i], b = off + 4;
    const uint32_t bs = rsipairs::rd32(d, off), l_name = d.at(b + 8);
    ncig = rsipairs::rd16(d, b + 12);
    lq = (int32_t)rsipairs::rd32(d, b + 16);
    if (32ull + l_name + 4ull * ncig > (uint64_t)bs) ncig = 0;      // overrun (the pair kernel flags it): the CIGAR is not read
    cig = b + 32 + l_name;
  }
  // the wave's reads take their words with one atomicAdd: an inclusive prefix over the lanes, the total from the last lane
  const uint32_t need = live ? ncig + 1 : 0;
  const int lane = threadIdx.x & 63;
  uint32_t incl = need;
  for (int s = 1; s < 64; s <<= 1) { const uint32_t v = __shfl_up(incl, s, 64); if (lane >= s) incl += v; }
  const uint32_t total = __shfl(incl, 63, 64);
  uint32_t wbase = 0;
  if (lane == 0 && total) wbase = atomicAdd(cursor, total);
  wbase = __shfl(wbase, 0, 64);
  if (!live) return;
  const long long k = base + i;
  const uint32_t at = wbase + (incl - need);
  t.lq[k] = lq;
  if ((unsigned long long)at + need > (unsigned long long)pool_cap) { t.coff[k] = 0; return; }   // pool[0] = 0: an empty CIGAR (the host sees the cursor)
  t.coff[k] = at;
  t.pool[at] = ncig;
  for (uint32_t c = 0; c < ncig; ++c) t.pool[at + 1 + c] = rsipairs::rd32(d, cig + 4ull * c);
}

// words[0]: 1 + the table index of the last read counted (atomicMax), words[1]: rsipin::SampleFlag
__global__ __launch_bounds__(kPairThreads) void k_pin_sample_rd(PairTable t, PinTable p, long long n, long long tid_len, const Seg* __restrict__ tile_pre,
                                                                const unsigned int* __restrict__ stop, int32_t* __restrict__ rdc,
                                                                unsigned int* __restrict__ words) {
  __shared__ Seg s[kPairThreads];
  const unsigned int st = *stop;
  const long long S = st == 0xffffffffu ? n : (long long)st;       // the reads before S add their bases; S itself may still be counted
  if ((long long)blockIdx.x * kPairSampleTile > S) return;
  const long long i0 = (long long)blockIdx.x * kPairSampleTile + (long long)threadIdx.x * kPairItems;
  pair_block_scan(pair_thread_seg(t, i0, n), s);
  Seg pz = rsipairs::compose(tile_pre[blockIdx.x], threadIdx.x ? s[threadIdx.x - 1] : rsipairs::seg_none());
  for (int k = 0; k < kPairItems; ++k) {
    const long long i = i0 + k;
    if (i >= n || i > S) break;
    const int32_t pos = t.pos[i], rend = t.rend[i];
    const uint32_t info = t.info[i];
    if (!rsipairs::sample_kept(pos, rend, info)) continue;
    pz = rsipairs::compose(pz, rsipairs::seg_one(pos));
    if (i == S && rsipin::stops_uncounted(pos, rend, info, tid_len)) break;
    int32_t offset, count;
    rsipairs::sample_state(pz, offset, count);
    if ((long long)rsipin::calend_of(pos, rend, info) - offset > rsipin::kRdcLimit) atomicOr(words + 1, (unsigned int)rsipin::kGrows);
    atomicMax(words, (unsigned int)i + 1u);
    if (i == S) break;
    const uint32_t* c = p.pool + p.coff[i];
    rsipin::sample_add(c + 1, c[0], pos, offset, tid_len, [&](long long at, int dlt) { if (at < rsipin::kRdcSize) atomicAdd(rdc + at, dlt); });
  }
}

// One workgroup: what the serial loop holds behind the last read counted.
__global__ __launch_bounds__(kPairThreads) void k_pin_sample_state(PairTable t, PinTable p, long long n, const Seg* __restrict__ tile_pre,
                                                                   const unsigned int* __restrict__ words, rsipin::SampleState* __restrict__ out) {
  __shared__ Seg s[kPairThreads];
  __shared__ int32_t s_state[2];
  __shared__ unsigned long long s_part[kPairThreads / 64];
  const unsigned int lastc = words[0];
  if (lastc == 0) {
    if (threadIdx.x == 0) *out = rsipin::SampleState{0, -10000, 0, (int32_t)words[1], 0};
    return;
  }
  const long long L = (long long)lastc - 1, tile = L / kPairSampleTile;
  const long long i0 = tile * kPairSampleTile + (long long)threadIdx.x * kPairItems;
  pair_block_scan(pair_thread_seg(t, i0, n), s);
  if (L >= i0 && L < i0 + kPairItems) {
    Seg pz = rsipairs::compose(tile_pre[tile], threadIdx.x ? s[threadIdx.x - 1] : rsipairs::seg_none());
    for (long long i = i0; i <= L; ++i)
      if (rsipairs::sample_kept(t.pos[i], t.rend[i], t.info[i])) pz = rsipairs::compose(pz, rsipairs::seg_one(t.pos[i]));
    rsipairs::sample_state(pz, s_state[0], s_state[1]);
  }
  __syncthreads();
  // the stretch's reads are the accepted ones from the first pos >= its start on (the one before it lies 1000 bases lower)
  const int32_t pos_start = s_state[0];
  unsigned long long sum = 0;
  for (long long i = (long long)lower_bound_pos(t.pos, (uint32_t)n, pos_start) + threadIdx.x; i <= L; i += kPairThreads)
    if (rsipairs::sample_kept(t.pos[i], t.rend[i], t.info[i])) sum += (unsigned long long)(long long)p.lq[i];
  for (int d = 32; d > 0; d >>= 1) sum += __shfl_down(sum, d, 64);
  if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long v = 0;
    for (int w = 0; w < kPairThreads / 64; ++w) v += s_part[w];
    *out = rsipin::SampleState{pos_start, t.pos[L], s_state[1], (int32_t)words[1], (long long)v};
  }
}

__global__ __launch_bounds__(kPairThreads) void k_pin_sample_drd(const int32_t* __restrict__ rdc, int32_t* __restrict__ drd, int lo, int hi, int l_qseq) {
  const int k = lo + blockIdx.x * kPairThreads + threadIdx.x;
  if (k < hi) drd[k] = rsipin::sample_drd(rdc, k, l_qseq);
}

__global__ __launch_bounds__(kPairThreads) void k_pin_windows(PairTable t, PinTable p, uint32_t n, int maxspan, long long tid_len,
                                                              const rsipin::Bp* __restrict__ bps, int r_len, int l_qseq, double drd_sd,
                                                              int32_t* __restrict__ out) {
  extern __shared__ int32_t s_cnt[];                 // rd, s_beg, s_end: 2 r_len + 1 each
  __shared__ rsipin::Best s_best[kPairThreads];
  const int size = 2 * r_len + 1;
  for (int i = threadIdx.x; i < 3 * size; i += kPairThreads) s_cnt[i] = 0;
  __syncthreads();
  const rsipin::Bp b = bps[blockIdx.x];
  const long long beg = (long long)b.bp - r_len, end = (long long)b.bp + r_len;
  // a read that reaches the window begins above its first base - maxspan; one that begins at `end` or later is not read
  const uint32_t lo = lower_bound_pos(t.pos, n, (beg < 0 ? 0 : beg) - (long long)maxspan);
  const uint32_t hi = lower_bound_pos(t.pos, n, end);
#pragma unroll 1
  for (uint32_t i = lo + threadIdx.x; i < hi; i += kPairThreads) {
    const int32_t pos = t.pos[i], rend = t.rend[i];
    if (!rsipin::window_kept(pos, rend, t.info[i], tid_len, beg, end)) continue;
    const uint32_t* c = p.pool + p.coff[i];
    rsipin::window_add(c + 1, c[0], pos, rend, beg, r_len, [&](int which, int32_t ipos) { atomicAdd(s_cnt + which * size + ipos, 1); });
  }
  __syncthreads();
  const int32_t* clips = s_cnt + (b.five ? rsipin::kSEnd : rsipin::kSBeg) * size;
  rsipin::Best best = rsipin::best_none();
  for (int i = threadIdx.x; i < size; i += kPairThreads)
    best = rsipin::best_take(best, rsipin::score_of(rsipin::window_drd(s_cnt, size, i, l_qseq), clips[i], drd_sd, b.five != 0), i);
  s_best[threadIdx.x] = best;
  __syncthreads();
  for (int d = kPairThreads / 2; d > 0; d >>= 1) {
    if ((int)threadIdx.x < d) s_best[threadIdx.x] = rsipin::best_of(s_best[threadIdx.x], s_best[threadIdx.x + d]);
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const int32_t im = s_best[0].i;
    out[2 * blockIdx.x] = im;
    out[2 * blockIdx.x + 1] = im >= 0 ? clips[im] : 0;
  }
}

}  // namespace

void launch_bam_pin(const void* data, const uint32_t* rec_off, int nrec, long long base, PinTable t, unsigned int* cursor, unsigned int pool_cap,
                    hipStream_t stream) {
  if (nrec <= 0) return;
  RSI_LAUNCH(k_bam_pin, dim3((nrec + kPairThreads - 1) / kPairThreads), dim3(kPairThreads), 0, stream, static_cast<const uint8_t*>(data), rec_off, nrec,
             base, t, cursor, pool_cap);
}

void launch_pin_sample(PairTable t, PinTable p, long long n, long long tid_len, const void* ws, int32_t* rdc, int32_t* scan_scratch, void* state,
                       hipStream_t stream) {
  const long long ntiles = (n + kPairSampleTile - 1) / kPairSampleTile;
  const unsigned int* stop = static_cast<const unsigned int*>(ws);
  const Seg* tile_pre = static_cast<const Seg*>(pair_sample_tile_pre(ws, n));
  unsigned int* words = reinterpret_cast<unsigned int*>(rdc + rsipin::kRdcSize);     // the tail of rdc, cleared with it
  (void)hipMemsetAsync(rdc, 0, (size_t)kPinRdcWords * 4, stream);
  if (ntiles > 0) RSI_LAUNCH(k_pin_sample_rd, dim3((unsigned)ntiles), dim3(kPairThreads), 0, stream, t, p, n, tid_len, tile_pre, stop, rdc, words);
  RSI_LAUNCH(k_pin_sample_state, dim3(1), dim3(kPairThreads), 0, stream, t, p, n, tile_pre, words, static_cast<rsipin::SampleState*>(state));
  launch_inclusive_scan_i32(rdc, (long long)rsipin::kRdcSize, scan_scratch, stream);
}

void launch_pin_sample_drd(const int32_t* rdc, int32_t* drd, int lo, int hi, int l_qseq, hipStream_t stream) {
  if (hi <= lo) return;
  RSI_LAUNCH(k_pin_sample_drd, dim3((hi - lo + kPairThreads - 1) / kPairThreads), dim3(kPairThreads), 0, stream, rdc, drd, lo, hi, l_qseq);
}

void launch_pin_windows(PairTable t, PinTable p, long long n, int maxspan, long long tid_len, const void* bps, int nbp, int r_len, int l_qseq,
                        double drd_sd, int32_t* out, hipStream_t stream) {
  if (nbp <= 0) return;
  const size_t lds = (size_t)3 * (2 * (size_t)r_len + 1) * 4;
  RSI_LAUNCH(k_pin_windows, dim3(nbp), dim3(kPairThreads), lds, stream, t, p, (uint32_t)n, maxspan, tid_len, static_cast<const rsipin::Bp*>(bps), r_len,
             l_qseq, drd_sd, out);
}

}  // namespace rsik
