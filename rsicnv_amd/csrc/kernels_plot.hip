// kernels_plot.hip -- the numbers of planned gnuplot figures from an int32 array in HBM: the exact sum of every
// queried running-mean window, the queried values, and the expansion of a run's compacted depth.  The quartiles, sums and counts
// of body and neighbourhood are geno's (kernels_geno.hip).  A window sum is the difference of two prefix sums of the figure's
// neighbourhood; no prefix array is ever stored: tile sums, a scan of them per figure, then every tile is scanned once more in LDS
// from its base and hands out the prefix at the window ends that fall into it.  Every neighbourhood value is read twice, whatever
// the band and the number of queries.  The kernel boundary is the only synchronisation between workgroups.
#include "kernels.h"

namespace rsik {

namespace {

constexpr int kT = kPlotThreads;
constexpr int kWaves = kT / 64;

// the job whose tiles hold tile b: the last one with tile0 <= b
__device__ inline int job_of_tile(const PlotJob* __restrict__ jobs, int njobs, int b) {
  int lo = 0, hi = njobs - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (jobs[mid].tile0 <= b) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// value r of a job's neighbourhood: the front piece, then the back piece
__device__ inline int32_t ref_value(const int32_t* __restrict__ d, const PlotJob& j, int r) {
  return r < j.la ? d[(long long)j.a0 + r] : d[(long long)j.b0 + (r - j.la)];
}

// inclusive scan of one value per thread over the workgroup; ws: kWaves words of LDS.  Begins with a barrier.
__device__ inline long long block_scan_incl64(long long v, long long* ws) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int s = 1; s < 64; s <<= 1) { const long long o = __shfl_up(v, s, 64); if (lane >= s) v += o; }
  __syncthreads();   // ws may still be read from the scan before
  if (lane == 63) ws[wave] = v;
  __syncthreads();
  for (int w = 0; w < wave; ++w) v += ws[w];
  return v;
}

__global__ __launch_bounds__(kT) void k_plot_tile_sums(const int32_t* __restrict__ d, const PlotJob* __restrict__ jobs, int njobs, int tile,
                                                       long long* __restrict__ tsum) {
  __shared__ long long ws[kWaves];
  const PlotJob j = jobs[job_of_tile(jobs, njobs, (int)blockIdx.x)];
  const int nref = j.la + j.lb;
  const long long r0 = (long long)((int)blockIdx.x - j.tile0) * tile;
  const int len = (int)min((long long)tile, (long long)nref - r0);
  long long s = 0;
  for (int i = threadIdx.x; i < len; i += kT) s += ref_value(d, j, (int)r0 + i);
  for (int k = 32; k > 0; k >>= 1) s += __shfl_down(s, k, 64);
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < kWaves; ++k) s += ws[k];
    tsum[blockIdx.x] = s;
  }
}

// one workgroup per job: its tile sums become the sums in front of each tile
__global__ __launch_bounds__(kT) void k_plot_tile_scan(const PlotJob* __restrict__ jobs, int tile, long long* __restrict__ tsum) {
  __shared__ long long ws[kWaves];
  __shared__ long long carry_s;
  const PlotJob j = jobs[blockIdx.x];
  const int nt = (int)(((long long)j.la + j.lb + tile - 1) / tile);
  long long* t = tsum + j.tile0;
  long long carry = 0;
  for (int base = 0; base < nt; base += kT) {
    const int i = base + (int)threadIdx.x;
    const long long v = i < nt ? t[i] : 0;
    const long long incl = block_scan_incl64(v, ws);
    if (i < nt) t[i] = carry + incl - v;
    if (threadIdx.x == kT - 1) carry_s = carry + incl;
    __syncthreads();
    carry = carry_s;
  }
}

// the window end of query q's centre: kind 0 the window's last value c + h, kind 1 the value in front of its first, c - h - 1
__device__ inline int window_end(int ref, int h, int nref, int kind) {
  const int c = min(max(ref, h), nref - 1 - h);
  return kind == 0 ? c + h : c - h - 1;
}

__global__ __launch_bounds__(kT) void k_plot_window_ends(const int32_t* __restrict__ d, const PlotJob* __restrict__ jobs, int njobs, int tile,
                                                         const long long* __restrict__ tsum, const int32_t* __restrict__ qref,
                                                         long long* __restrict__ ends) {
  __shared__ long long pre[kPlotMaxTile];
  __shared__ long long ws[kWaves];
  __shared__ int bound[8][2];   // per (block 0 | block 2, kind): the queries whose end falls into this tile, [first, last)
  const PlotJob j = jobs[job_of_tile(jobs, njobs, (int)blockIdx.x)];
  const int nref = j.la + j.lb, h = j.band / 2;
  const int r0 = (int)((long long)((int)blockIdx.x - j.tile0) * tile);
  const int len = min(tile, nref - r0), r1 = r0 + len;
  for (int i = threadIdx.x; i < len; i += kT) pre[i] = ref_value(d, j, r0 + i);
  // the query ranges: four ascending runs of window ends, a search for each of r0 and r1 in each
  if (threadIdx.x < 8) {
    const int run = threadIdx.x >> 2, kind = (threadIdx.x >> 1) & 1, which = threadIdx.x & 1;
    const long long first = j.q0 + (run ? (long long)j.nq0 + j.nq1 : 0);
    const int cnt = run ? j.nq2 : j.nq0;
    const int want = which ? r1 : r0;
    int lo = 0, hi = cnt;   // the first query whose end is >= want
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (window_end(qref[first + mid], h, nref, kind) < want) lo = mid + 1; else hi = mid;
    }
    bound[run * 2 + kind][which] = lo;
  }
  __syncthreads();
  // inclusive prefix sums of the tile in place: a run of consecutive values per thread, a scan of the runs' sums
  const int per = (tile + kT - 1) / kT;
  const int b = min((int)threadIdx.x * per, len), e = min(b + per, len);
  long long s = 0;
  for (int i = b; i < e; ++i) s += pre[i];
  long long run = tsum[blockIdx.x] + block_scan_incl64(s, ws) - s;
  for (int i = b; i < e; ++i) { run += pre[i]; pre[i] = run; }
  __syncthreads();
  for (int rk = 0; rk < 4; ++rk) {
    const int run_i = rk >> 1, kind = rk & 1;
    const long long first = j.q0 + (run_i ? (long long)j.nq0 + j.nq1 : 0);
    for (int k = bound[rk][0] + (int)threadIdx.x; k < bound[rk][1]; k += kT) {
      const int we = window_end(qref[first + k], h, nref, kind);
      ends[2 * (first + k) + kind] = pre[we - r0];
    }
  }
  if (threadIdx.x < 4) {   // block 3's two rows
    const long long q = j.q0 + (long long)j.nq0 + j.nq1 + j.nq2 + (threadIdx.x >> 1);
    const int kind = threadIdx.x & 1;
    const int we = window_end(qref[q], h, nref, kind);
    if (we >= r0 && we < r1) ends[2 * q + kind] = pre[we - r0];
  }
}

__global__ __launch_bounds__(kT) void k_plot_gather(const int32_t* __restrict__ d, const int32_t* __restrict__ qdepth, const int32_t* __restrict__ qref,
                                                    const long long* __restrict__ ends, long long nq, int32_t* __restrict__ value,
                                                    long long* __restrict__ wsum) {
  const long long q = (long long)blockIdx.x * kT + threadIdx.x;
  if (q >= nq) return;
  const int32_t di = qdepth[q];
  value[q] = di >= 0 ? d[di] : 0;
  wsum[q] = qref[q] >= 0 ? ends[2 * q] - ends[2 * q + 1] : 0;
}

template <class T>
__global__ __launch_bounds__(kT) void k_plot_expand(const T* __restrict__ src, const int32_t* __restrict__ starts, const int32_t* __restrict__ ends,
                                                    const long long* __restrict__ before, int npairs, int32_t* __restrict__ out, long long n) {
  const long long i = (long long)blockIdx.x * kT + threadIdx.x;
  if (i >= n) return;
  int lo = 0, hi = npairs;   // the pairs that start at or below i
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (starts[mid] <= i) lo = mid + 1; else hi = mid;
  }
  if (lo == 0) { out[i] = (int32_t)src[i]; return; }
  const int k = lo - 1;
  if (i <= ends[k]) { out[i] = 0; return; }
  out[i] = (int32_t)src[i - (before[k] + ((long long)ends[k] - starts[k] + 1))];
}

}  // namespace

void launch_plot_tile_sums(const int32_t* d, const PlotJob* jobs, int njobs, int ntiles, int tile, long long* tsum, hipStream_t stream) {
  if (ntiles > 0) RSI_LAUNCH(k_plot_tile_sums, dim3((unsigned)ntiles), dim3(kT), 0, stream, d, jobs, njobs, tile, tsum);
}
void launch_plot_tile_scan(const PlotJob* jobs, int njobs, int tile, long long* tsum, hipStream_t stream) {
  if (njobs > 0) RSI_LAUNCH(k_plot_tile_scan, dim3((unsigned)njobs), dim3(kT), 0, stream, jobs, tile, tsum);
}
void launch_plot_window_ends(const int32_t* d, const PlotJob* jobs, int njobs, int ntiles, int tile, const long long* tsum, const int32_t* qref,
                             long long* ends, hipStream_t stream) {
  if (ntiles > 0) RSI_LAUNCH(k_plot_window_ends, dim3((unsigned)ntiles), dim3(kT), 0, stream, d, jobs, njobs, tile, tsum, qref, ends);
}
void launch_plot_gather(const int32_t* d, const int32_t* qdepth, const int32_t* qref, const long long* ends, long long nq, int32_t* value,
                        long long* wsum, hipStream_t stream) {
  if (nq > 0) RSI_LAUNCH(k_plot_gather, dim3((unsigned)((nq + kT - 1) / kT)), dim3(kT), 0, stream, d, qdepth, qref, ends, nq, value, wsum);
}
void launch_plot_expand(const void* src, int storage, const int32_t* starts, const int32_t* ends, const long long* before, int npairs, int32_t* out,
                        long long n, hipStream_t stream) {
  if (n <= 0) return;
  const dim3 grid((unsigned)((n + kT - 1) / kT));
  if (storage == 1) RSI_LAUNCH(k_plot_expand<uint8_t>, grid, dim3(kT), 0, stream, static_cast<const uint8_t*>(src), starts, ends, before, npairs, out, n);
  else RSI_LAUNCH(k_plot_expand<int32_t>, grid, dim3(kT), 0, stream, static_cast<const int32_t*>(src), starts, ends, before, npairs, out, n);
}

}  // namespace rsik
