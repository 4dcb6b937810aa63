// kernels_cand.hip -- candidate stages on the device: boundary refinement
// (optimize_with_derivative, rsi.cpp:889-944) and the neighbourhood test (isitcnvwrap + isitcnv,
// rsi.cpp:175-287, 101-172) directly on the compacted depth in HBM, one workgroup per candidate.
// The host keeps the list logic (who is whose neighbour, what is deleted, merge decisions); the
// device does every array-sized step, so the per-base depth never has to be paged to the host.
//
// Exactness: all sums of depths are integers (int64); window means are (float)((double)S/width)
// as in the reference; quantiles come from integer histograms on the reference's grids.  The one
// deviation is the second moment of the window means, summed here as a tree of doubles instead of
// sequentially (relative difference ~1e-15; it only enters the p-value).
//
// Two forms of the neighbourhood test.  k_candidate_test: one workgroup per test, window sums from an exact prefix array.
// The split form, three launches: k_cand_gather (the two walks side by side), k_cand_sums (sixteen chunks of windows per
// test, window sums by sliding differences -- no prefix array, no int64 scratch, nothing waits for another workgroup --
// and the candidate's own statistics in a seventeenth workgroup), k_cand_hist (0.01-grid histogram, last-workgroup fold).
#include "kernels.h"

namespace rsik {

namespace {

constexpr int kThreads = 256;        // boundary refinement, range sums
constexpr int kTestThreads = 1024;   // neighbourhood test: one workgroup per candidate, so make it a big one
constexpr int kMaxWaves = kTestThreads / 64;
__device__ inline int lane_id() { return threadIdx.x & 63; }

// ---- block-wide helpers (256 threads) --------------------------------------------------------
template <class T, class Op>
__device__ inline T block_reduce(T v, Op op, T* s_tmp /* kMaxWaves */) {
  for (int d = 32; d >= 1; d >>= 1) v = op(v, __shfl_xor(v, d));
  __syncthreads();
  if (lane_id() == 0) s_tmp[threadIdx.x >> 6] = v;
  __syncthreads();
  T r = s_tmp[0];
  for (int w = 1; w < (int)(blockDim.x >> 6); ++w) r = op(r, s_tmp[w]);
  __syncthreads();
  return r;
}
// exclusive prefix of one int per thread; returns the thread's offset, *total = sum over the block
__device__ inline int block_exscan(int v, int* s_tmp /* kMaxWaves */, int* total) {
  const int incl = wave_incl_scan(v);
  __syncthreads();
  if (lane_id() == 63) s_tmp[threadIdx.x >> 6] = incl;
  __syncthreads();
  int base = 0, tot = 0;
  for (int w = 0; w < (int)(blockDim.x >> 6); ++w) { if (w < (int)(threadIdx.x >> 6)) base += s_tmp[w]; tot += s_tmp[w]; }
  __syncthreads();
  *total = tot;
  return base + incl - v;
}
// exact int64 prefix of f(0..len-1) into P[0..len] (P[0] = 0), in tiles of blockDim.x consecutive elements
// (coalesced reads and writes) with a running carry
template <class F>
__device__ inline void block_prefix_i64(long long* __restrict__ P, int len, F f, long long* s_tmp /* kMaxWaves */);

// exclusive prefix of one int64 per thread over the block; *total = block sum
__device__ inline long long block_exscan_i64(long long v, long long* s_tmp /* kMaxWaves */, long long* total) {
  const long long incl = wave_incl_scan(v);
  __syncthreads();
  if (lane_id() == 63) s_tmp[threadIdx.x >> 6] = incl;
  __syncthreads();
  long long base = 0, tot = 0;
  for (int w = 0; w < (int)(blockDim.x >> 6); ++w) { if (w < (int)(threadIdx.x >> 6)) base += s_tmp[w]; tot += s_tmp[w]; }
  __syncthreads();
  *total = tot;
  return base + incl - v;
}

template <class F>
__device__ inline void block_prefix_i64(long long* __restrict__ P, int len, F f, long long* s_tmp) {
  long long carry = 0;
  if (threadIdx.x == 0) P[0] = 0;
  for (int t0 = 0; t0 < len; t0 += (int)blockDim.x) {
    const int e = t0 + (int)threadIdx.x;
    const long long v = e < len ? f(e) : 0;
    long long total;
    const long long ex = block_exscan_i64(v, s_tmp, &total);
    if (e < len) P[e + 1] = carry + ex + v;
    carry += total;
  }
  __syncthreads();
}

// ------------------------------------------------------------------------------------------
// Boundary refinement (optimize_with_derivative, rsi.cpp:889-944; detectcnv calls it twice, rsi.cpp:
// 1876-1877: one launch per call).  dd[i] = sum of the len values left of q = from+i minus the sum of
// the len values from q on; the new start is the first maximum (DEL) / minimum (DUP) of dd over its
// first 2*reach entries, the new end the first minimum / maximum over its last 2*reach entries; only
// strictly positive / negative values count and index 0 never moves anything.
// Each of the two search windows of a candidate is cut into kEdgeChunks pieces, one workgroup each.
// A workgroup walks its piece in tiles of 256 with dd[i+1] - dd[i] = -p[q-len] + 2 p[q] - p[q+len] and an
// exact int64 block scan, RELATIVE to the piece's first index: the extremum of a piece sits at the same index
// whatever the offset, and the sign test is monotone in the value, so both wait for the fold.  dd at a
// window's first index (a sum over 2*len values) is itself shared out: every workgroup of the window adds
// a sixteenth of it to the window's accumulator.  The last workgroup of a candidate to finish chains the
// pieces (offset of piece c = window start + totals of the pieces before it), applies the sign test, folds
// (smallest index wins ties, as the reference's strict comparisons do) and writes the new coordinates.
// Per candidate this reads about 7*len values instead of 2*len per workgroup.
constexpr int kEdgeChunks = 16;
struct ArgBest { long long v; int i; };
__device__ inline ArgBest arg_pick(ArgBest a, ArgBest b, bool want_max) {
  if (b.i < 0) return a;
  if (a.i < 0) return b;
  if (a.v != b.v) return (want_max ? (b.v > a.v) : (b.v < a.v)) ? b : a;
  return b.i < a.i ? b : a;
}

struct SharpenWs {   // views into the workspace of one launch (sharpen_workspace_bytes)
  unsigned long long* start_acc;   // [njobs][2]   dd at the first index of each window, accumulated; zero between launches
  uint32_t* done;                  // [njobs]      finished workgroups; zero between launches
  long long* part_v;               // [njobs][32]  extremum of the piece, relative to its first index
  long long* part_t;               // [njobs][32]  sum of the piece's steps
  int32_t* part_i;                 // [njobs][32]  index of the extremum (-1: empty piece)
};
__host__ __device__ inline size_t sharpen_zero_bytes(int njobs) { return ((size_t)njobs * 16 + (size_t)njobs * 4 + 15) & ~size_t(15); }
__host__ __device__ inline SharpenWs sharpen_views(void* ws, int njobs) {
  unsigned char* p = static_cast<unsigned char*>(ws);
  const size_t slots = (size_t)njobs * 2 * kEdgeChunks;
  SharpenWs w;
  w.start_acc = reinterpret_cast<unsigned long long*>(p);
  w.done = reinterpret_cast<uint32_t*>(p + (size_t)njobs * 16);
  p += sharpen_zero_bytes(njobs);
  w.part_v = reinterpret_cast<long long*>(p);
  w.part_t = w.part_v + slots;
  w.part_i = reinterpret_cast<int32_t*>(w.part_t + slots);
  return w;
}

template <typename TD>
__global__ __launch_bounds__(kThreads) void k_sharpen_edges(const TD* __restrict__ rdc, int64_t ncompact,
                                                            EdgeJob* __restrict__ jobs, int njobs /* capacity the workspace is laid out for */,
                                                            void* __restrict__ ws) {
  __shared__ long long s_l[kMaxWaves];
  __shared__ long long s_v[kThreads / 64];
  __shared__ int s_i[kThreads / 64];
  __shared__ int s_last;
  const SharpenWs W = sharpen_views(ws, njobs);
  const int jb = blockIdx.y;
  const EdgeJob job = jobs[jb];
  const int len = job.end - job.start + 1;
  const int reach = len / 4 > 250 ? len / 4 : 250;
  const int from = job.start - reach, to = job.end + reach;
  if (job.type > 1) return;                                                  // untyped candidate: the reference moves nothing
  if (from < 2 * len || (int64_t)to > ncompact - 2 * (int64_t)len) return;   // too close to the ends: unchanged
  const int nstep = to - from;
  const int win = blockIdx.x / kEdgeChunks, chunk = blockIdx.x % kEdgeChunks;   // win 0: start search, 1: end search
  const int wlen = 2 * reach;
  // The two search windows are the first and the last 2 * reach entries of dd[0 .. nstep).  A candidate whose first
  // refinement left end < start (len <= 0) has FEWER than 2 * reach entries: the reference's loops then index its vector out
  // of range (rsi.cpp:917, 930: undefined); here, as in the host path (host_calls.cpp:sharpen_edges) and the oracle, both
  // searches cover the entries that exist.  (Until round 4 this kernel continued dd's recurrence beyond the vector instead --
  // a third answer, found by tests/test_fallback_paths.py's bimodal chromosome as one call's neighbourhood statistics.)
  const int wbase = win == 0 ? 0 : (nstep - wlen > 0 ? nstep - wlen : 0);
  const int wend = win == 0 ? (wlen < nstep ? wlen : nstep) : nstep;
  const int wspan = wend > wbase ? wend - wbase : 0;
  const int cs = (wspan + kEdgeChunks - 1) / kEdgeChunks;
  const int i0 = wbase + chunk * cs;
  int i1 = i0 + cs; if (i1 > wend) i1 = wend;
  const bool del = job.type == 0;
  const bool want_max = win == 0 ? del : !del;
  {   // this workgroup's share of dd at the window's first index
    const int q0 = from + wbase;
    const int js = (len + kEdgeChunks - 1) / kEdgeChunks;
    const int j0 = chunk * js;
    int j1 = j0 + js; if (j1 > len) j1 = len;
    long long acc = 0;
    for (int j = j0 + (int)threadIdx.x; j < j1; j += kThreads) acc += (long long)rdc[q0 - len + j] - (long long)rdc[q0 + j];
    acc = block_reduce(acc, [](long long a, long long b) { return a + b; }, s_l);
    if (threadIdx.x == 0 && acc != 0) atomicAdd(&W.start_acc[jb * 2 + win], (unsigned long long)acc);
  }
  ArgBest best{0, -1};
  long long cur = 0;   // dd relative to the piece's first index
  for (int t0 = i0; t0 < i1; t0 += kThreads) {
    const int i = t0 + (int)threadIdx.x;
    long long delta = 0;
    if (i < i1) { const int q = from + i; delta = -(long long)rdc[q - len] + 2ll * rdc[q] - (long long)rdc[q + len]; }
    long long total;
    const long long dd = cur + block_exscan_i64(delta, s_l, &total);
    if (i < i1) best = arg_pick(best, ArgBest{dd, i}, want_max);
    cur += total;
  }
  // block arg-reduction (values first, then smallest index)
  for (int d = 32; d >= 1; d >>= 1) { ArgBest o; o.v = __shfl_xor(best.v, d); o.i = __shfl_xor(best.i, d); best = arg_pick(best, o, want_max); }
  __syncthreads();
  if (lane_id() == 0) { s_v[threadIdx.x >> 6] = best.v; s_i[threadIdx.x >> 6] = best.i; }
  __syncthreads();
  if (threadIdx.x == 0) {
    ArgBest r{s_v[0], s_i[0]};
    for (int w = 1; w < kThreads / 64; ++w) r = arg_pick(r, ArgBest{s_v[w], s_i[w]}, want_max);
    const size_t slot = (size_t)jb * 2 * kEdgeChunks + blockIdx.x;
    // hand-over without fences (device_util.h): write-through stores, wait for them, then the arrival counter; the reader
    // uses coherent loads.  An agent-scope fence here writes back the XCD's whole L2 -- in a pool that is other
    // chromosomes' streaming output, and 1280 workgroups per launch each waited for it.
    st_cg(reinterpret_cast<unsigned long long*>(&W.part_v[slot]), (unsigned long long)r.v);
    st_cg(reinterpret_cast<unsigned int*>(&W.part_i[slot]), (unsigned int)r.i);
    st_cg(reinterpret_cast<unsigned long long*>(&W.part_t[slot]), (unsigned long long)cur);
    drain();
    s_last = atomicAdd(&W.done[jb], 1u) == 2 * kEdgeChunks - 1;
  }
  __syncthreads();
  if (s_last && threadIdx.x == 0) {   // every piece of this candidate is in: chain and fold them
    ArgBest pick[2] = {{0, -1}, {0, -1}};
    for (int w = 0; w < 2; ++w) {
      const bool wmax = w == 0 ? del : !del;
      long long off = (long long)atomicAdd(&W.start_acc[jb * 2 + w], 0ull);   // dd at the window's first index
      for (int c = 0; c < kEdgeChunks; ++c) {
        const size_t a = (size_t)jb * 2 * kEdgeChunks + w * kEdgeChunks + c;
        const int pi = (int)ld_cg(reinterpret_cast<const unsigned int*>(&W.part_i[a]));
        if (pi >= 0) {
          const long long v = (long long)ld_cg(reinterpret_cast<const unsigned long long*>(&W.part_v[a])) + off;
          if (wmax ? v > 0 : v < 0) pick[w] = arg_pick(pick[w], ArgBest{v, pi}, wmax);
        }
        off += (long long)ld_cg(reinterpret_cast<const unsigned long long*>(&W.part_t[a]));
      }
      W.start_acc[jb * 2 + w] = 0;   // ready for the second call
    }
    if (pick[0].i > 0) jobs[jb].start = from + pick[0].i;
    if (pick[1].i > 0) jobs[jb].end = to - nstep + pick[1].i;
    W.done[jb] = 0;
  }
}

// ------------------------------------------------------------------------------------------
// Neighbourhood test.  See CandJob in kernels.h for what the host prepares.
// The gathered values are stored as TS: bytes where the compacted depth is bytes, int32 where it is int32 -- or where
// RSI_HOT_CAND_BYTES=0 asks for the wide form of byte depth (pipeline.hip).  The values, their order and everything the
// walk decides are the same in both; the width only sets what the scratch arrays hold and how far a trip of the walk reaches.
constexpr int kWalkLds = kCandHistBins * 4;   // the walks stage a trip's taken values in the histogram's LDS

// s_scan doubles as scratch of hist_ranks; the rest is the walk's per-trip exchange, double-buffered by trip parity
struct WalkShared { int s_scan[kMaxWaves]; int cnt[2][kMaxWaves]; int trg[2][kMaxWaves]; int kept[2]; int lastt[2]; };

// Sixteen consecutive values in walk order from `first` (first, first + dir, ...): one or four 16-byte loads where the
// block lies inside the array, clamped single loads at the chromosome's ends (those positions are masked by the caller).
struct __attribute__((packed, aligned(1))) WalkBytes16 { uint32_t w[4]; };
struct __attribute__((packed, aligned(4))) WalkInts4 { int x, y, z, w; };
__device__ inline void walk_load16(const uint8_t* __restrict__ A, int64_t N, long long first, int dir, int* out) {
  const long long lo = dir > 0 ? first : first - 15;
  if (lo >= 0 && lo + 15 <= N - 1) {
    const WalkBytes16 b = *reinterpret_cast<const WalkBytes16*>(A + lo);
#pragma unroll
    for (int j = 0; j < 16; ++j) { const int k = dir > 0 ? j : 15 - j; out[j] = (int)((b.w[k >> 2] >> (8 * (k & 3))) & 0xffu); }
  } else {
#pragma unroll
    for (int j = 0; j < 16; ++j) { long long p = first + (long long)dir * j; p = p < 0 ? 0 : (p > N - 1 ? N - 1 : p); out[j] = (int)A[p]; }
  }
}
__device__ inline void walk_load16(const int32_t* __restrict__ A, int64_t N, long long first, int dir, int* out) {
  const long long lo = dir > 0 ? first : first - 15;
  if (lo >= 0 && lo + 15 <= N - 1) {
    int v[16];
#pragma unroll
    for (int q = 0; q < 4; ++q) { const WalkInts4 b = *reinterpret_cast<const WalkInts4*>(A + lo + 4 * q); v[4 * q] = b.x; v[4 * q + 1] = b.y; v[4 * q + 2] = b.z; v[4 * q + 3] = b.w; }
#pragma unroll
    for (int j = 0; j < 16; ++j) out[j] = v[dir > 0 ? j : 15 - j];
  } else {
#pragma unroll
    for (int j = 0; j < 16; ++j) { long long p = first + (long long)dir * j; p = p < 0 ? 0 : (p > N - 1 ? N - 1 : p); out[j] = A[p]; }
  }
}

// What one thread holds of a trip: kPer consecutive positions in walk order.
// int32 storage: sixteen values as ints (16 384 positions per trip: the 64 KB stage holds that many ints).
// byte storage: sixty-four values packed in sixteen registers (65 536 positions per trip, the same 64 KB as bytes); unpacked
// they would be 2 x 64 registers with the trip loaded ahead.  The registers keep memory order; get() turns it for the walk to the left.
// swz: a thread's values have consecutive ranks, so the lanes of a wave write the stage kPer slots apart; the rank's
// bits that tell the lanes apart are XORed into the bits that choose the LDS bank.  A bijection on every aligned block.
template <typename TS> struct WalkTrip;
template <> struct WalkTrip<int32_t> {
  static constexpr int kPer = 16;
  typedef unsigned int Mask;
  int v[16];
  template <typename TD>
  __device__ inline void load(const TD* __restrict__ A, int64_t N, long long first, int dir) { walk_load16(A, N, first, dir, v); }
  __device__ inline int get(int j, int) const { return v[j]; }
  __device__ inline void pin(int, int) {}
  __device__ inline Mask extreme(int hi_lim, int lo_lim, int) const {   // bit j: value j is extreme
    Mask m = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) if (v[j] > hi_lim || v[j] < lo_lim) m |= (Mask)1 << j;
    return m;
  }
  __device__ static inline int swz(int r) { return r ^ ((r >> 4) & 15); }
};
template <> struct WalkTrip<uint8_t> {
  static constexpr int kPer = 64;
  typedef unsigned long long Mask;
  uint32_t w[16];   // the 64 bytes in memory order: value j of the walk is byte j (dir > 0) or 63 - j (dir < 0)
  // four 16-byte loads, requested together, where the 64 positions lie inside the array
  __device__ inline void load(const uint8_t* __restrict__ A, int64_t N, long long first, int dir) {
    const long long lo = dir > 0 ? first : first - 63;
    if (lo >= 0 && lo + 63 <= N - 1) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const WalkBytes16 b = *reinterpret_cast<const WalkBytes16*>(A + lo + 16 * q);
        w[4 * q] = b.w[0]; w[4 * q + 1] = b.w[1]; w[4 * q + 2] = b.w[2]; w[4 * q + 3] = b.w[3];
      }
    } else {   // clamped single loads at the chromosome's ends, a register at a time
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        uint32_t x = 0;
#pragma unroll
        for (int i = 4 * k; i < 4 * k + 4; ++i) { long long p = lo + i; p = p < 0 ? 0 : (p > N - 1 ? N - 1 : p); x |= (uint32_t)A[p] << (8 * (i & 3)); }
        w[k] = x;
      }
    }
  }
  __device__ inline int get(int j, int dir) const { const int i = dir > 0 ? j : 63 - j; return (int)((w[i >> 2] >> (8 * (i & 3))) & 0xffu); }
  // Called in front of the use of value j in an unrolled loop: keeps the unpacking of a register behind the work on the one
  // before it.  Left alone the compiler unpacks all sixty-four values first, and a workgroup of 1024 has 128 registers a thread.
  __device__ inline void pin(int j, int dir) { if ((j & 3) == 0) asm volatile("" : "+v"(w[(dir > 0 ? j : 63 - j) >> 2]) : : "memory"); }
  // bit j: value j is extreme.  Gathered in memory order, a register's four bits at a time behind a pin (sixty-four
  // one-bit terms would otherwise each get a register of their own), and mirrored for the walk to the left.
  __device__ inline Mask extreme(int hi_lim, int lo_lim, int dir) const {
    uint32_t half[2] = {0u, 0u};
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      uint32_t nib = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i) { const int x = (int)((w[k] >> (8 * i)) & 0xffu); if (x > hi_lim || x < lo_lim) nib |= 1u << i; }
      half[k >> 3] |= nib << (4 * (k & 7));
      asm volatile("" : "+v"(half[k >> 3]));
    }
    const Mask m = (Mask)half[0] | ((Mask)half[1] << 32);
    return dir > 0 ? m : (Mask)__brevll(m);
  }
  __device__ static inline int swz(int r) { return r ^ (((r >> 7) & 15) << 2); }
};

// One side of the reference gather (rsi.cpp:206-257).  dir = -1: left of the candidate, values land
// in dst[fill], dst[fill-1], ...; dir = +1: right, values land in dst[used], dst[used+1], ...
// Returns the number of values stored; *reach = last position examined.
// A trip examines kBlock positions in walk order (kPer consecutive ones per thread): which are
// taken (not extreme, not inside the neighbour the walk is about to meet), and where the walk first
// steps into that neighbour (the trigger, rsi.cpp:222-228 / 246-252: everything after it is dropped
// and the walk jumps).  One barrier per trip: the waves exchange their taken-counts and triggers; a
// second one only when there is a trigger, a third when the slots run out.
template <int dir, typename TD, typename TS>
__device__ inline int gather_side(const TD* __restrict__ A, int64_t N, int pos, int room /* slots left */,
                                  TS* __restrict__ dst, int first_slot, const int2* __restrict__ chain, int nchain,
                                  int kind, double too_high, double too_low, WalkShared& W, int* reach, int* chain_used,
                                  TS* __restrict__ stage /* LDS, kBlock values: a trip's taken values in rank order */) {
  typedef WalkTrip<TS> Trip;
  typedef typename Trip::Mask Mask;
  constexpr int kPer = Trip::kPer;
  constexpr int kBlock = kPer * kTestThreads;   // positions examined per trip
  static_assert((size_t)kBlock * sizeof(TS) <= (size_t)kWalkLds, "a trip's values fit the stage");
  constexpr int kNone = 0x7fffffff;
  auto bits_below = [](long long n) -> Mask {   // bits 0 .. n-1 of a thread's kPer positions
    const Mask all = kPer == 64 ? ~(Mask)0 : (Mask)((1ull << (kPer & 63)) - 1);
    return n <= 0 ? (Mask)0 : (n >= kPer ? all : (Mask)(((Mask)1 << n) - 1));
  };
  // A thread's values have consecutive ranks, so a store of value j by the 64 lanes of a wave would touch 64 cache
  // lines -- the walk spent most of its time in those stores.  The values go to LDS first (swizzled, see WalkTrip)
  // and leave as consecutive values per wave.
  int stored = 0, ci = 0, trip = 0;
  int last = pos;
  const int lane = lane_id(), wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
  // "extreme" for integer values: (double)v > too_high <=> v > floor(too_high), (double)v < too_low <=> v < ceil(too_low)
  // (rsi.cpp:213, 237); the limits are clamped into the int range first, which changes no comparison with an int
  const double th = too_high > 2147483646.0 ? 2147483646.0 : (too_high < -2147483647.0 ? -2147483647.0 : floor(too_high));
  const double tl = too_low > 2147483646.0 ? 2147483646.0 : (too_low < -2147483647.0 ? -2147483647.0 : ceil(too_low));
  const int hi_lim = kind == 0 && too_high == too_high ? (too_high > 2147483646.0 ? 0x7fffffff : (int)th) : 0x7fffffff;   // extreme: v > hi_lim (never for a NaN limit)
  const int lo_lim = kind == 1 && too_low == too_low ? (too_low < -2147483647.0 ? (int)0x80000000 : (int)tl) : (int)0x80000000;   // extreme: v < lo_lim
  // the values of a trip are loaded one trip ahead (the walk continues straight on unless it meets a
  // neighbour, which is rare)
  Trip vnext;
  auto load_trip = [&](int from) { vnext.load(A, N, (long long)from + (long long)dir * (1 + kPer * (int)threadIdx.x), dir); };
  load_trip(pos);
  // the neighbour the walk may meet next: read when it changes, not per trip (the list may sit in mapped host memory)
  int2 cur = ci < nchain ? chain[ci] : make_int2(1, 0);   // empty interval when the chain is used up
  while (room > 0 && (dir < 0 ? pos > 2 : (int64_t)pos < N - 2)) {
    const int par = trip & 1;
    ++trip;
    // positions of this trip in walk order: p_t = pos + dir*(1+t)
    const int avail = dir < 0 ? pos - 2 : (int)(N - 2 - pos);     // how many positions the walk may still visit
    const int cnt = avail < kBlock ? avail : kBlock;
    Trip v = vnext;
    load_trip(pos + dir * cnt);                                    // next trip, if the walk goes straight on
    const int t0 = kPer * (int)threadIdx.x;
    // one bit per position of this thread: which exist (t < cnt) and which lie inside the neighbour follow from the
    // coordinates alone, which are extreme from the values
    const Mask valid = bits_below(cnt - t0);
    const long long in_lo = dir > 0 ? (long long)cur.x - pos - 1 : (long long)pos - 1 - cur.y;   // inside <=> in_lo <= t <= in_hi
    const long long in_hi = dir > 0 ? (long long)cur.y - pos - 1 : (long long)pos - 1 - cur.x;
    const Mask inside = bits_below(in_hi - t0 + 1) & ~bits_below(in_lo - t0);
    const Mask extm = v.extreme(hi_lim, lo_lim, dir);
    const Mask accm = valid & ~extm & ~inside;                     // taken unless a trigger in front of them drops them
    const Mask hits = valid & ~extm & inside;                      // the first of these in the block is the trigger
    const int nacc = __popcll((unsigned long long)accm);
    const int trig = hits ? t0 + __ffsll((unsigned long long)hits) - 1 : kNone;
    int incl = wave_incl_scan(nacc), wtrig = trig;
    for (int d = 32; d >= 1; d >>= 1) { const int o = __shfl_xor(wtrig, d); wtrig = o < wtrig ? o : wtrig; }
    if (lane == 63) W.cnt[par][wave] = incl;
    if (lane == 0) W.trg[par][wave] = wtrig;
    __syncthreads();
    int base = 0, all = 0, tstar = kNone;
    for (int w = 0; w < nwaves; ++w) { const int c = W.cnt[par][w]; if (w < wave) base += c; all += c; const int g = W.trg[par][w]; tstar = g < tstar ? g : tstar; }
    int rank = base + incl - nacc;             // rank of this thread's first taken value if nothing were dropped
    int total = all;
    if (tstar != kNone) {                       // values taken before the trigger = the trigger position's rank
      if ((int)threadIdx.x == tstar / kPer) {
        W.kept[par] = rank + __popcll((unsigned long long)(accm & bits_below(tstar - t0)));
      }
      __syncthreads();
      total = W.kept[par];
    }
    const bool fills = total >= room;
    const Mask keep = tstar != kNone ? accm & bits_below((long long)tstar - t0) : accm;
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      v.pin(j, dir);
      if ((keep >> j) & 1u) {
        if (rank < room) stage[Trip::swz(rank)] = (TS)v.get(j, dir);
        if (fills && rank == room - 1) W.lastt[par] = t0 + j;   // the value that fills the last slot
        ++rank;
      }
    }
    __syncthreads();
    {
      const int ncopy = total < room ? total : room;
      for (int e = threadIdx.x; e < ncopy; e += blockDim.x) dst[first_slot + dir * (stored + e)] = stage[Trip::swz(e)];
    }   // the next trip writes `stage` only behind its own exchange barrier, which every thread reaches after this loop
    if (fills) {   // the walk stops right after the value that filled the last slot
      last = pos + dir * (1 + W.lastt[par]);
      stored += room; room = 0;
      break;
    }
    stored += total; room -= total;
    if (tstar != kNone) {      // jump over the neighbour
      last = pos + dir * (1 + tstar);
      pos = dir < 0 ? cur.x - 1 : cur.y + 1;
      ++ci;
      cur = ci < nchain ? chain[ci] : make_int2(1, 0);
      load_trip(pos);          // the prefetch was for the straight continuation
    } else {
      pos += dir * cnt;
      last = pos;
    }
  }
  __syncthreads();   // the next user of W (or of dst) starts from a quiet block
  *reach = last;
  *chain_used = ci;
  return stored;
}

// Buckets where the cumulated count first reaches n/4, n/2, 3n/4 (partition_stat_tp's walk,
// wufunctions.cpp:398-420), -1 where it never does; every thread gets the result.
__device__ inline void hist_ranks(const unsigned int* hist, unsigned nbk, size_t n, int* s_scan, int* s_q, int* out) {
  const size_t r1 = n / 4, r2 = n / 2, r3 = n * 3 / 4;
  if (threadIdx.x < 3) s_q[threadIdx.x] = -1;
  const unsigned chunk = (nbk + blockDim.x - 1) / blockDim.x;
  const unsigned b0 = threadIdx.x * chunk;
  int local = 0;
  for (unsigned b = b0; b < b0 + chunk && b < nbk; ++b) local += (int)hist[b];
  int total;
  size_t seen = (size_t)block_exscan(local, s_scan, &total);   // syncs: s_q is initialised before any write below
  for (unsigned b = b0; b < b0 + chunk && b < nbk; ++b) {
    const size_t upto = seen + hist[b];
    if (seen < r1 && upto >= r1) s_q[0] = (int)b;
    if (seen < r2 && upto >= r2) s_q[1] = (int)b;
    if (seen < r3 && upto >= r3) s_q[2] = (int)b;
    seen = upto;
  }
  __syncthreads();
  out[0] = s_q[0]; out[1] = s_q[1]; out[2] = s_q[2];
  __syncthreads();
}

// The scratch of one test (the host sizes it the same way, DeviceTester::test): the gathered values -- left part, thinned
// copy, the split form's right part -- in `vb` bytes each (1 or 4: the storage type of the launch), the window means as
// floats in `ref` (which the one-workgroup form fills with the neighbourhood's values first), the prefixes in P.  Every
// piece starts on a 16-byte boundary.
struct CandBufs { unsigned char *left, *thin, *right; int32_t* ref; long long* P; };
__device__ inline CandBufs cand_buffers(const CandJob& J, int32_t* iscratch, long long* lscratch, int vb) {
  auto up16 = [](size_t x) { return (x + 15) & ~size_t(15); };
  CandBufs b;
  unsigned char* p = reinterpret_cast<unsigned char*>(iscratch + J.iscratch_off);
  b.left = p; p += up16((size_t)(J.top + 1 > 0 ? J.top + 1 : 0) * vb);
  b.ref = reinterpret_cast<int32_t*>(p); p += up16((size_t)J.capacity * 4);
  b.thin = p; p += up16((size_t)(J.capacity < J.budget ? J.capacity : J.budget) * vb);
  b.right = p;
  b.P = lscratch ? lscratch + J.lscratch_off : nullptr;   // the split form has no prefix array
  return b;
}
// four consecutive stored values from a 4-aligned index of a piece
__device__ inline int4 cand_load4(const int32_t* p) { return *reinterpret_cast<const int4*>(p); }
__device__ inline int4 cand_load4(const uint8_t* p) {
  const uint32_t u = *reinterpret_cast<const uint32_t*>(p);
  return make_int4((int)(u & 0xffu), (int)((u >> 8) & 0xffu), (int)((u >> 16) & 0xffu), (int)(u >> 24));
}

template <typename TD, typename TS>
__global__ __launch_bounds__(kTestThreads) void k_candidate_test(const TD* __restrict__ A, int64_t N,
                                                             const CandJob* __restrict__ jobs, const int2* __restrict__ chains,
                                                             int32_t* __restrict__ iscratch, long long* __restrict__ lscratch,
                                                             double RDmedian, CandOut* __restrict__ outs) {
  extern __shared__ unsigned int s_hist[];   // kCandHistBins counters
  __shared__ WalkShared W;
  __shared__ double s_d[kMaxWaves];
  __shared__ float s_f[kMaxWaves];
  __shared__ long long s_l[kMaxWaves];
  __shared__ long long s_x[2][4 * kMaxWaves];   // prefix rounds: wave totals of four tiles, by round parity
  __shared__ int s_i2[kMaxWaves];
  __shared__ int s_q[3];
  const CandJob J = jobs[blockIdx.x];
  CandOut O;
  O.flags = 0;
  const CandBufs B = cand_buffers(J, iscratch, lscratch, (int)sizeof(TS));
  TS* left = reinterpret_cast<TS*>(B.left);     // J.top + 1 slots
  TS* ref = reinterpret_cast<TS*>(B.ref);       // J.capacity slots (sized for the float means that replace the values)
  TS* thin = reinterpret_cast<TS*>(B.thin);     // min(capacity, budget) slots
  long long* P = B.P;                           // capacity + 1
  const double too_high = RDmedian * 3.0, too_low = RDmedian * 0.15;

  // ---- gather: left side into left[top..], then ref = left part ++ right part ----
  int lreach = J.start, rreach = J.end;
  int lcnt = 0, lused = 0, rused = 0;
  if (J.top >= 0)
    lcnt = gather_side<-1>(A, N, J.start - J.margin, J.top + 1, left, J.top, chains + J.left_off, J.nleft, J.kind, too_high, too_low, W, &lreach, &lused, reinterpret_cast<TS*>(s_hist));
  __syncthreads();
  // the reference closes the gap when the left side ran out of sequence, otherwise used = top + 1 (rsi.cpp:231-236)
  const int used0 = lcnt < J.top + 1 ? lcnt : J.top + 1;
  for (int j0 = threadIdx.x; j0 < used0; j0 += 8 * kTestThreads) {   // eight independent loads per round
    TS x[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) { const int j = j0 + k * kTestThreads; x[k] = left[J.top + 1 - used0 + (j < used0 ? j : j0)]; }
#pragma unroll
    for (int k = 0; k < 8; ++k) { const int j = j0 + k * kTestThreads; if (j < used0) ref[j] = x[k]; }
  }
  __syncthreads();
  int room = J.capacity - used0;
  {   // `used < 2*chklen*d` with the double right-hand side (rsi.cpp:243)
    const int lim = (int)ceil(J.right_cap);
    if (lim - used0 < room) room = lim - used0;
    if (room < 0) room = 0;
  }
  const int rcnt = gather_side<+1>(A, N, J.end + J.margin, room, ref, used0, chains + J.right_off, J.nright, J.kind, too_high, too_low, W, &rreach, &rused, reinterpret_cast<TS*>(s_hist));
  __syncthreads();
  // a chain the host cut short was consumed to its end: the walk may have missed a neighbour
  if (((J.cut & 1) && lused >= J.nleft) || ((J.cut & 2) && rused >= J.nright)) O.flags |= 8;
  int nref = used0 + rcnt;
  int nbody = J.end - J.start + 1;
  // ---- thinning to about `budget` points (rsi.cpp:264-282) ----
  const TS* R = ref;
  int body_len = nbody;       // source length of the body
  bool thin_body = false;
  int nbody_eff = nbody;
  if (nref + nbody > J.budget) {
    const int total = nref + nbody;
    const int tref = (int)((double)nref / (double)total * (double)J.budget);
    const int tbody = (int)((double)nbody / (double)total * (double)J.budget);
    for (int q0 = threadIdx.x; q0 < tref; q0 += 8 * kTestThreads) {   // eight independent loads per round
      TS x[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) { const int q = q0 + k * kTestThreads; x[k] = ref[(int)((double)(q < tref ? q : q0) / (double)tref * (double)nref)]; }
#pragma unroll
      for (int k = 0; k < 8; ++k) { const int q = q0 + k * kTestThreads; if (q < tref) thin[q] = x[k]; }
    }
    __syncthreads();
    R = thin; nref = tref; thin_body = true; nbody_eff = tbody;
  }
  auto body_at = [&](int q) -> int {
    return (int)(thin_body ? A[J.start + (int)((double)q / (double)nbody_eff * (double)body_len)] : A[J.start + q]);
  };
  const int width = nbody_eff;
  const int nwin = nref - width;
  O.nref = nref; O.nbody = nbody_eff; O.nwin = nwin; O.left_reach = lreach; O.right_reach = rreach;
  if (nwin <= 0 || width <= 0) { O.flags |= 1; if (threadIdx.x == 0) outs[blockIdx.x] = O; return; }

  // ---- body statistics: integer histogram quantiles (partition_stat_tp with dy = 1), sum, sum of squares ----
  {
    int lo = 0x7fffffff, hi = (int)0x80000000; long long s1 = 0, s2 = 0;
    for (int q0 = threadIdx.x; q0 < width; q0 += 8 * kTestThreads) {   // eight independent loads per round (see k_cand_sums)
      int x[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) { const int q = q0 + k * kTestThreads; x[k] = body_at(q < width ? q : q0); }
#pragma unroll
      for (int k = 0; k < 8; ++k) if (q0 + k * kTestThreads < width) { lo = x[k] < lo ? x[k] : lo; hi = x[k] > hi ? x[k] : hi; s1 += x[k]; s2 += (long long)x[k] * x[k]; }
    }
    lo = block_reduce(lo, [](int a, int b) { return a < b ? a : b; }, s_i2);
    hi = block_reduce(hi, [](int a, int b) { return a > b ? a : b; }, s_i2);
    s1 = block_reduce(s1, [](long long a, long long b) { return a + b; }, s_l);
    s2 = block_reduce(s2, [](long long a, long long b) { return a + b; }, s_l);
    O.body_min = lo; O.body_max = hi; O.body_s1 = (double)s1; O.body_s2 = (double)s2;
    O.body_q[0] = lo; O.body_q[1] = (double)s1 / (double)width; O.body_q[2] = hi;
    if ((double)hi - (double)lo >= 1.0) {
      const unsigned nbk = (unsigned)(hi - lo) + 2;
      if (nbk > kCandHistBins) O.flags |= 2;
      else {
        for (unsigned e = threadIdx.x; e < nbk; e += kTestThreads) s_hist[e] = 0;
        __syncthreads();
        for (int q0 = threadIdx.x; q0 < width; q0 += 8 * kTestThreads) {
          int x[8];
#pragma unroll
          for (int k = 0; k < 8; ++k) { const int q = q0 + k * kTestThreads; x[k] = body_at(q < width ? q : q0); }
#pragma unroll
          for (int k = 0; k < 8; ++k) if (q0 + k * kTestThreads < width) atomicAdd(&s_hist[x[k] - lo], 1u);
        }
        __syncthreads();
        int qb[3];
        hist_ranks(s_hist, nbk, (size_t)width, W.s_scan, s_q, qb);
        if (qb[0] >= 0) O.body_q[0] = (double)lo + qb[0] * 1.0;
        if (qb[1] >= 0) O.body_q[1] = (double)lo + qb[1] * 1.0;
        if (qb[2] >= 0) O.body_q[2] = (double)lo + qb[2] * 1.0;
        __syncthreads();
      }
    }
  }
  // ---- running mean of width `width` over the neighbourhood (rsi.cpp:113-124): exact prefix, float means ----
  {   // rounds of four tiles (4096 values each, four consecutive values per thread and tile, one load each): the
      // four wave scans of a round share ONE barrier, the exchange buffer alternates with the round's parity
    constexpr int kTile = 4 * kTestThreads, kRound = 4 * kTile;
    long long carry = 0;
    if (threadIdx.x == 0) P[0] = 0;
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    auto load_tile = [&](int t0) {
      const int e = t0 + 4 * (int)threadIdx.x;
      int4 v = make_int4(0, 0, 0, 0);
      if (e + 3 < nref) v = cand_load4(R + e);
      else { if (e < nref) v.x = (int)R[e]; if (e + 1 < nref) v.y = (int)R[e + 1]; if (e + 2 < nref) v.z = (int)R[e + 2]; }
      return v;
    };
    int4 nx0 = load_tile(0), nx1 = load_tile(kTile), nx2 = load_tile(2 * kTile), nx3 = load_tile(3 * kTile);
    int par = 0;
    for (int t0 = 0; t0 < nref; t0 += kRound, par ^= 1) {
      const int4 v0 = nx0, v1 = nx1, v2 = nx2, v3 = nx3;
      if (t0 + kRound < nref) {   // the next round's loads fly during this round's scans
        nx0 = load_tile(t0 + kRound); nx1 = load_tile(t0 + kRound + kTile);
        nx2 = load_tile(t0 + kRound + 2 * kTile); nx3 = load_tile(t0 + kRound + 3 * kTile);
      }
      // named variables only: a runtime-indexed array would live in scratch memory
      auto quad = [](const int4& v) { return (long long)v.x + v.y + v.z + v.w; };
      long long i0 = quad(v0), i1 = quad(v1), i2 = quad(v2), i3 = quad(v3);   // inclusive wave scans of the quad sums
      i0 = wave_incl_scan(i0); i1 = wave_incl_scan(i1); i2 = wave_incl_scan(i2); i3 = wave_incl_scan(i3);   // DPP: no LDS round trips
      long long* X = s_x[par];   // [4][kMaxWaves] wave totals
      if (lane == 63) { X[wave] = i0; X[kMaxWaves + wave] = i1; X[2 * kMaxWaves + wave] = i2; X[3 * kMaxWaves + wave] = i3; }
      __syncthreads();
      long long b0 = 0, b1 = 0, b2 = 0, b3 = 0, T0 = 0, T1 = 0, T2 = 0, T3 = 0;
#pragma unroll 1
      for (int w = 0; w < kMaxWaves; ++w) {
        const long long c0 = X[w], c1 = X[kMaxWaves + w], c2 = X[2 * kMaxWaves + w], c3 = X[3 * kMaxWaves + w];
        if (w < wave) { b0 += c0; b1 += c1; b2 += c2; b3 += c3; }
        T0 += c0; T1 += c1; T2 += c2; T3 += c3;
      }
      auto store_quad = [&](int e, const int4& v, long long before) {   // P[e+1..e+4] = before + running sums of v
        const long long a1 = before + v.x, a2 = a1 + v.y, a3 = a2 + v.z, a4 = a3 + v.w;
        if (e < nref) P[e + 1] = a1;
        if (e + 1 < nref) P[e + 2] = a2;
        if (e + 2 < nref) P[e + 3] = a3;
        if (e + 3 < nref) P[e + 4] = a4;
      };
      const int e = t0 + 4 * (int)threadIdx.x;
      store_quad(e, v0, carry + b0 + i0 - quad(v0));
      store_quad(e + kTile, v1, carry + T0 + b1 + i1 - quad(v1));
      store_quad(e + 2 * kTile, v2, carry + T0 + T1 + b2 + i2 - quad(v2));
      store_quad(e + 3 * kTile, v3, carry + T0 + T1 + T2 + b3 + i3 - quad(v3));
      carry += T0 + T1 + T2 + T3;
    }
    __syncthreads();
  }
  const double dw = (double)width;
  // the means are kept (as floats, over the neighbourhood values, which are not needed any more) for the histogram pass
  float* Wm = reinterpret_cast<float*>(B.ref);
  {
    float flo = 3.0e38f, fhi = -3.0e38f; double m1 = 0, m2 = 0;
    for (int i = threadIdx.x; i < nwin; i += 4 * kTestThreads) {
      long long hi4[4], lo4[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) { const int q = i + k * kTestThreads; const int qq = q < nwin ? q : i; hi4[k] = P[qq + width]; lo4[k] = P[qq]; }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int q = i + k * kTestThreads;
        if (q < nwin) {
          const float w = (float)((double)(hi4[k] - lo4[k]) / dw);
          Wm[q] = w;
          flo = w < flo ? w : flo; fhi = w > fhi ? w : fhi; m1 += (double)w; m2 += (double)w * (double)w;
        }
      }
    }
    flo = block_reduce(flo, [](float a, float b) { return a < b ? a : b; }, s_f);
    fhi = block_reduce(fhi, [](float a, float b) { return a > b ? a : b; }, s_f);
    m1 = block_reduce(m1, [](double a, double b) { return a + b; }, s_d);
    m2 = block_reduce(m2, [](double a, double b) { return a + b; }, s_d);
    const double lo = flo, hi = fhi;
    O.ref_s1 = m1; O.ref_s2 = m2;
    O.ref_q[0] = lo; O.ref_q[1] = m1 / (double)nwin; O.ref_q[2] = hi;
    if ((hi - lo) >= 0.01) {
      const size_t nbk = (size_t)((hi - lo) / 0.01 + 2);
      if (nbk > kCandHistBins) O.flags |= 4;
      else {
        for (unsigned e = threadIdx.x; e < nbk; e += kTestThreads) s_hist[e] = 0;
        __syncthreads();
        // neighbouring windows differ by one value in `width`, so their means mostly share a bucket:
        // every thread takes eight consecutive means and merges equal buckets before touching LDS
        for (int i0 = 8 * (int)threadIdx.x; i0 < nwin; i0 += 8 * kTestThreads) {
          float w8[8];
          if (i0 + 7 < nwin) {
            const float4 a = *reinterpret_cast<const float4*>(Wm + i0), b = *reinterpret_cast<const float4*>(Wm + i0 + 4);
            w8[0] = a.x; w8[1] = a.y; w8[2] = a.z; w8[3] = a.w; w8[4] = b.x; w8[5] = b.y; w8[6] = b.z; w8[7] = b.w;
          } else {
#pragma unroll
            for (int k = 0; k < 8; ++k) w8[k] = Wm[i0 + k < nwin ? i0 + k : i0];
          }
          unsigned pend_b = 0xffffffffu, pend_c = 0;
#pragma unroll
          for (int k = 0; k < 8; ++k) {
            if (i0 + k < nwin) {
              const double idx = ((double)w8[k] - lo) / 0.01 + 0.5;   // wufunctions.cpp:396
              const unsigned bkt = (unsigned)(unsigned long long)idx;
              if (bkt != pend_b) { if (pend_c) atomicAdd(&s_hist[pend_b], pend_c); pend_b = bkt; pend_c = 0; }
              ++pend_c;
            }
          }
          if (pend_c) atomicAdd(&s_hist[pend_b], pend_c);
        }
        __syncthreads();
        int qb[3];
        hist_ranks(s_hist, (unsigned)nbk, (size_t)nwin, W.s_scan, s_q, qb);
        if (qb[0] >= 0) O.ref_q[0] = lo + qb[0] * 0.01;
        if (qb[1] >= 0) O.ref_q[1] = lo + qb[1] * 0.01;
        if (qb[2] >= 0) O.ref_q[2] = lo + qb[2] * 0.01;
        __syncthreads();
      }
    }
  }
  if (threadIdx.x == 0) outs[blockIdx.x] = O;
}

// ------------------------------------------------------------------------------------------
// The neighbourhood test over several workgroups.  Same arithmetic as k_candidate_test (see there for the reference
// lines); only the order in which the two float moments of the window means are summed differs (a thread's sixteen
// consecutive windows, the chunk's threads as a tree, then a fixed order over the chunks).  The neighbourhood is not
// materialised: ref(j) = left part ++ right part is read in place.
struct CandGeom { int used0, rcnt, nref_raw, nref, nbody, nbody_eff, width, nwin; bool thin; };

__device__ inline CandGeom cand_geometry(const CandJob& J, const CandMid& M) {
  CandGeom g;
  g.used0 = J.top >= 0 ? (M.lcnt < J.top + 1 ? M.lcnt : J.top + 1) : 0;
  int room = J.capacity - g.used0;
  const int lim = (int)ceil(J.right_cap);                  // `used < 2*chklen*d` (rsi.cpp:243)
  if (lim - g.used0 < room) room = lim - g.used0;
  if (room < 0) room = 0;
  g.rcnt = M.rcnt_max < room ? M.rcnt_max : room;
  g.nref_raw = g.used0 + g.rcnt;
  g.nbody = J.end - J.start + 1;
  g.nref = g.nref_raw; g.nbody_eff = g.nbody; g.thin = false;
  if (g.nref_raw + g.nbody > J.budget) {                    // thinning (rsi.cpp:264-282)
    const int total = g.nref_raw + g.nbody;
    g.nref = (int)((double)g.nref_raw / (double)total * (double)J.budget);
    g.nbody_eff = (int)((double)g.nbody / (double)total * (double)J.budget);
    g.thin = true;
  }
  g.width = g.nbody_eff;
  g.nwin = g.nref - g.width;
  return g;
}
// element i of the (possibly thinned) neighbourhood
template <typename TS>
__device__ inline int cand_value(const CandJob& J, const CandGeom& g, const TS* __restrict__ left, const TS* __restrict__ right, int i) {
  const int j = g.thin ? (int)((double)i / (double)g.nref * (double)g.nref_raw) : i;
  return (int)(j < g.used0 ? left[J.top + 1 - g.used0 + j] : right[j - g.used0]);
}
__device__ inline int cand_chunk_len(int n) { return (((n + kCandChunks - 1) / kCandChunks) + 3) & ~3; }
// launch 1: grid (2, njobs) -- the left and the right walk of every test side by side
template <typename TD, typename TS>
__global__ __launch_bounds__(kTestThreads) void k_cand_gather(const TD* __restrict__ A, int64_t N, const CandJob* __restrict__ jobs,
                                                          const int2* __restrict__ chains, int32_t* __restrict__ iscratch,
                                                          long long* __restrict__ lscratch, double RDmedian, CandMid* __restrict__ mid) {
  __shared__ WalkShared W;
  extern __shared__ int s_stage_raw[];   // kWalkLds bytes: a trip's taken values on their way to coalesced stores
  TS* const s_stage = reinterpret_cast<TS*>(s_stage_raw);
  const CandJob J = jobs[blockIdx.y];
  const CandBufs b = cand_buffers(J, iscratch, lscratch, (int)sizeof(TS));
  const double too_high = RDmedian * 3.0, too_low = RDmedian * 0.15;
  CandMid& M = mid[blockIdx.y];
  if (blockIdx.x == 0) {
    int lreach = J.start, lused = 0, lcnt = 0;
    if (J.top >= 0)
      lcnt = gather_side<-1>(A, N, J.start - J.margin, J.top + 1, reinterpret_cast<TS*>(b.left), J.top, chains + J.left_off, J.nleft, J.kind, too_high, too_low, W, &lreach, &lused, s_stage);
    if (threadIdx.x == 0) { M.lcnt = lcnt; M.lreach = lreach; M.lused = lused; }
  } else {
    // The right walk does not know yet how many slots the left one leaves.  Where the host vouches that the left walk fills
    // all of its top + 1 slots (J.cut bit 2: more than twice as many positions to the left, known neighbours taken off, as
    // slots -- it would take every other base to be extreme for that to fail, and k_cand_hist checks: flag 16 sends the test
    // to the host path) the right walk takes what is left, about half the capacity; else as many as it could ever get.  The
    // right walk is the launch's critical path: a trip of 16 384 positions at a time (65 536 with byte storage), twice as many
    // trips as needed before.
    int room = J.capacity;
    const int lim = (int)ceil(J.right_cap);
    if (lim < room) room = lim;
    if ((J.cut & 4) && J.top >= 0) room -= J.top + 1;
    if (room < 0) room = 0;
    int rreach = J.end, rused = 0;
    const int rcnt = gather_side<+1>(A, N, J.end + J.margin, room, reinterpret_cast<TS*>(b.right), 0, chains + J.right_off, J.nright, J.kind, too_high, too_low, W, &rreach, &rused, s_stage);
    if (threadIdx.x == 0) { M.rcnt_max = rcnt; M.rreach = rreach; M.rused = rused; }
  }
}

// Sixteen consecutive values of the neighbourhood as a thread holds them: in the width they are stored in, so that the
// sixteen bytes of a load stay four registers until a value is used.
template <typename TS> struct CandRun16;
template <> struct CandRun16<uint8_t> {
  uint32_t w[4];
  __device__ inline void clear() { w[0] = w[1] = w[2] = w[3] = 0u; }
  __device__ inline void load(const uint8_t* p) { const WalkBytes16 b = *reinterpret_cast<const WalkBytes16*>(p); w[0] = b.w[0]; w[1] = b.w[1]; w[2] = b.w[2]; w[3] = b.w[3]; }
  __device__ inline void put(int k, int x) { w[k >> 2] |= (uint32_t)x << (8 * (k & 3)); }   // behind clear(), k a constant
  __device__ inline int get(int k) const { return (int)((w[k >> 2] >> (8 * (k & 3))) & 0xffu); }
  __device__ inline long long sum() const {   // four bytes a step: sum of absolute differences against zero
    unsigned s = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) s = __builtin_amdgcn_sad_u8(w[q], 0u, s);
    return (long long)s;
  }
};
template <> struct CandRun16<int32_t> {
  int v[16];
  __device__ inline void clear() {
#pragma unroll
    for (int k = 0; k < 16; ++k) v[k] = 0;
  }
  __device__ inline void load(const int32_t* p) {
#pragma unroll
    for (int q = 0; q < 4; ++q) { const WalkInts4 b = *reinterpret_cast<const WalkInts4*>(p + 4 * q); v[4 * q] = b.x; v[4 * q + 1] = b.y; v[4 * q + 2] = b.z; v[4 * q + 3] = b.w; }
  }
  __device__ inline void put(int k, int x) { v[k] = x; }
  __device__ inline int get(int k) const { return v[k]; }
  __device__ inline long long sum() const {
    long long s = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) s += v[k];
    return s;
  }
};
// ref(i0 .. i0 + 15); those at `lim` and beyond come back as 0.  Where the sixteen lie on one side of the seam at used0 and
// nothing is thinned: ONE 16-byte load of stored bytes, four of stored ints (a load per value makes the 64 lanes of every
// load touch 64 cache lines, sixteen times over); else a value at a time through cand_value.
template <typename TS>
__device__ inline void cand_load16(const CandJob& J, const CandGeom& g, const TS* __restrict__ left, const TS* __restrict__ right,
                                   int i0, int lim, CandRun16<TS>& r) {
  if (!g.thin && i0 + 16 <= lim && (i0 + 16 <= g.used0 || i0 >= g.used0)) {
    r.load(i0 < g.used0 ? left + (J.top + 1 - g.used0 + i0) : right + (i0 - g.used0));
  } else {
    r.clear();
#pragma unroll
    for (int k = 0; k < 16; ++k) if (i0 + k < lim) r.put(k, cand_value(J, g, left, right, i0 + k));
  }
}

// How many of the kCandChunks workgroups share a job's windows.  Every chunk sums its first window by itself (`width`
// values), so that no chunk waits for another; with all sixteen that is 16 x width values, 3.2 x nref at the default
// -reflen (nref = 5 x width).  Where the candidate is long against its window count the job takes fewer, longer chunks:
// as many as keep chunks x width <= 4 x nref (at least four, since nref > width where there is a window at all).
__device__ inline int cand_sum_chunks(const CandGeom& g) {
  const long long fit = 4ll * g.nref / g.width;
  return fit < kCandChunks ? (int)fit : kCandChunks;
}
__device__ inline int cand_sum_chunk_len(int nwin, int chunks) { return (((nwin + chunks - 1) / chunks) + 3) & ~3; }   // cand_chunk_len for all sixteen

// launch 2: grid (kCandChunks + 1, njobs) -- float window means of a chunk of windows, their extremes and moments, from
// exact window sums by sliding differences: S(q + 1) = S(q) + ref(q + width) - ref(q).  No prefix array: a chunk sums its
// first window outright, then takes rounds of 16 x 1024 windows -- sixteen consecutive ones per thread, their differences
// from two 16-byte loads, ONE exact int64 block scan of the per-thread totals, a carry from round to round.  Every sum is
// the integer the prefix difference was, so every mean is the same float.  The last workgroup of a job computes the
// candidate's own statistics meanwhile.
template <typename TD, typename TS>
__global__ __launch_bounds__(kTestThreads) void k_cand_sums(const TD* __restrict__ A, const CandJob* __restrict__ jobs,
                                                        int32_t* __restrict__ iscratch, CandMid* __restrict__ mid) {
  extern __shared__ unsigned int s_hist[];   // kCandHistBins counters (candidate statistics only)
  __shared__ long long s_l[kMaxWaves];       // also the double moments' exchange
  __shared__ int s_i2[kMaxWaves];            // also the float extremes' exchange
  __shared__ int s_scan[kMaxWaves];
  __shared__ int s_q[3];
  const CandJob J = jobs[blockIdx.y];
  CandMid& M = mid[blockIdx.y];
  const CandGeom g = cand_geometry(J, M);
  const CandBufs b = cand_buffers(J, iscratch, nullptr, (int)sizeof(TS));
  const TS* const left = reinterpret_cast<const TS*>(b.left);
  const TS* const right = reinterpret_cast<const TS*>(b.right);
  if (g.nwin <= 0 || g.width <= 0) return;
  const int width = g.width;
  if (blockIdx.x < kCandChunks) {
    constexpr int kPer = 16, kRound = kPer * kTestThreads;
    const int chunks = cand_sum_chunks(g);
    const int Wc = cand_sum_chunk_len(g.nwin, chunks);
    const int wb = (int)blockIdx.x < chunks ? (int)blockIdx.x * Wc : g.nwin;
    int we = wb + Wc; if (we > g.nwin) we = g.nwin;
    float flo = 3.0e38f, fhi = -3.0e38f; double m1 = 0, m2 = 0;
    if (wb >= we) {   // a chunk without windows leaves the neutral elements
      if (threadIdx.x == 0) { M.flo[blockIdx.x] = flo; M.fhi[blockIdx.x] = fhi; M.m1[blockIdx.x] = m1; M.m2[blockIdx.x] = m2; }
      return;
    }
    // ---- the first window's sum: a plain reduction, four blocks of sixteen values in flight per thread ----
    long long carry = 0;
    {
      const int lim = wb + width;
      for (int i0 = wb + kPer * (int)threadIdx.x; i0 < lim; i0 += 4 * kRound) {
        CandRun16<TS> v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) cand_load16(J, g, left, right, i0 + r * kRound, lim, v[r]);
#pragma unroll
        for (int r = 0; r < 4; ++r) carry += v[r].sum();
      }
      carry = block_reduce(carry, [](long long a, long long b2) { return a + b2; }, s_l);
    }
    // ---- the other windows by differences (depths are not negative, so a difference of two fits an int) ----
    float* const Wm = reinterpret_cast<float*>(b.ref);
    const double dw = (double)width;
    for (int q0 = wb; q0 < we; q0 += kRound) {
      const int e = q0 + kPer * (int)threadIdx.x;
      CandRun16<TS> out, in;   // the values that leave the sixteen windows and those that enter them
      cand_load16(J, g, left, right, e, we, out);
      cand_load16(J, g, left, right, e + width, we + width, in);
      int d[kPer];
      long long run = 0;
#pragma unroll
      for (int k = 0; k < kPer; ++k) { d[k] = in.get(k) - out.get(k); run += d[k]; }
      long long total;
      long long S = carry + block_exscan_i64(run, s_l, &total);   // the sum of window e
      float w[kPer];
#pragma unroll
      for (int k = 0; k < kPer; ++k) { w[k] = (float)((double)S / dw); S += d[k]; }
      if (e + kPer <= we) {   // e is a multiple of four (so is every chunk's length): 16-byte stores
#pragma unroll
        for (int q = 0; q < 4; ++q) *reinterpret_cast<float4*>(Wm + e + 4 * q) = make_float4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
      } else {
#pragma unroll
        for (int k = 0; k < kPer; ++k) if (e + k < we) Wm[e + k] = w[k];
      }
#pragma unroll
      for (int k = 0; k < kPer; ++k)
        if (e + k < we) { flo = w[k] < flo ? w[k] : flo; fhi = w[k] > fhi ? w[k] : fhi; m1 += (double)w[k]; m2 += (double)w[k] * (double)w[k]; }
      carry += total;
    }
    flo = block_reduce(flo, [](float a, float b2) { return a < b2 ? a : b2; }, reinterpret_cast<float*>(s_i2));
    fhi = block_reduce(fhi, [](float a, float b2) { return a > b2 ? a : b2; }, reinterpret_cast<float*>(s_i2));
    m1 = block_reduce(m1, [](double a, double b2) { return a + b2; }, reinterpret_cast<double*>(s_l));
    m2 = block_reduce(m2, [](double a, double b2) { return a + b2; }, reinterpret_cast<double*>(s_l));
    if (threadIdx.x == 0) { M.flo[blockIdx.x] = flo; M.fhi[blockIdx.x] = fhi; M.m1[blockIdx.x] = m1; M.m2[blockIdx.x] = m2; }
    return;
  }
  // ---- candidate statistics: integer histogram quantiles (partition_stat_tp with dy = 1), sum, sum of squares ----
  auto body_at = [&](int q) -> int {
    return (int)(g.thin ? A[J.start + (int)((double)q / (double)g.nbody_eff * (double)g.nbody)] : A[J.start + q]);
  };
  int lo = 0x7fffffff, hi = (int)0x80000000; long long s1 = 0, s2 = 0;
  if (sizeof(TD) == 1 && !g.thin) {
    // Byte depth, no thinning (the usual case): ONE pass with 16-byte loads -- sixteen values each, four loads in flight per
    // thread -- into a histogram over the byte values themselves; minimum, maximum, sum and sum of squares follow from its 256
    // counters exactly, and the quantile walk starts at the minimum's counter.  The general form below reads the candidate
    // twice, a value per load: 100 us for a candidate of 200 000 bases, the longest workgroup of the launch by far.
    // At 30x nearly every base falls into some twenty values, and the lanes of an LDS atomic that meet on a counter take
    // turns.  So every value has a counter per bank, [256][32], and a lane adds to the column of its own bank: the 32 lanes
    // the LDS serves together never meet.  (A set of counters per wave would not help: waves take turns at the LDS anyway,
    // it is the lanes of ONE instruction that collide.)  Folded into 256 counters behind the pass, 260 for the walk.
    constexpr unsigned kCols = 32, kFold = 256 * kCols;
    for (unsigned e = threadIdx.x; e < kFold + 260; e += kTestThreads) s_hist[e] = 0;
    __syncthreads();
    const unsigned col = threadIdx.x & (kCols - 1);
    const uint8_t* B = reinterpret_cast<const uint8_t*>(A) + J.start;
    for (int q0 = 16 * (int)threadIdx.x; q0 < width; q0 += 4 * 16 * kTestThreads) {
      WalkBytes16 v[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int q = q0 + k * 16 * kTestThreads;
        if (q + 16 <= width) v[k] = *reinterpret_cast<const WalkBytes16*>(B + q);
        else {
#pragma unroll
          for (int w = 0; w < 4; ++w) v[k].w[w] = 0;
          for (int j = 0; j < 16 && q + j < width; ++j) v[k].w[j >> 2] |= (uint32_t)B[q + j] << (8 * (j & 3));
        }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int q = q0 + k * 16 * kTestThreads;
#pragma unroll
        for (int j = 0; j < 16; ++j) if (q + j < width) atomicAdd(&s_hist[((v[k].w[j >> 2] >> (8 * (j & 3))) & 0xffu) * kCols + col], 1u);
      }
    }
    __syncthreads();
    if (threadIdx.x < 256) {
      unsigned n = 0;   // row threadIdx.x, read from the thread's own column on: the lanes of a load stay on different banks
#pragma unroll 8
      for (unsigned j = 0; j < kCols; ++j) n += s_hist[threadIdx.x * kCols + ((j + threadIdx.x) & (kCols - 1))];
      s_hist[kFold + threadIdx.x] = n;
      const long long c = n;
      if (c) { lo = (int)threadIdx.x; hi = (int)threadIdx.x; s1 = c * (long long)threadIdx.x; s2 = c * (long long)threadIdx.x * (long long)threadIdx.x; }
    }
    lo = block_reduce(lo, [](int a, int b2) { return a < b2 ? a : b2; }, s_i2);
    hi = block_reduce(hi, [](int a, int b2) { return a > b2 ? a : b2; }, s_i2);
    s1 = block_reduce(s1, [](long long a, long long b2) { return a + b2; }, s_l);
    s2 = block_reduce(s2, [](long long a, long long b2) { return a + b2; }, s_l);
    double q0 = lo, q1 = (double)s1 / (double)width, q2 = hi;
    unsigned flags = 0;
    if ((double)hi - (double)lo >= 1.0) {
      const unsigned nbk = (unsigned)(hi - lo) + 2;
      int qb[3];
      hist_ranks(s_hist + kFold + lo, nbk, (size_t)width, s_scan, s_q, qb);
      if (qb[0] >= 0) q0 = (double)lo + qb[0] * 1.0;
      if (qb[1] >= 0) q1 = (double)lo + qb[1] * 1.0;
      if (qb[2] >= 0) q2 = (double)lo + qb[2] * 1.0;
    }
    if (threadIdx.x == 0) {
      M.body_flags = flags; M.body_min = lo; M.body_max = hi; M.body_s1 = (double)s1; M.body_s2 = (double)s2;
      M.body_q[0] = q0; M.body_q[1] = q1; M.body_q[2] = q2;
    }
    return;
  }
  // eight independent loads per thread and round: one after the other, each waiting for memory, the 200 000 values of a large
  // candidate took 120 us through this one workgroup
  for (int q0 = threadIdx.x; q0 < width; q0 += 8 * kTestThreads) {
    int x[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) { const int q = q0 + k * kTestThreads; x[k] = body_at(q < width ? q : q0); }
#pragma unroll
    for (int k = 0; k < 8; ++k) if (q0 + k * kTestThreads < width) { lo = x[k] < lo ? x[k] : lo; hi = x[k] > hi ? x[k] : hi; s1 += x[k]; s2 += (long long)x[k] * x[k]; }
  }
  lo = block_reduce(lo, [](int a, int b2) { return a < b2 ? a : b2; }, s_i2);
  hi = block_reduce(hi, [](int a, int b2) { return a > b2 ? a : b2; }, s_i2);
  s1 = block_reduce(s1, [](long long a, long long b2) { return a + b2; }, s_l);
  s2 = block_reduce(s2, [](long long a, long long b2) { return a + b2; }, s_l);
  double q0 = lo, q1 = (double)s1 / (double)width, q2 = hi;
  unsigned flags = 0;
  if ((double)hi - (double)lo >= 1.0) {
    const unsigned nbk = (unsigned)(hi - lo) + 2;
    if (nbk > kCandHistBins) flags = 2;
    else {
      for (unsigned e = threadIdx.x; e < nbk; e += kTestThreads) s_hist[e] = 0;
      __syncthreads();
      for (int q0 = threadIdx.x; q0 < width; q0 += 8 * kTestThreads) {
        int x[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) { const int q = q0 + k * kTestThreads; x[k] = body_at(q < width ? q : q0); }
#pragma unroll
        for (int k = 0; k < 8; ++k) if (q0 + k * kTestThreads < width) atomicAdd(&s_hist[x[k] - lo], 1u);
      }
      __syncthreads();
      int qb[3];
      hist_ranks(s_hist, nbk, (size_t)width, s_scan, s_q, qb);
      if (qb[0] >= 0) q0 = (double)lo + qb[0] * 1.0;
      if (qb[1] >= 0) q1 = (double)lo + qb[1] * 1.0;
      if (qb[2] >= 0) q2 = (double)lo + qb[2] * 1.0;
    }
  }
  if (threadIdx.x == 0) {
    M.body_flags = flags; M.body_min = lo; M.body_max = hi; M.body_s1 = (double)s1; M.body_s2 = (double)s2;
    M.body_q[0] = q0; M.body_q[1] = q1; M.body_q[2] = q2;
  }
}

// launch 3: grid (kCandChunks, njobs) -- 0.01-grid histogram of the means; the last workgroup of a job walks it and
// writes the result.  ghist and the ticket are left zero.
__global__ __launch_bounds__(kTestThreads) void k_cand_hist(const CandJob* __restrict__ jobs, int32_t* __restrict__ iscratch,
                                                        long long* __restrict__ lscratch, CandMid* __restrict__ mid,
                                                        uint32_t* __restrict__ ghist_all, CandOut* __restrict__ outs,
                                                        int vb /* bytes per stored neighbourhood value: where `ref` lies */) {
  extern __shared__ unsigned int s_hist[];   // kCandHistBins counters
  __shared__ int s_scan[kMaxWaves];
  __shared__ int s_q[3];
  __shared__ int s_last;
  const CandJob J = jobs[blockIdx.y];
  CandMid& M = mid[blockIdx.y];
  const CandGeom g = cand_geometry(J, M);
  const CandBufs b = cand_buffers(J, iscratch, lscratch, vb);
  uint32_t* ghist = ghist_all + (size_t)blockIdx.y * kCandHistBins;
  CandOut O;
  O.flags = M.body_flags;
  if (((J.cut & 1) && M.lused >= J.nleft) || ((J.cut & 2) && M.rused >= J.nright)) O.flags |= 8;
  if ((J.cut & 4) && J.top >= 0 && M.lcnt < J.top + 1) O.flags |= 16;   // the left walk ran short after all: the right one gathered too little
  O.nref = g.nref; O.nbody = g.nbody_eff; O.nwin = g.nwin; O.left_reach = M.lreach; O.right_reach = M.rreach;
  if (g.nwin <= 0 || g.width <= 0) {
    O.flags = (O.flags & 24) | 1;
    O.body_min = O.body_max = 0; O.body_s1 = O.body_s2 = O.ref_s1 = O.ref_s2 = 0;
    for (int k = 0; k < 3; ++k) { O.body_q[k] = 0; O.ref_q[k] = 0; }
    if (blockIdx.x == 0 && threadIdx.x == 0) outs[blockIdx.y] = O;
    return;
  }
  O.body_min = M.body_min; O.body_max = M.body_max; O.body_s1 = M.body_s1; O.body_s2 = M.body_s2;
  O.body_q[0] = M.body_q[0]; O.body_q[1] = M.body_q[1]; O.body_q[2] = M.body_q[2];
  float flo = 3.0e38f, fhi = -3.0e38f; double m1 = 0, m2 = 0;
  for (int c = 0; c < kCandChunks; ++c) {   // chunks without windows left their neutral elements
    flo = M.flo[c] < flo ? M.flo[c] : flo; fhi = M.fhi[c] > fhi ? M.fhi[c] : fhi; m1 += M.m1[c]; m2 += M.m2[c];
  }
  const double lo = flo, hi = fhi;
  O.ref_s1 = m1; O.ref_s2 = m2;
  O.ref_q[0] = lo; O.ref_q[1] = m1 / (double)g.nwin; O.ref_q[2] = hi;
  const bool spread = (hi - lo) >= 0.01;
  const size_t nbk = spread ? (size_t)((hi - lo) / 0.01 + 2) : 0;
  if (!spread || nbk > kCandHistBins) {
    if (spread) O.flags |= 4;
    if (blockIdx.x == 0 && threadIdx.x == 0) outs[blockIdx.y] = O;
    return;
  }
  const float* Wm = reinterpret_cast<const float*>(b.ref);
  for (unsigned e = threadIdx.x; e < nbk; e += kTestThreads) s_hist[e] = 0;
  __syncthreads();
  const int Wc = cand_chunk_len(g.nwin);
  const int wb = blockIdx.x * Wc;
  int we = wb + Wc; if (we > g.nwin) we = g.nwin;
  // neighbouring windows mostly share a bucket: eight consecutive means per thread, equal buckets merged before the atomic
  for (int i0 = wb + 8 * (int)threadIdx.x; i0 < we; i0 += 8 * kTestThreads) {
    unsigned pend_b = 0xffffffffu, pend_c = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      if (i0 + k < we) {
        const double idx = ((double)Wm[i0 + k] - lo) / 0.01 + 0.5;   // wufunctions.cpp:396
        const unsigned bkt = (unsigned)(unsigned long long)idx;
        if (bkt != pend_b) { if (pend_c) atomicAdd(&s_hist[pend_b], pend_c); pend_b = bkt; pend_c = 0; }
        ++pend_c;
      }
    }
    if (pend_c) atomicAdd(&s_hist[pend_b], pend_c);
  }
  __syncthreads();
  for (unsigned e = threadIdx.x; e < nbk; e += kTestThreads) { const unsigned c = s_hist[e]; if (c) atomicAdd(&ghist[e], c); }
  sync_drained();   // this workgroup's atomics have completed (no fence: device_util.h)
  if (threadIdx.x == 0) s_last = atomicAdd(&M.done, 1u) == kCandChunks - 1;
  __syncthreads();
  if (!s_last) return;
  for (unsigned e = threadIdx.x; e < nbk; e += kTestThreads) s_hist[e] = ld_cg(&ghist[e]);   // the folded histogram, read past the caches
  __syncthreads();
  int qb[3];
  hist_ranks(s_hist, (unsigned)nbk, (size_t)g.nwin, s_scan, s_q, qb);
  if (qb[0] >= 0) O.ref_q[0] = lo + qb[0] * 0.01;
  if (qb[1] >= 0) O.ref_q[1] = lo + qb[1] * 0.01;
  if (qb[2] >= 0) O.ref_q[2] = lo + qb[2] * 0.01;
  for (unsigned e = threadIdx.x; e < nbk; e += kTestThreads) ghist[e] = 0;
  if (threadIdx.x == 0) { M.done = 0; outs[blockIdx.y] = O; }
}

// Sums of depth over inclusive ranges (mean_tp of mergesegments, rsi.cpp:775-779): exact integers.
template <typename TD>
__global__ __launch_bounds__(kThreads) void k_range_sums(const TD* __restrict__ A, const int2* __restrict__ ranges,
                                                         long long* __restrict__ sums) {
  __shared__ long long s_l[kThreads / 64 + 1];
  const int2 r = ranges[blockIdx.x];
  long long acc = 0;
  for (int p = r.x + (int)threadIdx.x; p <= r.y; p += kThreads) acc += A[p];
  acc = block_reduce(acc, [](long long a, long long b) { return a + b; }, s_l);
  if (threadIdx.x == 0) sums[blockIdx.x] = acc;
}

}  // namespace

// The capped, compacted depth is an int32 array or, behind K4', a byte array (DepthRef): every kernel exists for both.
#define RSI_DEPTH_DISPATCH(D, CALL32, CALL8) do { if ((D).bytes == 1) { const uint8_t* rdc = static_cast<const uint8_t*>((D).p); CALL8; } \
                                                 else { const int32_t* rdc = static_cast<const int32_t*>((D).p); CALL32; } } while (0)

void launch_range_sums(DepthRef d, const void* ranges, int nranges, long long* sums, hipStream_t stream) {
  if (nranges <= 0) return;
  RSI_DEPTH_DISPATCH(d,
    RSI_LAUNCH(k_range_sums<int32_t>, dim3(nranges), dim3(kThreads), 0, stream, rdc, static_cast<const int2*>(ranges), sums),
    RSI_LAUNCH(k_range_sums<uint8_t>, dim3(nranges), dim3(kThreads), 0, stream, rdc, static_cast<const int2*>(ranges), sums));
}

void launch_sharpen_edges(DepthRef d, int64_t ncompact, EdgeJob* jobs, int njobs, void* ws, int ws_jobs, hipStream_t stream) {
  if (njobs <= 0) return;
  RSI_DEPTH_DISPATCH(d,
    RSI_LAUNCH(k_sharpen_edges<int32_t>, dim3(2 * kEdgeChunks, njobs), dim3(kThreads), 0, stream, rdc, ncompact, jobs, ws_jobs, ws),
    RSI_LAUNCH(k_sharpen_edges<uint8_t>, dim3(2 * kEdgeChunks, njobs), dim3(kThreads), 0, stream, rdc, ncompact, jobs, ws_jobs, ws));
}
namespace {
template <typename TD, typename TS>
void cand_launch_split(const TD* rdc, int64_t ncompact, const CandJob* jobs, int njobs, const int2* ch, int32_t* iscratch,
                       double RDmedian, CandMid* mid, uint32_t* ghist, CandOut* outs, hipStream_t stream) {
  const size_t lds = (size_t)kCandHistBins * 4;
  RSI_ALLOW_FULL_LDS((k_cand_gather<TD, TS>));
  RSI_ALLOW_FULL_LDS((k_cand_sums<TD, TS>));
  RSI_ALLOW_FULL_LDS(k_cand_hist);
  const int vb = (int)sizeof(TS);
  long long* const lscratch = nullptr;   // no int64 scratch in this form
  RSI_LAUNCH((k_cand_gather<TD, TS>), dim3(2, njobs), dim3(kTestThreads), lds, stream, rdc, ncompact, jobs, ch, iscratch, lscratch, RDmedian, mid);
  RSI_LAUNCH((k_cand_sums<TD, TS>), dim3(kCandChunks + 1, njobs), dim3(kTestThreads), lds, stream, rdc, jobs, iscratch, mid);
  RSI_LAUNCH(k_cand_hist, dim3(kCandChunks, njobs), dim3(kTestThreads), lds, stream, jobs, iscratch, lscratch, mid, ghist, outs, vb);
}
template <typename TD, typename TS>
void cand_launch_one_wg(const TD* rdc, int64_t ncompact, const CandJob* jobs, int njobs, const int2* ch, int32_t* iscratch,
                        long long* lscratch, double RDmedian, CandOut* outs, hipStream_t stream) {
  const size_t lds = (size_t)kCandHistBins * 4;
  RSI_ALLOW_FULL_LDS((k_candidate_test<TD, TS>));
  RSI_LAUNCH((k_candidate_test<TD, TS>), dim3(njobs), dim3(kTestThreads), lds, stream, rdc, ncompact, jobs, ch, iscratch, lscratch, RDmedian, outs);
}
}  // namespace
// value_bytes: how the gathered values are stored, 1 (byte depth only) or 4; the caller sizes iscratch accordingly
void launch_candidate_test_split(DepthRef d, int64_t ncompact, const CandJob* jobs, int njobs, const void* chains,
                                 int32_t* iscratch, double RDmedian, CandMid* mid, uint32_t* ghist,
                                 CandOut* outs, int value_bytes, hipStream_t stream) {
  if (njobs <= 0) return;
  const int2* ch = static_cast<const int2*>(chains);
  if (d.bytes == 1 && value_bytes == 1)
    cand_launch_split<uint8_t, uint8_t>(static_cast<const uint8_t*>(d.p), ncompact, jobs, njobs, ch, iscratch, RDmedian, mid, ghist, outs, stream);
  else if (d.bytes == 1)
    cand_launch_split<uint8_t, int32_t>(static_cast<const uint8_t*>(d.p), ncompact, jobs, njobs, ch, iscratch, RDmedian, mid, ghist, outs, stream);
  else
    cand_launch_split<int32_t, int32_t>(static_cast<const int32_t*>(d.p), ncompact, jobs, njobs, ch, iscratch, RDmedian, mid, ghist, outs, stream);
}
size_t sharpen_workspace_bytes(int njobs) { return sharpen_zero_bytes(njobs) + (size_t)njobs * 2 * kEdgeChunks * (8 + 8 + 4); }
size_t sharpen_workspace_zero_bytes(int njobs) { return sharpen_zero_bytes(njobs); }
void launch_candidate_test(DepthRef d, int64_t ncompact, const CandJob* jobs, int njobs, const void* chains,
                           int32_t* iscratch, long long* lscratch, double RDmedian, CandOut* outs, int value_bytes, hipStream_t stream) {
  if (njobs <= 0) return;
  const int2* ch = static_cast<const int2*>(chains);
  if (d.bytes == 1 && value_bytes == 1)
    cand_launch_one_wg<uint8_t, uint8_t>(static_cast<const uint8_t*>(d.p), ncompact, jobs, njobs, ch, iscratch, lscratch, RDmedian, outs, stream);
  else if (d.bytes == 1)
    cand_launch_one_wg<uint8_t, int32_t>(static_cast<const uint8_t*>(d.p), ncompact, jobs, njobs, ch, iscratch, lscratch, RDmedian, outs, stream);
  else
    cand_launch_one_wg<int32_t, int32_t>(static_cast<const int32_t*>(d.p), ncompact, jobs, njobs, ch, iscratch, lscratch, RDmedian, outs, stream);
}
#undef RSI_DEPTH_DISPATCH

// The int32 form of a byte array (rsi_hot_fetch("rd_concat"), the host's page fetches): 16 values per thread.
__global__ __launch_bounds__(256) void k_widen_u8(const uint8_t* __restrict__ src, int64_t n, int32_t* __restrict__ dst) {
  const int64_t i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 16;
  if (i0 + 16 <= n) {
    const uint4 b = *reinterpret_cast<const uint4*>(src + i0);
    const uint32_t w[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
    for (int q = 0; q < 4; ++q)
      *reinterpret_cast<int4*>(dst + i0 + 4 * q) = make_int4((int)(w[q] & 0xffu), (int)((w[q] >> 8) & 0xffu), (int)((w[q] >> 16) & 0xffu), (int)(w[q] >> 24));
  } else {
    for (int64_t i = i0; i < n; ++i) dst[i] = (int)src[i];
  }
}
void launch_widen_u8(const uint8_t* src, int64_t n, int32_t* dst, hipStream_t stream) {
  if (n <= 0) return;
  const int64_t blocks = (n + 256 * 16 - 1) / (256 * 16);
  RSI_LAUNCH(k_widen_u8, dim3((unsigned int)blocks), dim3(256), 0, stream, src, n, dst);
}

// dst[pos[k]] = val[k]: the depths that did not fit a byte, behind launch_widen_u8 (rsi_hot_run's narrowed upload)
__global__ __launch_bounds__(256) void k_patch_i32(int32_t* __restrict__ dst, const int32_t* __restrict__ pos, const int32_t* __restrict__ val, int64_t cnt) {
  for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < cnt; k += (int64_t)gridDim.x * 256) dst[pos[k]] = val[k];
}
void launch_patch_i32(int32_t* dst, const int32_t* pos, const int32_t* val, int64_t cnt, hipStream_t stream) {
  if (cnt <= 0) return;
  const int64_t blocks = std::min<int64_t>((cnt + 255) / 256, 1024);
  RSI_LAUNCH(k_patch_i32, dim3((unsigned int)blocks), dim3(256), 0, stream, dst, pos, val, cnt);
}

}  // namespace rsik
