// kernels_track.hip -- an int32 array in HBM as bedGraph text (bedtools genomecov -bga: one line per maximal run of equal
// values, zeros included), run-length encoded and formatted on the device so that only finished text crosses PCIe.  The mirror
// image of the bedGraph reader's expansion (kernels_io.hip); the passes and the slice rule: DESIGN.md 6f.
// All of it is integer work: digits come from comparisons and divisions by ten, nothing is printed through printf.
#include "kernels.h"

namespace rsik {
namespace {

static_assert(kTrackTile == 256, "the kernels below are written for four waves of 64 lanes");

// Exclusive prefix of v over the workgroup's 256 threads; *total: the workgroup's sum (in every thread).  s_w: four words of LDS.
__device__ inline unsigned int wg_exscan_u32(unsigned int v, unsigned int* s_w, unsigned int* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned int incl = (unsigned int)wave_incl_scan((int)v);
  __syncthreads();   // the previous call's readers are through with s_w
  if (lane == 63) s_w[wave] = incl;
  __syncthreads();
  unsigned int base = 0, tot = 0;
  for (int w = 0; w < kTrackTile / 64; ++w) { const unsigned int s = s_w[w]; if (w < wave) base += s; tot += s; }
  *total = tot;
  return base + incl - v;
}

__device__ inline bool run_start(const int32_t* __restrict__ v, long long i) { return i == 0 || v[i] != v[i - 1]; }

// ---- pass 1: run starts per tile of 256 bases ----
__global__ __launch_bounds__(kTrackTile) void k_track_count(const int32_t* __restrict__ v, long long b, long long e,
                                                            unsigned int* __restrict__ tiles) {
  __shared__ unsigned int s_w[kTrackTile / 64];
  const long long i = b + (long long)blockIdx.x * kTrackTile + threadIdx.x;
  const unsigned int flag = i < e && run_start(v, i) ? 1u : 0u;
  unsigned int total;
  (void)wg_exscan_u32(flag, s_w, &total);
  if (threadIdx.x == 0) tiles[blockIdx.x] = total;
}

// Exclusive scan of t[0, nt) in place by one workgroup, the first entry becoming `base`; returns base + the sum (every thread).
__device__ inline unsigned long long scan_tile_words(unsigned int* __restrict__ t, int nt, unsigned int base, unsigned int* s_w) {
  unsigned long long run = base;
  for (int t0 = 0; t0 < nt; t0 += kTrackTile) {
    const int k = t0 + (int)threadIdx.x;
    const unsigned int x = k < nt ? t[k] : 0u;
    unsigned int total;
    const unsigned int ex = wg_exscan_u32(x, s_w, &total);
    if (k < nt) t[k] = (unsigned int)run + ex;
    run += total;
  }
  return run;
}

// ---- pass 2: the tile counts become offsets into starts[]; the carried start in front, the closing n behind the last slice's ----
__global__ __launch_bounds__(kTrackTile) void k_track_scan_starts(unsigned int* __restrict__ tiles, int ntiles, long long* __restrict__ starts,
                                                                  TrackState* __restrict__ st, long long e, long long n) {
  __shared__ unsigned int s_w[kTrackTile / 64];
  const long long carry = st->carry;
  const unsigned long long m = scan_tile_words(tiles, ntiles, carry >= 0 ? 1u : 0u, s_w);
  if (threadIdx.x == 0) {
    if (carry >= 0) starts[0] = carry;
    const bool last = e == n;
    if (last) starts[m] = n;
    st->nstarts = (long long)m;
    st->nlines = last ? (long long)m : (m > 0 ? (long long)m - 1 : 0);   // the last start stays open until a later slice ends its run
  }
}

// ---- pass 3: the starts of [b, e) into starts[], in order ----
__global__ __launch_bounds__(kTrackTile) void k_track_scatter(const int32_t* __restrict__ v, long long b, long long e,
                                                              const unsigned int* __restrict__ tiles, long long* __restrict__ starts) {
  __shared__ unsigned int s_w[kTrackTile / 64];
  const long long i = b + (long long)blockIdx.x * kTrackTile + threadIdx.x;
  const unsigned int flag = i < e && run_start(v, i) ? 1u : 0u;
  unsigned int total;
  const unsigned int rank = wg_exscan_u32(flag, s_w, &total);
  if (flag) starts[(unsigned long long)tiles[blockIdx.x] + rank] = i;
}

// ---- decimal digits without division where a count is enough ----
__device__ inline int dec_len_u32(unsigned int x) {
  return x < 10u ? 1 : x < 100u ? 2 : x < 1000u ? 3 : x < 10000u ? 4 : x < 100000u ? 5 : x < 1000000u ? 6 : x < 10000000u ? 7
       : x < 100000000u ? 8 : x < 1000000000u ? 9 : 10;
}
__device__ inline int dec_len_u64(unsigned long long x) {
  if (x <= 0xffffffffull) return dec_len_u32((unsigned int)x);
  int d = 10;
  unsigned long long p = 10000000000ull;   // 10^10: the smallest number of 11 digits
  while (x >= p) { ++d; if (d == 20) break; p *= 10ull; }   // 10^19 is the last power of ten below 2^64
  return d;
}
__device__ inline int dec_len_i64(long long x) { return x < 0 ? 1 + dec_len_u64(0ull - (unsigned long long)x) : dec_len_u64((unsigned long long)x); }
__device__ inline int dec_len_i32(int x) { return x < 0 ? 1 + dec_len_u32(0u - (unsigned int)x) : dec_len_u32((unsigned int)x); }   // INT32_MIN: 11
// x as `len` = its digit count characters at p, last digit first; the 64-bit divisions end once the rest fits 32 bits
__device__ inline void put_dec(char* __restrict__ p, int len, unsigned long long x) {
  while (x > 0xffffffffull) { p[--len] = (char)('0' + (int)(x % 10ull)); x /= 10ull; }
  unsigned int y = (unsigned int)x;
  do { p[--len] = (char)('0' + (int)(y % 10u)); y /= 10u; } while (len > 0);
}
__device__ inline char* put_i64(char* __restrict__ p, long long x, int len) {
  if (x < 0) { p[0] = '-'; put_dec(p + 1, len - 1, 0ull - (unsigned long long)x); }
  else put_dec(p, len, (unsigned long long)x);
  return p + len;
}

// Where the lines come from.  The length, scan and format passes see (start, end, value) triples only: another source of
// triples (a per-bin signal, say) takes the same passes with a struct of its own.
struct RunLines {
  const int32_t* __restrict__ v;
  const long long* __restrict__ starts;
  __device__ void get(long long j, long long& s, long long& e, int& val) const { s = starts[j]; e = starts[j + 1]; val = v[s]; }
};
struct LineShape { long long s, e; int val, ls, le, lv; unsigned long long q; };

// How a line's value is written, chosen at compile time: its length for line_shape, its digits for the format pass.
struct DecValue {   // %d
  __device__ int len(int val, unsigned long long& q) const { q = 0; return dec_len_i32(val); }
  __device__ char* put(char* __restrict__ p, int val, unsigned long long, int lv) const { return put_i64(p, (long long)val, lv); }
};
// val over half of m2, three decimals, rounded half up: q = (4000 val + m2) / (2 m2) thousandths, in integers (val >= 0, m2 > 0)
struct RatioValue {
  long long m2;
  __device__ int len(int val, unsigned long long& q) const {
    q = val < 0 ? 0ull : (4000ull * (unsigned long long)val + (unsigned long long)m2) / (2ull * (unsigned long long)m2);
    return dec_len_u64(q / 1000ull) + 4;   // the point and three places
  }
  __device__ char* put(char* __restrict__ p, int, unsigned long long q, int lv) const {
    put_dec(p, lv - 4, q / 1000ull);
    unsigned int f = (unsigned int)(q % 1000ull);
    p[lv - 4] = '.';
    p[lv - 1] = (char)('0' + (int)(f % 10u)); f /= 10u;
    p[lv - 2] = (char)('0' + (int)(f % 10u)); f /= 10u;
    p[lv - 3] = (char)('0' + (int)f);
    return p + lv;
  }
};

template <class Lines, class Value>
__device__ inline int line_shape(const Lines& src, const Value& fmt, long long j, long long pos0, int name_len, LineShape& L) {
  src.get(j, L.s, L.e, L.val);
  L.s += pos0; L.e += pos0;
  L.ls = dec_len_i64(L.s); L.le = dec_len_i64(L.e); L.lv = fmt.len(L.val, L.q);
  return name_len + 4 + L.ls + L.le + L.lv;   // three tabs and the newline
}

// ---- pass 4: bytes per tile of 256 lines ----
template <class Lines, class Value>
__global__ __launch_bounds__(kTrackTile) void k_track_line_bytes(Lines src, Value fmt, const TrackState* __restrict__ st, long long pos0, int name_len,
                                                                 unsigned int* __restrict__ ltiles) {
  __shared__ unsigned int s_w[kTrackTile / 64];
  const long long nlines = st->nlines;
  if ((long long)blockIdx.x * kTrackTile >= nlines) return;   // the grid covers the most lines a slice can have
  const long long j = (long long)blockIdx.x * kTrackTile + threadIdx.x;
  LineShape L;
  const unsigned int len = j < nlines ? (unsigned int)line_shape(src, fmt, j, pos0, name_len, L) : 0u;
  unsigned int total;
  (void)wg_exscan_u32(len, s_w, &total);
  if (threadIdx.x == 0) ltiles[blockIdx.x] = total;
}

// ... scanned: every tile's byte offset, the slice's bytes, and the run left open for the next slice
__global__ __launch_bounds__(kTrackTile) void k_track_scan_lines(unsigned int* __restrict__ ltiles, const long long* __restrict__ starts,
                                                                 TrackState* __restrict__ st) {
  __shared__ unsigned int s_w[kTrackTile / 64];
  const unsigned long long bytes = scan_tile_words(ltiles, track_tiles(st->nlines), 0u, s_w);
  if (threadIdx.x == 0) {
    st->nbytes = (long long)bytes;
    if (st->nstarts > 0) st->carry = starts[st->nstarts - 1];
  }
}

// ---- pass 5: one thread per line ----
template <class Lines, class Value>
__global__ __launch_bounds__(kTrackTile) void k_track_format(Lines src, Value fmt, const unsigned int* __restrict__ ltiles, long long nlines, long long pos0,
                                                             const TrackName name, char* __restrict__ text, long long cap) {
  __shared__ unsigned int s_w[kTrackTile / 64];
  const long long j = (long long)blockIdx.x * kTrackTile + threadIdx.x;
  LineShape L;
  const unsigned int len = j < nlines ? (unsigned int)line_shape(src, fmt, j, pos0, name.len, L) : 0u;
  unsigned int total;
  const unsigned long long off = (unsigned long long)ltiles[blockIdx.x] + wg_exscan_u32(len, s_w, &total);
  if (len == 0u || (long long)(off + len) > cap) return;
  char* p = text + off;
  for (int k = 0; k < name.len; ++k) p[k] = name.s[k];
  p += name.len;
  *p++ = '\t';
  p = put_i64(p, L.s, L.ls);
  *p++ = '\t';
  p = put_i64(p, L.e, L.le);
  *p++ = '\t';
  p = fmt.put(p, L.val, L.q, L.lv);
  *p = '\n';
}

// ---- per-bin lines: one line per piece of a bin, a piece being a maximal stretch of consecutive reference positions ----
// Bin b covers the compacted positions [b m, (b + 1) m); a compacted position p lies at p + cum[k], k = #{cbreak <= p}
// (rsih::compact_table).  A bin is cut at every break strictly inside it, so it has 1 + #{b m < cbreak < (b + 1) m} pieces; a
// break at b m belongs to the gap in front.  The table comes from HBM, at most 4096 entries: twelve steps per search.
struct BinTable { const long long* __restrict__ cbreak; const long long* __restrict__ cum; int nreg; int m; };
__device__ inline int breaks_le(const BinTable& t, long long p) {   // #{cbreak <= p}
  int lo = 0, hi = t.nreg;
  while (lo < hi) { const int mid = (lo + hi) >> 1; if (t.cbreak[mid] <= p) lo = mid + 1; else hi = mid; }
  return lo;
}
__device__ inline int breaks_lt(const BinTable& t, long long p) {   // #{cbreak < p}
  int lo = 0, hi = t.nreg;
  while (lo < hi) { const int mid = (lo + hi) >> 1; if (t.cbreak[mid] < p) lo = mid + 1; else hi = mid; }
  return lo;
}
// pieces of bin b and the region index of its first one (= the breaks at or in front of its first position)
__device__ inline unsigned int bin_pieces(const BinTable& t, long long b, int& k0) {
  const long long lo = b * t.m;
  k0 = breaks_le(t, lo);
  return 1u + (unsigned int)(breaks_lt(t, lo + t.m) - k0);
}

// A piece is stored as (bin - b0) << 16 | region index: eight bytes where the triple takes twenty, and the accessor needs no
// search to get the triple back -- the piece of bin b with k breaks in front runs from max(b m, cbreak[k - 1]) to
// min((b + 1) m, cbreak[k]) in compacted positions, shifted by cum[k].
constexpr int kPieceRegionBits = 16;
static_assert((1 << kPieceRegionBits) > 4096, "a region index fits the low bits of a piece");

// pass 1: pieces per tile of 256 bins
__global__ __launch_bounds__(kTrackTile) void k_bintrack_count(BinTable t, long long b0, long long b1, unsigned int* __restrict__ tiles) {
  __shared__ unsigned int s_w[kTrackTile / 64];
  const long long b = b0 + (long long)blockIdx.x * kTrackTile + threadIdx.x;
  int k0;
  const unsigned int cnt = b < b1 ? bin_pieces(t, b, k0) : 0u;
  unsigned int total;
  (void)wg_exscan_u32(cnt, s_w, &total);
  if (threadIdx.x == 0) tiles[blockIdx.x] = total;
}

// pass 2: the tile counts become offsets into pieces[]; nothing is carried from slice to slice
__global__ __launch_bounds__(kTrackTile) void k_bintrack_scan(unsigned int* __restrict__ tiles, int ntiles, TrackState* __restrict__ st) {
  __shared__ unsigned int s_w[kTrackTile / 64];
  const unsigned long long total = scan_tile_words(tiles, ntiles, 0u, s_w);
  if (threadIdx.x == 0) { st->carry = -1; st->nstarts = 0; st->nlines = (long long)total; st->nbytes = 0; }
}

// pass 3: every bin writes its pieces, in order, at its offset; the loop is as long as the breaks inside the bin (at most the table)
__global__ __launch_bounds__(kTrackTile) void k_bintrack_scatter(BinTable t, long long b0, long long b1, const unsigned int* __restrict__ tiles,
                                                                 unsigned long long* __restrict__ pieces, long long cap) {
  __shared__ unsigned int s_w[kTrackTile / 64];
  const long long b = b0 + (long long)blockIdx.x * kTrackTile + threadIdx.x;
  int k0 = 0;
  const unsigned int cnt = b < b1 ? bin_pieces(t, b, k0) : 0u;
  unsigned int total;
  const unsigned long long off = (unsigned long long)tiles[blockIdx.x] + wg_exscan_u32(cnt, s_w, &total);
  const unsigned long long word = (unsigned long long)(b - b0) << kPieceRegionBits;
  for (unsigned int i = 0; i < cnt; ++i)
    if ((long long)(off + i) < cap) pieces[off + i] = word | (unsigned int)(k0 + (int)i);
}

struct BinLines {
  const int32_t* __restrict__ v;   // the bins' values, v[0] = bin 0 of the chromosome
  const unsigned long long* __restrict__ pieces;
  BinTable t;
  long long b0;
  __device__ void get(long long j, long long& s, long long& e, int& val) const {
    const unsigned long long w = pieces[j];
    const int k = (int)(w & ((1u << kPieceRegionBits) - 1u));
    const long long b = b0 + (long long)(w >> kPieceRegionBits);
    const long long lo = b * t.m, hi = lo + t.m;
    s = lo; e = hi;
    if (k > 0) { const long long c = t.cbreak[k - 1]; if (c > s) s = c; }
    if (k < t.nreg) { const long long c = t.cbreak[k]; if (c < e) e = c; }
    const long long shift = t.cum[k];
    s += shift; e += shift;
    val = v[b];
  }
};

// ---- region lines (`rsicnv depth -by`): a line per (start, end, sum) triple, its value the mean ----
// The passes hand a line's `val` from the source to the value format; here it is the line's index in the slice, and the format
// reads the triple behind it: a mean needs 64 bits of sum and a length, which no int holds.
struct RegionLines {
  const long long* __restrict__ start;
  const long long* __restrict__ end;
  __device__ void get(long long j, long long& s, long long& e, int& val) const { s = start[j]; e = end[j]; val = (int)j; }
};
// sum / (end - start), two decimals, rounded half up: q = 100 a + h hundredths with a = S / L, r = S mod L, h = (200 r + L) / (2 L)
// (h = 100 is the carry into a); 0.00 for an empty line or a sum that is not positive.  200 r stays below 2^63 for L < 2^55, and
// 100 a in 64 bits because a, a mean of int32 depths, is below 2^31.
struct MeanValue {
  const long long* __restrict__ start;
  const long long* __restrict__ end;
  const long long* __restrict__ sum;
  __device__ int len(int j, unsigned long long& q) const {
    const long long L = end[j] - start[j], S = sum[j];
    q = 0ull;
    if (L > 0 && S > 0) {
      const unsigned long long l = (unsigned long long)L, a = (unsigned long long)S / l, r = (unsigned long long)S % l;
      q = 100ull * a + (200ull * r + l) / (2ull * l);
    }
    return dec_len_u64(q / 100ull) + 3;   // the point and two places
  }
  __device__ char* put(char* __restrict__ p, int, unsigned long long q, int lv) const {
    put_dec(p, lv - 3, q / 100ull);
    const unsigned int f = (unsigned int)(q % 100ull);
    p[lv - 3] = '.';
    p[lv - 2] = (char)('0' + (int)(f / 10u));
    p[lv - 1] = (char)('0' + (int)(f % 10u));
    return p + lv;
  }
};

__global__ void k_regiontrack_begin(TrackState* __restrict__ st, long long nlines) {
  st->carry = -1; st->nstarts = 0; st->nlines = nlines; st->nbytes = 0;
}

// ---- the index pass: one thread per line, as the format pass (kernels.h states the records) ----
// tabix's reg2bin of [s, e1], e1 the line's last base: the first level at which both fall into one bin
__device__ inline unsigned int reg2bin(long long s, long long e1) {
  if (s >> 14 == e1 >> 14) return 4681u + (unsigned int)(s >> 14);
  if (s >> 17 == e1 >> 17) return 585u + (unsigned int)(s >> 17);
  if (s >> 20 == e1 >> 20) return 73u + (unsigned int)(s >> 20);
  if (s >> 23 == e1 >> 23) return 9u + (unsigned int)(s >> 23);
  if (s >> 26 == e1 >> 26) return 1u + (unsigned int)(s >> 26);
  return 0u;
}

template <class Lines, class Value>
__global__ __launch_bounds__(kTrackTile) void k_track_index(Lines src, Value fmt, const unsigned int* __restrict__ ltiles, long long nlines, long long pos0,
                                                            int name_len, const unsigned int* __restrict__ sizes, int nmembers, TrackIndexOut out) {
  __shared__ unsigned int s_w[kTrackTile / 64];
  __shared__ unsigned int s_front[kTrackIndexMembers + 1];   // compressed bytes in front of every member of the slice
  __shared__ unsigned int s_base[2];
  if (nmembers > kTrackIndexMembers) {   // (the host plans at most that many: never)
    if (blockIdx.x == 0 && threadIdx.x == 0) out.head->bad = 1u;
    return;
  }
  for (int k = threadIdx.x; k < nmembers; k += kTrackTile) s_front[k] = sizes[k] & 0x7fffffffu;   // bit 31: a stored member
  __syncthreads();
  (void)scan_tile_words(s_front, nmembers, 0u, s_w);
  __syncthreads();

  const long long j = (long long)blockIdx.x * kTrackTile + threadIdx.x;
  const bool live = j < nlines;
  LineShape L;
  const unsigned int len = live ? (unsigned int)line_shape(src, fmt, j, pos0, name_len, L) : 0u;
  unsigned int total;
  const unsigned long long off = (unsigned long long)ltiles[blockIdx.x] + wg_exscan_u32(len, s_w, &total);
  unsigned int cflag = 0u, wflag = 0u, bin = 0u, w_first = 0u, w_last = 0u;
  unsigned long long voff = 0ull;
  if (live) {
    const long long e1 = L.e - 1;
    bin = reg2bin(L.s, e1);
    w_first = (unsigned int)(L.s >> 14);
    w_last = (unsigned int)(e1 >> 14);
    cflag = wflag = 1u;
    if (j > 0) {
      long long ps, pe; int pv;
      src.get(j - 1, ps, pe, pv);
      const long long p1 = pe + pos0 - 1;
      cflag = reg2bin(ps + pos0, p1) != bin ? 1u : 0u;
      wflag = (e1 >> 14) > (p1 >> 14) ? 1u : 0u;
      const unsigned int reached = (unsigned int)(p1 >> 14) + 1u;
      if (reached > w_first) w_first = reached;
    }
    const unsigned int member = (unsigned int)(off / kDeflateMemberText);
    const unsigned int front = member < (unsigned int)nmembers ? s_front[member] : 0u;
    voff = (unsigned long long)front << 16 | (off - (unsigned long long)member * kDeflateMemberText);
  }
  unsigned int ctot, wtot;
  const unsigned int crank = wg_exscan_u32(cflag, s_w, &ctot);
  const unsigned int wrank = wg_exscan_u32(wflag, s_w, &wtot);
  if (threadIdx.x == 0) {
    s_base[0] = ctot ? atomicAdd(&out.head->nchunk, ctot) : 0u;
    s_base[1] = wtot ? atomicAdd(&out.head->nwin, wtot) : 0u;
  }
  __syncthreads();
  if (cflag) {
    const unsigned int k = s_base[0] + crank;
    if (k < out.chunk_cap) out.chunks[k] = TrackIndexRec{voff, bin, 0u};
  }
  if (wflag) {
    const unsigned int k = s_base[1] + wrank;
    if (k < out.win_cap) out.wins[k] = TrackIndexRec{voff, w_first, w_last};
  }
}

}  // namespace

void launch_track_index(const int32_t* v, const long long* starts, const unsigned int* ltiles, long long nlines, long long pos0, int name_len,
                        const unsigned int* sizes, int nmembers, const TrackIndexOut& out, hipStream_t stream) {
  const int ntiles = track_tiles(nlines);
  if (ntiles <= 0) return;
  RSI_LAUNCH((k_track_index<RunLines, DecValue>), dim3(ntiles), dim3(kTrackTile), 0, stream, RunLines{v, starts}, DecValue{}, ltiles, nlines, pos0, name_len,
             sizes, nmembers, out);
}

void launch_bintrack_index(const BinTrackSource& src, const unsigned int* ltiles, long long nlines, int name_len, const unsigned int* sizes,
                           int nmembers, const TrackIndexOut& out, hipStream_t stream) {
  const int ntiles = track_tiles(nlines);
  if (ntiles <= 0) return;
  const BinLines lines{src.v, src.pieces, BinTable{src.cbreak, src.cum, src.nreg, src.m}, src.b0};
  if (src.which == 1)
    RSI_LAUNCH((k_track_index<BinLines, RatioValue>), dim3(ntiles), dim3(kTrackTile), 0, stream, lines, RatioValue{src.median2}, ltiles, nlines, 0ll, name_len,
               sizes, nmembers, out);
  else
    RSI_LAUNCH((k_track_index<BinLines, DecValue>), dim3(ntiles), dim3(kTrackTile), 0, stream, lines, DecValue{}, ltiles, nlines, 0ll, name_len,
               sizes, nmembers, out);
}

void launch_track_starts(const int32_t* v, long long b, long long e, long long n, unsigned int* tiles, long long* starts, TrackState* st,
                         hipStream_t stream) {
  const int ntiles = track_tiles(e - b);
  if (ntiles <= 0) return;
  RSI_LAUNCH(k_track_count, dim3(ntiles), dim3(kTrackTile), 0, stream, v, b, e, tiles);
  RSI_LAUNCH(k_track_scan_starts, dim3(1), dim3(kTrackTile), 0, stream, tiles, ntiles, starts, st, e, n);
  RSI_LAUNCH(k_track_scatter, dim3(ntiles), dim3(kTrackTile), 0, stream, v, b, e, tiles, starts);
}

void launch_track_line_bytes(const int32_t* v, const long long* starts, TrackState* st, long long pos0, int name_len, long long max_lines,
                             unsigned int* ltiles, hipStream_t stream) {
  const int ntiles = track_tiles(max_lines);
  if (ntiles <= 0) return;
  RSI_LAUNCH((k_track_line_bytes<RunLines, DecValue>), dim3(ntiles), dim3(kTrackTile), 0, stream, RunLines{v, starts}, DecValue{}, st, pos0, name_len, ltiles);
  RSI_LAUNCH(k_track_scan_lines, dim3(1), dim3(kTrackTile), 0, stream, ltiles, starts, st);
}

void launch_track_format(const int32_t* v, const long long* starts, const unsigned int* ltiles, long long nlines, long long pos0,
                         const TrackName& name, char* text, long long cap, hipStream_t stream) {
  const int ntiles = track_tiles(nlines);
  if (ntiles <= 0) return;
  RSI_LAUNCH((k_track_format<RunLines, DecValue>), dim3(ntiles), dim3(kTrackTile), 0, stream, RunLines{v, starts}, DecValue{}, ltiles, nlines, pos0, name, text, cap);
}

void launch_bintrack_pieces(const long long* cbreak, const long long* cum, int nreg, int m, long long b0, long long b1, unsigned int* tiles,
                            unsigned long long* pieces, long long cap, TrackState* st, hipStream_t stream) {
  const int ntiles = track_tiles(b1 - b0);
  if (ntiles <= 0) return;
  const BinTable t{cbreak, cum, nreg, m};
  RSI_LAUNCH(k_bintrack_count, dim3(ntiles), dim3(kTrackTile), 0, stream, t, b0, b1, tiles);
  RSI_LAUNCH(k_bintrack_scan, dim3(1), dim3(kTrackTile), 0, stream, tiles, ntiles, st);
  RSI_LAUNCH(k_bintrack_scatter, dim3(ntiles), dim3(kTrackTile), 0, stream, t, b0, b1, tiles, pieces, cap);
}

void launch_bintrack_line_bytes(const BinTrackSource& src, TrackState* st, int name_len, long long max_lines, unsigned int* ltiles,
                                hipStream_t stream) {
  const int ntiles = track_tiles(max_lines);
  if (ntiles <= 0) return;
  const BinLines lines{src.v, src.pieces, BinTable{src.cbreak, src.cum, src.nreg, src.m}, src.b0};
  if (src.which == 1)
    RSI_LAUNCH((k_track_line_bytes<BinLines, RatioValue>), dim3(ntiles), dim3(kTrackTile), 0, stream, lines, RatioValue{src.median2}, st, 0ll, name_len, ltiles);
  else
    RSI_LAUNCH((k_track_line_bytes<BinLines, DecValue>), dim3(ntiles), dim3(kTrackTile), 0, stream, lines, DecValue{}, st, 0ll, name_len, ltiles);
  RSI_LAUNCH(k_track_scan_lines, dim3(1), dim3(kTrackTile), 0, stream, ltiles, static_cast<const long long*>(nullptr), st);
}

void launch_bintrack_format(const BinTrackSource& src, const unsigned int* ltiles, long long nlines, const TrackName& name, char* text,
                            long long cap, hipStream_t stream) {
  const int ntiles = track_tiles(nlines);
  if (ntiles <= 0) return;
  const BinLines lines{src.v, src.pieces, BinTable{src.cbreak, src.cum, src.nreg, src.m}, src.b0};
  if (src.which == 1)
    RSI_LAUNCH((k_track_format<BinLines, RatioValue>), dim3(ntiles), dim3(kTrackTile), 0, stream, lines, RatioValue{src.median2}, ltiles, nlines, 0ll, name, text, cap);
  else
    RSI_LAUNCH((k_track_format<BinLines, DecValue>), dim3(ntiles), dim3(kTrackTile), 0, stream, lines, DecValue{}, ltiles, nlines, 0ll, name, text, cap);
}

void launch_regiontrack_line_bytes(const RegionTrackSource& src, TrackState* st, long long nlines, long long pos0, int name_len,
                                   unsigned int* ltiles, hipStream_t stream) {
  const int ntiles = track_tiles(nlines);
  if (ntiles <= 0) return;
  RSI_LAUNCH(k_regiontrack_begin, dim3(1), dim3(1), 0, stream, st, nlines);
  RSI_LAUNCH((k_track_line_bytes<RegionLines, MeanValue>), dim3(ntiles), dim3(kTrackTile), 0, stream, RegionLines{src.start, src.end},
             MeanValue{src.start, src.end, src.sum}, st, pos0, name_len, ltiles);
  RSI_LAUNCH(k_track_scan_lines, dim3(1), dim3(kTrackTile), 0, stream, ltiles, static_cast<const long long*>(nullptr), st);
}

void launch_regiontrack_format(const RegionTrackSource& src, const unsigned int* ltiles, long long nlines, long long pos0, const TrackName& name,
                               char* text, long long cap, hipStream_t stream) {
  const int ntiles = track_tiles(nlines);
  if (ntiles <= 0) return;
  RSI_LAUNCH((k_track_format<RegionLines, MeanValue>), dim3(ntiles), dim3(kTrackTile), 0, stream, RegionLines{src.start, src.end},
             MeanValue{src.start, src.end, src.sum}, ltiles, nlines, pos0, name, text, cap);
}

}  // namespace rsik
