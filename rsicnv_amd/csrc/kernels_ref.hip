// kernels_ref.hip -- the reference sequence unfolded on the device: a span of a FASTA file's text in HBM -> the
// bases of one sequence, one byte per base, the line terminators left out.  By the .fai's layout base k lies at text offset
// offset + (k / linebases) * linewidth + k % linebases, so nothing is scanned and nothing compacted: every thread computes where
// its sixteen bases lie and picks them.  Nothing is upper-cased or classified (K1 does that).
#include "kernels.h"

namespace rsik {

namespace {

constexpr int kThreads = 256;
static_assert(kRefTileBases == kThreads * 16, "sixteen bases, one 16-byte store, per thread");

struct Fetch {   // a byte of the span by its offset from the span's first byte; outside [lo, hi): not there (the caller counts it)
  const uint8_t* p;   // STAGED: the tile's text in LDS, p[0] = span byte `base`; else the span in HBM, base = 0
  long long base, lo, hi;
  __device__ bool has(long long x) const { return x >= lo && x < hi; }
  __device__ unsigned int at(long long x) const { return p[x - base]; }
};

// One workgroup: the bases [t0, t0 + kRefTileBases) of the sequence, as far as they are in [k0, k1).  t0 is a multiple of 16, so
// a thread's sixteen bases are one aligned 16-byte unit of out[].  STAGED: the tile's text -- one contiguous range of the span --
// goes through LDS in aligned 16-byte loads and the bases are picked from there; the launcher uses it when kRefStageBytes hold
// any tile's text.  Otherwise (terminators of many bytes on very short lines) the bytes are picked from HBM one by one.
// flags[0]: terminator positions holding something other than '\n' / '\r'; flags[1]: base positions holding '\n', '\r' or '>',
// or lying outside the span (a launch whose arguments break the contract counts there instead of reading out of bounds).
template <bool STAGED>
__global__ __launch_bounds__(kThreads) void k_ref_unfold(const uint8_t* __restrict__ span, long long span_off, long long span_len,
                                                         RefLayout L, long long k0, long long k1, uint8_t* __restrict__ out,
                                                         unsigned int* __restrict__ flags) {
  __shared__ uint4 s_text[STAGED ? kRefStageBytes / 16 : 1];
  __shared__ unsigned int s_bad[2];
  const unsigned int lb = (unsigned int)L.linebases, tw = (unsigned int)(L.linewidth - L.linebases);
  const long long t0 = (k0 & ~15ll) + (long long)blockIdx.x * kRefTileBases;
  const long long a = t0 > k0 ? t0 : k0, b = t0 + kRefTileBases < k1 ? t0 + kRefTileBases : k1;   // this tile's bases
  if (threadIdx.x < 2) s_bad[threadIdx.x] = 0;
  const long long rel = L.offset - span_off;   // the sequence's first byte, from the span's
  Fetch F{span, 0, 0, span_len};
  if (STAGED) {
    // the tile's text: from base a's byte to base b - 1's, with the terminator behind it when it ends a line
    const unsigned int qa = (unsigned int)a / lb, qb = (unsigned int)(b - 1) / lb;
    const unsigned int rb = (unsigned int)(b - 1) - qb * lb;
    long long lo = rel + (long long)qa * L.linewidth + ((unsigned int)a - qa * lb);
    long long hi = rel + (long long)qb * L.linewidth + rb + 1 + (rb + 1 == lb ? tw : 0);
    lo = lo < 0 ? 0 : lo;
    hi = hi > span_len ? span_len : hi;
    const long long base = lo & ~15ll;
    if (hi - base > kRefStageBytes) hi = base + kRefStageBytes;   // (never, by the launcher's choice: what lies behind is counted as missing)
    const int nvec = hi > base ? (int)((hi - base + 15) >> 4) : 0;
    const uint4* src = reinterpret_cast<const uint4*>(span + base);   // the span's buffer is 16-byte aligned and padded to 16
    for (int i = threadIdx.x; i < nvec; i += kThreads) s_text[i] = src[i];
    F = Fetch{reinterpret_cast<const uint8_t*>(s_text), base, lo, hi};
  }
  __syncthreads();
  const long long g = t0 + (long long)threadIdx.x * 16;
  unsigned int bad_term = 0, bad_base = 0;
  if (g < b && g + 16 > a) {
    const unsigned int q = (unsigned int)g / lb;
    unsigned int r = (unsigned int)g - q * lb;
    long long x = rel + (long long)q * L.linewidth + r;
    unsigned int w[4] = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const long long k = g + j;
      const bool mine = k >= a && k < b;
      if (mine) {
        unsigned int c = 0;
        if (F.has(x)) { c = F.at(x); bad_base += (c == '\n' || c == '\r' || c == '>') ? 1u : 0u; }
        else ++bad_base;
        w[j >> 2] |= c << (8 * (j & 3));
      }
      ++x; ++r;
      if (r == lb) {   // a full line ends: its terminator, as far as the span holds it (at the end of the file the last one may be cut or missing)
        if (mine)
          for (unsigned int t = 0; t < tw && x + t < span_len; ++t) { const unsigned int c = F.has(x + t) ? F.at(x + t) : 0u; bad_term += (c == '\n' || c == '\r') ? 0u : 1u; }
        x += tw; r = 0;
      }
    }
    if (g >= a && g + 16 <= b) *reinterpret_cast<uint4*>(out + g) = make_uint4(w[0], w[1], w[2], w[3]);
    else
      for (int j = 0; j < 16; ++j) if (g + j >= a && g + j < b) out[g + j] = (uint8_t)(w[j >> 2] >> (8 * (j & 3)));
  }
  if (bad_term) atomicAdd(&s_bad[0], bad_term);
  if (bad_base) atomicAdd(&s_bad[1], bad_base);
  __syncthreads();
  if (threadIdx.x < 2 && s_bad[threadIdx.x]) atomicAdd(&flags[threadIdx.x], s_bad[threadIdx.x]);
}

}  // namespace

bool ref_unfold_staged(const RefLayout& L) {
  // the longest text a tile of kRefTileBases bases spans: its bases, a terminator per line begun, the alignment in front
  const long long lines = kRefTileBases / L.linebases + 2;
  return kRefTileBases + lines * (long long)(L.linewidth - L.linebases) + 16 <= kRefStageBytes;
}

void launch_ref_unfold(const void* span, long long span_off, long long span_len, const RefLayout& L, long long k0, long long k1,
                       void* out, unsigned int* flags, hipStream_t stream) {
  if (k1 <= k0) return;
  const long long tiles = (k1 - (k0 & ~15ll) + kRefTileBases - 1) / kRefTileBases;
  if (ref_unfold_staged(L))
    RSI_LAUNCH(k_ref_unfold<true>, dim3((unsigned int)tiles), dim3(kThreads), 0, stream, static_cast<const uint8_t*>(span), span_off, span_len, L,
               k0, k1, static_cast<uint8_t*>(out), flags);
  else
    RSI_LAUNCH(k_ref_unfold<false>, dim3((unsigned int)tiles), dim3(kThreads), 0, stream, static_cast<const uint8_t*>(span), span_off, span_len, L,
               k0, k1, static_cast<uint8_t*>(out), flags);
}

}  // namespace rsik
