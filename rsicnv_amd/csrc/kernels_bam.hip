// kernels_bam.hip -- the records of a chunk of inflated BAM bytes found on the device: guess, walk, verify.
// The chunk is cut into segments of RSI_BAM_SEGMENT bytes, unrelated to BGZF members.  k_bam_guess tests every byte offset of
// a segment as a record start (one workgroup per segment, the segment and a halo staged in LDS); k_bam_walk follows the chain
// of every segment from its guess (one thread per segment, straight from HBM: the chain is a few dozen dependent loads
// per segment, all segments at once); k_bam_stitch, one workgroup, goes through the segments in order with the true entry,
// keeps the walks that began at it, walks the others again, and compacts the kept lists into the ascending rec_off[] that
// launch_bam_depth takes.  The per-offset logic is bam_walk_core.h's, the host harness's own.
#include "kernels.h"

namespace rsik {

namespace {

constexpr int kGuessThreads = 256;
constexpr uint32_t kSeg = RSI_BAM_SEGMENT;
constexpr uint32_t kHalo = 320;                    // the fixed fields and the longest name behind a segment's last offset (36 + 255), rounded up
constexpr uint32_t kStageBytes = kSeg + kHalo + 8; // + the bytes in front of an unaligned segment start and behind a ragged end
constexpr uint32_t kListCap = RSI_BAM_SEGMENT / 36 + 1;

// Chunk bytes [lo, hi) from LDS, every other offset from HBM
struct Staged {
  const uint8_t* lds; uint64_t lo, hi; const uint8_t* g;
  __device__ inline uint8_t at(uint64_t i) const { return i >= lo && i < hi ? lds[i - lo] : g[i]; }
};

__global__ __launch_bounds__(kGuessThreads) void k_bam_guess(const uint8_t* __restrict__ data, uint32_t len, int nref,
                                                             const int32_t* __restrict__ reflen, uint32_t* __restrict__ guess) {
  __shared__ uint32_t s_stage[kStageBytes / 4];
  __shared__ uint32_t s_best;
  const uint32_t a = blockIdx.x * kSeg;
  if (a >= len) return;
  const uint32_t b = min(a + kSeg, len), top = min(b + kHalo, len);
  // whole words from the word that holds data[a] to the one that holds data[top - 1]: up to 3 bytes on either side of the
  // chunk are read, inside the loader's buffer (kernels.h)
  const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t>(data + a) & 3);
  const uint32_t* src = reinterpret_cast<const uint32_t*>(data + a - mis);
  const uint32_t nwords = (mis + (top - a) + 3) / 4;
  for (uint32_t w = threadIdx.x; w < nwords; w += kGuessThreads) s_stage[w] = src[w];
  if (threadIdx.x == 0) s_best = rsibam::kNone;
  __syncthreads();
  const Staged d{reinterpret_cast<const uint8_t*>(s_stage) + mis, a, top, data};
  // thread t takes the offsets a + t, a + t + 256, ...: ascending, so its first hit is its lowest
  for (uint32_t p = a + threadIdx.x; p < b; p += kGuessThreads) {
    if (p >= *(volatile uint32_t*)&s_best) break;
    if (rsibam::guess_chain(d, (uint64_t)len, (uint64_t)p, nref, reflen)) { atomicMin(&s_best, p); break; }
  }
  __syncthreads();
  if (threadIdx.x == 0) guess[blockIdx.x] = s_best;
}

__global__ __launch_bounds__(64) void k_bam_walk(const uint8_t* __restrict__ data, uint32_t len, uint32_t nseg, int tid,
                                                 const uint32_t* __restrict__ guess, rsibam::SegOut* __restrict__ out,
                                                 uint32_t* __restrict__ lists) {
  const uint32_t s = blockIdx.x * 64 + threadIdx.x;
  if (s >= nseg) return;
  const uint32_t g = guess[s];
  const uint32_t b = min((s + 1) * kSeg, len);
  rsibam::SegOut o{rsibam::kNone, 0, 0, 0};
  if (g != rsibam::kNone && g < b) o = rsibam::walk_segment(rsibam::Span{data}, (uint64_t)len, (uint64_t)g, (uint64_t)b, tid, lists + (size_t)s * kListCap, kListCap);
  out[s] = o;
}

constexpr int kStitchThreads = 256;
constexpr uint32_t kStitchTile = 512;              // segments whose results sit in LDS at a time: 10 KB, so that the kernel finds room on a CU
                                                   // beside the inflate workgroups of the next chunk (two of them hold 132 of its 160 KB)

__global__ __launch_bounds__(kStitchThreads) void k_bam_stitch(const uint8_t* __restrict__ data, uint32_t len, uint32_t nseg, int tid,
                                                               const uint32_t* __restrict__ guess, const rsibam::SegOut* __restrict__ out,
                                                               uint32_t* __restrict__ lists, uint32_t* __restrict__ rec_off,
                                                               rsibam::Report* __restrict__ report) {
  __shared__ rsibam::SegOut s_out[kStitchTile];
  __shared__ uint32_t s_acc[kStitchTile];           // the guesses, then the accepted counts (the core's stitch allows the alias)
  __shared__ uint32_t s_wave[kStitchThreads / 64];
  __shared__ rsibam::StitchState s_st;
  if (threadIdx.x == 0) s_st = rsibam::stitch_begin(0);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t carry = 0;                               // records listed by the tiles before
  for (uint32_t t0 = 0; t0 < nseg; t0 += kStitchTile) {
    const uint32_t nt = min(kStitchTile, nseg - t0);
    for (uint32_t k = threadIdx.x; k < nt; k += kStitchThreads) { s_acc[k] = guess[t0 + k]; s_out[k] = out[t0 + k]; }
    __syncthreads();
    if (threadIdx.x == 0) rsibam::stitch_tile(rsibam::Span{data}, (uint64_t)len, kSeg, t0, t0 + nt, tid, s_acc, s_out, lists, kListCap, s_acc, s_st);
    __syncthreads();
    // exclusive scan of the tile's accepted counts into s_out[].exit (the walks' results are used up)
    for (uint32_t k0 = 0; k0 < nt; k0 += kStitchThreads) {
      const uint32_t k = k0 + threadIdx.x;
      const uint32_t v = k < nt ? s_acc[k] : 0;
      uint32_t incl = v;
      for (int dd = 1; dd < 64; dd <<= 1) { const uint32_t up = __shfl_up(incl, dd); if (lane >= dd) incl += up; }
      if (lane == 63) s_wave[wave] = incl;
      __syncthreads();
      uint32_t base = 0, tot = 0;
      for (int w = 0; w < kStitchThreads / 64; ++w) { if (w < wave) base += s_wave[w]; tot += s_wave[w]; }
      if (k < nt) s_out[k].exit = carry + base + incl - v;
      carry += tot;
      __syncthreads();
    }
    // a wave per segment copies its list to its place
    for (uint32_t k = wave; k < nt; k += kStitchThreads / 64) {
      const uint32_t cnt = s_acc[k], at = s_out[k].exit;
      const uint32_t* l = lists + (size_t)(t0 + k) * kListCap;
      for (uint32_t i = lane; i < cnt; i += 64) rec_off[at + i] = l[i];
    }
    const bool stopped = s_st.stopped != 0;         // (read before the barrier: thread 0 writes it again only behind the next one)
    __syncthreads();
    if (stopped) break;                             // the chain has ended: nothing behind it is listed
  }
  if (threadIdx.x == 0) *report = s_st.r;
}

}  // namespace

int bam_segments(long long len) { return len <= 0 ? 0 : (int)((len + RSI_BAM_SEGMENT - 1) / RSI_BAM_SEGMENT); }

void launch_bam_guess(const void* data, long long len, int nref, const int32_t* reflen, uint32_t* guess, hipStream_t stream) {
  const int nseg = bam_segments(len);
  if (nseg <= 0) return;
  RSI_LAUNCH(k_bam_guess, dim3(nseg), dim3(kGuessThreads), 0, stream, static_cast<const uint8_t*>(data), (uint32_t)len, nref, reflen, guess);
}
void launch_bam_walk(const void* data, long long len, int tid, const uint32_t* guess, BamSegOut* out, uint32_t* lists, hipStream_t stream) {
  const int nseg = bam_segments(len);
  if (nseg <= 0) return;
  RSI_LAUNCH(k_bam_walk, dim3((nseg + 63) / 64), dim3(64), 0, stream, static_cast<const uint8_t*>(data), (uint32_t)len, (uint32_t)nseg, tid, guess,
             out, lists);
}
void launch_bam_stitch(const void* data, long long len, int tid, const uint32_t* guess, const BamSegOut* out, uint32_t* lists, uint32_t* rec_off,
                       BamFindReport* report, hipStream_t stream) {
  const int nseg = bam_segments(len);
  RSI_LAUNCH(k_bam_stitch, dim3(1), dim3(kStitchThreads), 0, stream, static_cast<const uint8_t*>(data), (uint32_t)len, (uint32_t)nseg, tid, guess,
             out, lists, rec_off, report);
}

}  // namespace rsik
