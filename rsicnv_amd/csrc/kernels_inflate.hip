// kernels_inflate.hip -- BGZF blocks inflated on the device.  One wave64 workgroup per BGZF member: the
// wave runs the decoder of inflate_core.h with identical state in every lane (Huffman tables and the member's whole output
// in LDS), copies matches and stored bytes 64 lanes at a time, checks ISIZE and CRC32 (each lane the CRC of a 1/64 slice,
// shifted into place with the host-made x^(2^k) constants (a kernel argument) and folded across the wave), then writes the member to HBM with
// coalesced stores and reports its last line end.  A bad member records (member index, reason) in one word and stops; the
// launch always completes.
#include "kernels.h"
#include "inflate_core.h"

namespace rsik {

namespace {

constexpr int kLanes = 64;
constexpr uint32_t kMaxIsize = 65536;

__global__ __launch_bounds__(kLanes) void k_inflate_bgzf(const uint8_t* __restrict__ comp, const InflateBlock* __restrict__ blocks,
                                                         int nblocks, uint8_t* __restrict__ text, int* __restrict__ last_nl,
                                                         unsigned long long* __restrict__ status, const rsinf::X2n x2n) {
  __shared__ uint8_t s_out[kMaxIsize];
  __shared__ rsinf::Work s_w;
  const int b = blockIdx.x;
  if (b >= nblocks) return;
  const int lane = threadIdx.x;
  const InflateBlock B = blocks[b];
  int rc = rsinf::kOk;
  uint32_t produced = 0;
  if (B.isize > kMaxIsize) rc = rsinf::kOutputOverrun;
  else rc = rsinf::inflate_raw(comp + B.coff, B.clen, s_out, B.isize, &produced, s_w, lane, kLanes);
  if (rc == rsinf::kOk && produced != B.isize) rc = rsinf::kSizeMismatch;
  __syncthreads();   // one wave: the CRC slices and the copy-out read bytes other lanes wrote
  if (rc == rsinf::kOk) {
    const uint32_t slice = (B.isize + kLanes - 1) / kLanes;
    const uint32_t lo = min(B.isize, (uint32_t)lane * slice), hi = min(B.isize, lo + slice);
    uint32_t c = rsinf::crc32(0, s_out + lo, hi - lo);
    c = rsinf::shift_bytes(x2n.v, c, B.isize - hi);
    for (int o = kLanes / 2; o > 0; o >>= 1) c ^= (uint32_t)__shfl_xor((int)c, o, kLanes);
    if (c != B.crc) rc = rsinf::kCrcMismatch;
  }
  if (rc != rsinf::kOk) {
    if (lane == 0) atomicMin(status, ((unsigned long long)b << 8) | (unsigned long long)rc);
    return;
  }
  uint8_t* dst = text + B.out;
  int last = -1;
  for (uint32_t i = (uint32_t)lane; i < B.isize; i += kLanes) {
    const uint8_t ch = s_out[i];
    dst[i] = ch;
    if (ch == '\n') last = (int)i;
  }
  for (int o = kLanes / 2; o > 0; o >>= 1) last = max(last, __shfl_xor(last, o, kLanes));
  if (lane == 0 && last >= 0) atomicMax(last_nl, (int)B.out + last);
}

// The names of bounds[k0, k1) (k_text_name_bounds' entries), 256 bytes each, for the host: with BGZF input the text is in
// HBM only.
__global__ __launch_bounds__(256) void k_gather_names(const uint8_t* __restrict__ text, const NameBound* __restrict__ bounds,
                                                      unsigned k0, unsigned k1, char* __restrict__ out) {
  const unsigned i = k0 + blockIdx.x * 256 + threadIdx.x;
  if (i >= k1) return;
  const NameBound nb = bounds[i];
  const int len = nb.len < 255 ? nb.len : 255;
  char* o = out + (size_t)(i - k0) * 256;
  for (int c = 0; c < len; ++c) o[c] = (char)text[nb.name + c];
}

}  // namespace

void launch_gather_names(const void* text, const NameBound* bounds, unsigned k0, unsigned k1, char* out, hipStream_t stream) {
  if (k1 <= k0) return;
  RSI_LAUNCH(k_gather_names, dim3((k1 - k0 + 255) / 256), dim3(256), 0, stream, static_cast<const uint8_t*>(text), bounds, k0, k1, out);
}

void launch_inflate_bgzf(const void* comp, const InflateBlock* blocks, int nblocks, void* text, int* last_nl,
                         unsigned long long* status, hipStream_t stream) {
  static const rsinf::X2n x2n = rsinf::make_x2n();   // kernel argument: the same on every device
  if (nblocks <= 0) return;
  RSI_LAUNCH(k_inflate_bgzf, dim3(nblocks), dim3(kLanes), 0, stream, static_cast<const uint8_t*>(comp), blocks, nblocks,
             static_cast<uint8_t*>(text), last_nl, status, x2n);
}

}  // namespace rsik
