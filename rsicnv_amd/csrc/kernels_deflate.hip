// kernels_deflate.hip -- a slice's text deflated into BGZF members on the device.  k_deflate_bgzf: one workgroup
// of 256 threads per 65280 bytes of text; it stages them in LDS, runs the coder of deflate_core.h (hash table, one deflate block's
// matches and token bits and the code construction beside the text: 153 KiB of the CU's 160, so one workgroup a CU), computes the
// CRC32 as the inflate kernel does (a slice per thread, shifted into place and folded) and frames the payload in its slot of
// 65536 bytes.  k_bgzf_pack: one workgroup per member sums the sizes in front of its own (at most 515) and copies the member
// there; the first leaves the packed length and the stored members' count in the track state.  Plain launches, no hand-over
// inside a kernel: a launch reads what the launch before it wrote.
#include "kernels.h"
#include "deflate_core.h"

namespace rsik {

namespace {

constexpr int kDefThreads = rsdef::kMaxLanes;
constexpr unsigned int kStoredBit = 1u << 31;   // of a size word: the member is one stored block
static_assert(sizeof(rsdef::Work) + rsdef::kMaxText + 64 <= 160 * 1024, "text and scratch of one member fit a CU's LDS");
static_assert(kDeflateMemberText == rsdef::kMaxText && kDeflateSlotBytes == rsdef::kSlotBytes, "kernels.h states the coder's sizes");
static_assert(rsdef::kBgzfHeader + rsdef::kMaxText + 5 + rsdef::kBgzfFooter <= rsdef::kSlotBytes, "a stored member fits its slot");

__global__ __launch_bounds__(kDefThreads) void k_deflate_bgzf(const uint8_t* __restrict__ text, long long nbytes, uint8_t* __restrict__ slots,
                                                              unsigned int* __restrict__ sizes, const rsinf::X2n x2n) {
  __shared__ __attribute__((aligned(16))) uint8_t s_text[rsdef::kMaxText];
  __shared__ rsdef::Work s_w;
  __shared__ unsigned int s_crc;
  const long long off = (long long)blockIdx.x * rsdef::kMaxText;
  if (off >= nbytes) return;   // (the grid is the member count: never)
  const int lane = threadIdx.x;
  const uint32_t len = (uint32_t)(nbytes - off < (long long)rsdef::kMaxText ? nbytes - off : (long long)rsdef::kMaxText);
  // the text is 256-byte aligned and a member's offset a multiple of 16: whole 16-byte words, then the tail
  const uint4* src16 = reinterpret_cast<const uint4*>(text + off);
  uint4* dst16 = reinterpret_cast<uint4*>(s_text);
  for (uint32_t i = (uint32_t)lane; i < len / 16; i += kDefThreads) dst16[i] = src16[i];
  for (uint32_t i = (len & ~15u) + (uint32_t)lane; i < len; i += kDefThreads) s_text[i] = text[off + i];
  if (lane == 0) s_crc = 0;
  __syncthreads();
  uint8_t* member = slots + (size_t)blockIdx.x * rsdef::kSlotBytes;
  int stored = 0;
  const uint32_t payload = rsdef::deflate_raw(s_text, len, member + rsdef::kBgzfHeader, rsdef::kSlotBytes - rsdef::kBgzfHeader - rsdef::kBgzfFooter,
                                              s_w, lane, kDefThreads, &stored);
  const uint32_t piece = (len + kDefThreads - 1) / kDefThreads;
  const uint32_t lo = min(len, (uint32_t)lane * piece), hi = min(len, lo + piece);
  uint32_t c = rsinf::crc32(0, s_text + lo, hi - lo);
  c = rsinf::shift_bytes(x2n.v, c, len - hi);
  atomicXor(&s_crc, c);   // crc(A B) = crc(A) x^(8 |B|) + crc(B): a sum, in any order
  __syncthreads();
  if (lane == 0) {
    rsdef::bgzf_frame(member, payload, s_crc, len);
    sizes[blockIdx.x] = (rsdef::kBgzfHeader + payload + rsdef::kBgzfFooter) | (stored ? kStoredBit : 0u);
  }
}

// sizes[nmembers] -> member b at packed[sum of the sizes in front of it]
__global__ __launch_bounds__(256) void k_bgzf_pack(const uint8_t* __restrict__ slots, const unsigned int* __restrict__ sizes, int nmembers,
                                                   uint8_t* __restrict__ packed, long long cap, TrackState* __restrict__ st) {
  __shared__ unsigned long long s_front, s_total;
  __shared__ unsigned int s_stored;
  const int b = blockIdx.x;
  if (threadIdx.x == 0) { s_front = 0; s_total = 0; s_stored = 0; }
  __syncthreads();
  unsigned long long front = 0, total = 0;
  unsigned int stored = 0;
  for (int i = threadIdx.x; i < nmembers; i += 256) {
    const unsigned int w = sizes[i];
    const unsigned int sz = w & ~kStoredBit;
    total += sz;
    if (i < b) front += sz;
    stored += w >> 31;
  }
  atomicAdd(&s_front, front);
  atomicAdd(&s_total, total);
  atomicAdd(&s_stored, stored);
  __syncthreads();
  if (b == 0 && threadIdx.x == 0) { st->packed = (long long)s_total; st->stored = (long long)s_stored; }
  const unsigned int size = sizes[b] & ~kStoredBit;
  const unsigned long long at = s_front;
  if (size > rsdef::kSlotBytes || at + size > (unsigned long long)cap) return;   // the host refuses the slice by st->packed
  const uint8_t* src = slots + (size_t)b * rsdef::kSlotBytes;
  uint8_t* dst = packed + at;
  // bytes up to the destination's first 4-byte boundary, whole words from there (the slot is read byte-wise: its phase differs)
  const unsigned int head = min(size, (unsigned int)((4 - (at & 3)) & 3));
  if (threadIdx.x < head) dst[threadIdx.x] = src[threadIdx.x];
  const unsigned int words = (size - head) / 4;
  unsigned int* dst4 = reinterpret_cast<unsigned int*>(dst + head);
  for (unsigned int i = threadIdx.x; i < words; i += 256) {
    const uint8_t* s = src + head + 4 * i;
    dst4[i] = (unsigned int)s[0] | ((unsigned int)s[1] << 8) | ((unsigned int)s[2] << 16) | ((unsigned int)s[3] << 24);
  }
  for (unsigned int i = head + 4 * words + threadIdx.x; i < size; i += 256) dst[i] = src[i];
}

}  // namespace

void launch_deflate_bgzf(const void* text, long long nbytes, void* slots, unsigned int* sizes, hipStream_t stream) {
  static const rsinf::X2n x2n = rsinf::make_x2n();   // kernel argument: the same on every device
  const int nmembers = deflate_members(nbytes);
  if (nmembers <= 0) return;
  RSI_LAUNCH(k_deflate_bgzf, dim3(nmembers), dim3(kDefThreads), 0, stream, static_cast<const uint8_t*>(text), nbytes,
             static_cast<uint8_t*>(slots), sizes, x2n);
}

void launch_bgzf_pack(const void* slots, const unsigned int* sizes, int nmembers, void* packed, long long cap, TrackState* st,
                      hipStream_t stream) {
  if (nmembers <= 0) return;
  RSI_LAUNCH(k_bgzf_pack, dim3(nmembers), dim3(256), 0, stream, static_cast<const uint8_t*>(slots), sizes, nmembers,
             static_cast<uint8_t*>(packed), cap, st);
}

}  // namespace rsik
