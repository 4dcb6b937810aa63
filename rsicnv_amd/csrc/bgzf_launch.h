// bgzf_launch.h -- the one place where BGZF members are inflated on the device and a bad member is reported: a
// batch of members queued on a stream (payloads and member table up, status word set, launch_inflate_bgzf, status word back),
// and the word decoded behind the caller's wait.  The depth-text readers and the reference (chunk_source.h), the BAM's device
// read (ingest_bam.hip) and rsi_hot_inflate_bgzf (ingest.hip) differ in where the bytes come from and in how the message
// names the file; the sequence is this one.  Part of pipeline_internal.h, which includes it behind DevBuf and PinBuf (the
// context holds three of these).
#pragma once

// rsing: what the ingest units (ingest*.hip, ref.hip) share among themselves; none of it is a symbol of the library
namespace rsing __attribute__((visibility("hidden"))) {

constexpr size_t kMemberMax = 65536;   // a BGZF member's BSIZE and ISIZE at the most

// two DevBuf or PinBuf trade their allocations (staging lent to a reader and taken back: ref.hip)
template <class B> void swap_buf(B& a, B& b) { std::swap(a.p, b.p); std::swap(a.cap, b.cap); }

struct BgzfLaunch {
  rsip::PinBuf tpin, wpin;           // the member table on its way up; the status word (8 bytes) and last_nl (4) back on the host
  rsip::DevBuf tdev, wdev;
  hipEvent_t before = nullptr, after = nullptr;   // the caller's, around the last launch (either may be null)
  void swap(BgzfLaunch& o) { swap_buf(tpin, o.tpin); swap_buf(wpin, o.wpin); swap_buf(tdev, o.tdev); swap_buf(wdev, o.wdev); }

  struct Result {
    bool ok;             // every member inflated, its ISIZE and CRC32 right
    size_t member;       // else: the first bad member's index in the table ...
    int error;           // ... and what is wrong with it (rsinf::Err)
    int last_nl;         // offset of the last line end in the text (the start value when there is none)
    double kernel_ms;    // between `before` and `after` (0 without both)
  };

  // staging for a launch of `members` members
  hipError_t reserve(size_t members) {
    hipError_t e = tpin.ensure(members * sizeof(rsik::InflateBlock));
    if (e == hipSuccess) e = tdev.ensure(members * sizeof(rsik::InflateBlock));
    if (e == hipSuccess) e = wpin.ensure(16);
    if (e == hipSuccess) e = wdev.ensure(16);
    return e;
  }

  // Queued on s: comp[0, comp_bytes) (pinned, or any host memory) to d_comp and the table to the device, the status word set
  // to "no bad member" and last_nl to its start value, ev_before, the inflate of every member into d_text, ev_after, the
  // word's copy to the host.  reserve(tab.size()) comes first; result() is good once the caller has waited behind this.
  hipError_t queue(const std::vector<rsik::InflateBlock>& tab, const void* comp, size_t comp_bytes, void* d_comp, void* d_text, int last_nl,
                   hipStream_t s, hipEvent_t ev_before = nullptr, hipEvent_t ev_after = nullptr) {
    const size_t tb = tab.size() * sizeof(rsik::InflateBlock);
    memcpy(tpin.p, tab.data(), tb);
    char* w = wdev.as<char>();
    before = ev_before; after = ev_after;
    hipError_t e = hipMemcpyAsync(d_comp, comp, comp_bytes, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(tdev.p, tpin.p, tb, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemsetAsync(w, 0xff, 16, s);   // status ~0, last_nl -1
    if (e == hipSuccess && last_nl != -1) e = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(w + 8), last_nl, 1, s);
    if (e == hipSuccess && before) e = hipEventRecord(before, s);
    if (e != hipSuccess) return e;
    rsik::launch_inflate_bgzf(d_comp, tdev.as<rsik::InflateBlock>(), (int)tab.size(), d_text, reinterpret_cast<int*>(w + 8),
                              reinterpret_cast<unsigned long long*>(w), s);
    if (after) e = hipEventRecord(after, s);
    if (e == hipSuccess) e = hipMemcpyAsync(wpin.p, w, 16, hipMemcpyDeviceToHost, s);
    return e;
  }

  // behind the caller's wait: the status word is (member index << 8 | rsinf::Err) of the first bad member, ~0 without one
  Result result() const {
    unsigned long long status;
    memcpy(&status, wpin.p, 8);
    Result r{status == ~0ull, (size_t)(status >> 8), (int)(status & 0xff), -1, before && after ? rsip::elapsed_ms(before, after) : 0.0};
    memcpy(&r.last_nl, wpin.as<char>() + 8, 4);
    return r;
  }
};

}  // namespace rsing
