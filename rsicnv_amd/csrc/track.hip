// track.hip -- depth tracks and per-bin tracks as bedGraph (include/rsi_hot.h: rsi_hot_write_track, _write_track_device,
// rsi_hot_debug_track; rsi_hot_write_bin_track, rsi_hot_debug_bin_track), as text or as BGZF (rsi_hot_set_track_format).  The
// host drives kernels_track.hip slice by slice: the passes that find and measure a slice's lines, one wait for their two numbers,
// the format pass and the copy of exactly those bytes into one of two pinned buffers; while that runs, the slice before goes
// out through write().  A BGZF slice is deflated and packed behind its format pass (kernels_deflate.hip) and only the packed
// members are copied, one slice later: their length comes with the next slice's two numbers.  Slice rules, bounds and numbers:
// DESIGN.md 6f, 6g and 6h.
#include "pipeline_internal.h"
#include "track_host.h"
#include "track_index_host.h"
#include "depth_host.h"
#include <sys/stat.h>
#include <new>

using namespace rsik;
using namespace rsip;

namespace rsip {

void track_free(rsi_ctx* ctx) {
  rsi_ctx::TrackWs& w = ctx->track;
  if (w.dev) (void)hipFree(w.dev);
  for (char*& p : w.pin) { if (p) (void)hipHostFree(p); p = nullptr; }
  if (w.pin_state) (void)hipHostFree(w.pin_state);
  for (hipEvent_t& e : w.ev) { if (e) (void)hipEventDestroy(e); e = nullptr; }
  if (w.idx_dev) (void)hipFree(w.idx_dev);
  if (w.idx_pin) (void)hipHostFree(w.idx_pin);
  w.idx_dev = nullptr; w.idx_pin = nullptr; w.idx_bytes = 0;
  w.dev = w.pin_state = nullptr; w.dev_bytes = w.pin_bytes = 0;
}

}  // namespace rsip

namespace {

// Where a slice's text goes: a file, or (the test hook) host memory.
struct TrackSink {
  int fd = -1;
  std::string* text = nullptr;
  int64_t base = 0;   // bytes the file held before this call (what an index adds to its offsets)
  bool put(const char* p, size_t len) {
    if (text) { text->append(p, len); return true; }
    return rsitrack::write_all(fd, p, len);
  }
};

// events: the measuring passes; per pinned buffer: format begin / end, copy done, deflate and pack done, index pass done
enum { kEvP0, kEvP1, kEvF0, kEvF1 = kEvF0 + 2, kEvCopy = kEvF1 + 2, kEvD1 = kEvCopy + 2, kEvX1 = kEvD1 + 2, kEvCount = kEvX1 + 2 };
static_assert(kEvCount == sizeof(rsi_ctx::TrackWs::ev) / sizeof(hipEvent_t), "one event per use");

struct TrackLayout {
  size_t text, starts, tiles, ltiles, state, table, bytes;
  size_t sizes = 0, slots = 0, packed = 0;   // BGZF only: a size word and a slot per member of a slice, the members packed
  int64_t packed_cap = 0;
  size_t pin_bytes = 0;                      // what a slice sends to the host at most
};
size_t up256(size_t x) { return (x + 255) & ~size_t(255); }
// text_cap bytes of text, `entries` 8-byte starts or pieces, tile words for `items` (passes 1-3) and `lines` (passes 4-5),
// the state, and table_words 8-byte words of a region table; bgzf: what the members of text_cap bytes of text need on top
TrackLayout track_layout(int64_t text_cap, int64_t entries, int64_t items, int64_t lines, size_t table_words, bool bgzf) {
  TrackLayout L;
  L.text = 0;
  L.starts = up256((size_t)text_cap);
  L.tiles = L.starts + up256((size_t)entries * 8);
  L.ltiles = L.tiles + up256((size_t)(track_tiles(items) + 1) * 4);
  L.state = L.ltiles + up256((size_t)(track_tiles(lines) + 1) * 4);
  L.table = L.state + up256(sizeof(TrackState));
  L.bytes = L.table + up256(table_words * 8);
  L.pin_bytes = (size_t)text_cap;
  if (bgzf) {
    const int64_t members = rsitrack::members_of(text_cap);
    L.sizes = L.bytes;
    L.slots = L.sizes + up256((size_t)members * 4);
    L.packed = L.slots + (size_t)members * rsitrack::kMemberSlot;
    L.packed_cap = text_cap + members * rsitrack::kMemberOverhead;
    L.bytes = L.packed + up256((size_t)L.packed_cap);
    L.pin_bytes = (size_t)L.packed_cap;
  }
  return L;
}
TrackLayout track_layout(const rsitrack::Plan& p, bool bgzf) { return track_layout(p.text_cap, p.slice + 2, p.slice, p.slice + 1, 0, bgzf); }
static_assert(rsitrack::kMemberText == kDeflateMemberText && rsitrack::kMemberSlot == kDeflateSlotBytes, "the host plans the kernels' members");

// The compressed side of a call: where the members go on the device, and the figures (null / zero for a plain-text call)
struct TrackBgzf {
  unsigned int* sizes = nullptr;
  char* slots = nullptr;
  char* packed = nullptr;
  int64_t packed_cap = 0;
  rsi_deflate_stats D{};
  bool on() const { return packed != nullptr; }
  void place(void* dev, const TrackLayout& L) {
    sizes = reinterpret_cast<unsigned int*>(static_cast<char*>(dev) + L.sizes);
    slots = static_cast<char*>(dev) + L.slots;
    packed = static_cast<char*>(dev) + L.packed;
    packed_cap = L.packed_cap;
  }
};

int track_ensure(rsi_ctx* ctx, const TrackLayout& L) {
  rsi_ctx::TrackWs& w = ctx->track;
  for (hipEvent_t& e : w.ev) if (!e) HIPCHK(hipEventCreate(&e));
  if (!w.pin_state) HIPCHK(hipHostMalloc(&w.pin_state, 2 * sizeof(TrackState), hipHostMallocDefault));
  if (L.bytes > w.dev_bytes) {
    if (w.dev) (void)hipFree(w.dev);
    w.dev = nullptr; w.dev_bytes = 0;
    HIPCHK(hipMalloc(&w.dev, L.bytes));
    w.dev_bytes = L.bytes;
  }
  if (L.pin_bytes > w.pin_bytes) {
    for (char*& b : w.pin) { if (b) (void)hipHostFree(b); b = nullptr; }
    w.pin_bytes = 0;
    for (char*& b : w.pin) HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&b), L.pin_bytes, hipHostMallocDefault));
    w.pin_bytes = L.pin_bytes;
  }
  return RSI_OK;
}

// The index side of a call (null / off without rsi_hot_set_track_index): the builder, the call's name and file offset, and where a
// slice's records go on the device and in pinned memory.  A slice's records are laid out for its own capacities, so that one
// copy of exactly track_index_bytes() brings them over.
struct TrackIndexer {
  rsi_track_index* ix = nullptr;
  std::string name;
  int64_t base = 0;                   // the file's size before this call
  unsigned int chunk_cap = 0, win_cap = 0;   // of the slice whose records lie in pinned memory (or are on their way there)
  bool on() const { return ix != nullptr; }
};
int track_index_ensure(rsi_ctx* ctx, size_t bytes) {
  rsi_ctx::TrackWs& w = ctx->track;
  if (bytes <= w.idx_bytes) return RSI_OK;
  if (w.idx_dev) (void)hipFree(w.idx_dev);
  if (w.idx_pin) (void)hipHostFree(w.idx_pin);
  w.idx_dev = nullptr; w.idx_pin = nullptr; w.idx_bytes = 0;
  HIPCHK(hipMalloc(&w.idx_dev, bytes));
  HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&w.idx_pin), bytes, hipHostMallocDefault));
  w.idx_bytes = bytes;
  return RSI_OK;
}
// What every indexed call checks before it writes anything
int track_index_admit(rsi_ctx* ctx, bool bgzf, int64_t last_end) {
  if (!bgzf) return fail(ctx, RSI_ERR_BAD_ARG, "track: an index is set (rsi_hot_set_track_index) and the format is text: only a BGZF track is indexed");
  if (last_end > rsitbx::kMaxEnd) return fail(ctx, RSI_ERR_UNSUPPORTED, "track: a line would end beyond 2^29 = 536870912, the limit of a tabix index");
  return RSI_OK;
}

// The slices of one call, whatever their lines come from: per slice [b, end) of `count` items, measure(b, end) queues the passes
// that find and measure its lines; one wait for the state's two numbers, checked against max_lines(b, end), text_cap and
// max_line; format(b, nlines) queues the format pass, the text is copied into one of the two pinned buffers, and the slice
// before goes to the sink meanwhile.  With z.on() the format pass is followed by the deflate and pack passes, and what is copied
// are the packed members: their length is read together with the NEXT slice's state (the same stream: the pack is done by then),
// so the copy is issued one slice later and a slice still costs one wait; the last slice's length takes one wait of its own,
// once a call.  With X.on() (a BGZF call) windows(b, end) bounds the 16 384-base windows the slice's lines span and
// index(b, nlines, nbytes, out) queues the index pass behind the pack; its records are copied at once, for the slice's capacities,
// and read where the slice's compressed size is read: behind a wait the slice has anyway.  Nothing of the call is still queued
// when this returns.
template <class Measure, class MaxLines, class Format, class Windows, class Index>
int track_slices(rsi_ctx* ctx, int64_t count, int64_t slice, int64_t text_cap, int64_t max_line, TrackState* d_st, const char* d_text,
                 TrackSink& sink, rsi_track_stats& S, TrackBgzf& z, TrackIndexer& X, Measure measure, MaxLines max_lines, Format format,
                 Windows windows, Index index) {
  rsi_ctx::TrackWs& w = ctx->track;
  TrackState* h_st = static_cast<TrackState*>(w.pin_state);
  hipStream_t st = ctx->stream;
  int rc = RSI_OK;
  auto leave = [&](int code, const std::string& msg) { (void)ctx_sync(ctx); return fail(ctx, code, msg); };
  auto hip_failed = [&](hipError_t e, const char* what) { return leave(RSI_ERR_HIP, std::string("track: ") + what + ": " + hipGetErrorString(e)); };
  auto elapsed = [&](int a, int b) { return elapsed_ms(w.ev[a], w.ev[b]); };
  hipError_t e = hipSuccess;
  int pending = -1, next_buf = 0;   // the pinned buffer whose slice is formatted and on its way, not yet in the sink
  int64_t pending_bytes = 0;
  auto flush = [&]() -> int {       // the pending slice: wait for its copy, note its format time, hand it to the sink
    if (pending < 0) return RSI_OK;
    const hipError_t ew = event_wait(w.ev[kEvCopy + pending]);
    if (ew == hipErrorLaunchTimeOut) ctx->poisoned = true;
    if (ew != hipSuccess) return fail(ctx, RSI_ERR_HIP, std::string("track: waiting for a slice's text: ") + hipGetErrorString(ew));
    S.t_kernel_ms += elapsed(kEvF0 + pending, kEvF1 + pending);
    if (z.on()) z.D.t_kernel_ms += elapsed(kEvF1 + pending, kEvD1 + pending);
    if (X.on()) S.t_kernel_ms += elapsed(kEvD1 + pending, kEvX1 + pending);
    const double t0 = now_ms();
    const bool ok = sink.put(w.pin[pending], (size_t)pending_bytes);
    const int err = errno;
    S.t_write_ms += now_ms() - t0;
    pending = -1;
    if (!ok) return fail(ctx, RSI_ERR_INTERNAL, std::string("track: write failed: ") + strerror(err));
    return RSI_OK;
  };
  // BGZF: the slice whose members lie packed on the device, their length not yet known to the host
  int packed_buf = -1;
  int64_t packed_text = 0;
  auto copy_packed = [&]() -> int {   // h_st[0] holds the state read behind that slice's pack: copy its members, make it the pending slice
    const int64_t members = rsitrack::members_of(packed_text), bytes = h_st[0].packed, stored = h_st[0].stored;
    if (bytes <= 0 || bytes > packed_text + members * rsitrack::kMemberOverhead || bytes > z.packed_cap || stored < 0 || stored > members)
      return leave(RSI_ERR_INTERNAL, "track: a slice's compressed size is out of range");
    if (X.on()) {   // the slice's records: copied behind its index pass, in front of the wait that brought `bytes`
      const TrackIndexOut r = track_index_out(w.idx_pin, X.chunk_cap, X.win_cap);
      if (r.head->bad || r.head->nchunk > r.chunk_cap || r.head->nwin > r.win_cap)
        return leave(RSI_ERR_INTERNAL, "track: a slice's index records are out of range");
      static_assert(sizeof(rsitbx::Rec) == sizeof(TrackIndexRec), "the builder reads the device's records");
      const int k = X.ix->add_slice(X.name, X.base + z.D.file_bytes, bytes, reinterpret_cast<const rsitbx::Rec*>(r.chunks), r.head->nchunk,
                                    reinterpret_cast<const rsitbx::Rec*>(r.wins), r.head->nwin);
      if (k != rsitbx::kOk) return leave(k == rsitbx::kUnsupported ? RSI_ERR_UNSUPPORTED : RSI_ERR_INTERNAL, X.ix->err);
    }
    z.D.members += members;
    z.D.stored_members += stored;
    z.D.text_bytes += packed_text;
    z.D.file_bytes += bytes;
    e = hipMemcpyAsync(w.pin[packed_buf], z.packed, (size_t)bytes, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipEventRecord(w.ev[kEvCopy + packed_buf], st);
    if (e != hipSuccess) return hip_failed(e, "hipMemcpyAsync");
    pending = packed_buf; pending_bytes = bytes;
    packed_buf = -1;
    return RSI_OK;
  };
  for (int64_t b = 0; b < count; b += slice) {
    const int64_t end = std::min(count, b + slice);
    (void)hipEventRecord(w.ev[kEvP0], st);
    measure(b, end);
    (void)hipEventRecord(w.ev[kEvP1], st);
    e = hipMemcpyAsync(&h_st[0], d_st, sizeof(TrackState), hipMemcpyDeviceToHost, st);
    if (e != hipSuccess) return hip_failed(e, "hipMemcpyAsync");
    e = ctx_sync(ctx);   // (the slice before has been formatted and copied by now too: same stream)
    if (e != hipSuccess) return fail(ctx, RSI_ERR_HIP, std::string("track: waiting for a slice's line count: ") + hipGetErrorString(e));
    S.t_kernel_ms += elapsed(kEvP0, kEvP1);
    const int64_t nlines = h_st[0].nlines, nbytes = h_st[0].nbytes;
    // the format pass writes nbytes of text for nlines lines: both must be what this slice's buffers were sized for
    if (nlines < 0 || nlines > max_lines(b, end) || nbytes < 0 || nbytes > text_cap || nbytes > nlines * max_line)
      return leave(RSI_ERR_INTERNAL, "track: a slice's line or byte count is out of range");
    ++S.slices;
    S.lines += nlines;
    S.bytes += nbytes;
    if (packed_buf >= 0 && (rc = copy_packed()) != RSI_OK) return rc;   // the slice before: out of the packed buffer before this one's pack
    int fresh = -1;
    if (nlines > 0) {
      fresh = next_buf;
      next_buf ^= 1;   // (at most one slice is pending, in the other buffer)
      (void)hipEventRecord(w.ev[kEvF0 + fresh], st);
      format(b, nlines);
      (void)hipEventRecord(w.ev[kEvF1 + fresh], st);
      if (z.on()) {
        launch_deflate_bgzf(d_text, nbytes, z.slots, z.sizes, st);
        launch_bgzf_pack(z.slots, z.sizes, deflate_members(nbytes), z.packed, z.packed_cap, d_st, st);
        (void)hipEventRecord(w.ev[kEvD1 + fresh], st);
        if (X.on()) {
          const int64_t span = windows(b, end);
          X.chunk_cap = rsitbx::chunk_capacity(span); X.win_cap = rsitbx::window_capacity(span);
          const size_t xbytes = track_index_bytes(X.chunk_cap, X.win_cap);
          if (xbytes > w.idx_bytes) return leave(RSI_ERR_INTERNAL, "track: a slice's index records do not fit their buffer");
          e = hipMemsetAsync(w.idx_dev, 0, sizeof(TrackIndexHead), st);
          if (e != hipSuccess) return hip_failed(e, "hipMemsetAsync");
          index(b, nlines, nbytes, track_index_out(w.idx_dev, X.chunk_cap, X.win_cap));
          (void)hipEventRecord(w.ev[kEvX1 + fresh], st);
          e = hipMemcpyAsync(w.idx_pin, w.idx_dev, xbytes, hipMemcpyDeviceToHost, st);
          if (e != hipSuccess) return hip_failed(e, "hipMemcpyAsync");
        }
      } else {
        e = hipMemcpyAsync(w.pin[fresh], d_text, (size_t)nbytes, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipEventRecord(w.ev[kEvCopy + fresh], st);
        if (e != hipSuccess) return hip_failed(e, "hipMemcpyAsync");
      }
    }
    if ((rc = flush()) != RSI_OK) { (void)ctx_sync(ctx); return rc; }   // the slice before, while this one is formatted and copied
    if (fresh >= 0 && z.on()) { packed_buf = fresh; packed_text = nbytes; }
    else if (fresh >= 0) { pending = fresh; pending_bytes = nbytes; }
  }
  if (packed_buf >= 0) {   // the last slice's members: their length has no next slice to travel with
    e = hipMemcpyAsync(&h_st[0], d_st, sizeof(TrackState), hipMemcpyDeviceToHost, st);
    if (e != hipSuccess) return hip_failed(e, "hipMemcpyAsync");
    e = ctx_sync(ctx);
    if (e != hipSuccess) return fail(ctx, RSI_ERR_HIP, std::string("track: waiting for a slice's compressed size: ") + hipGetErrorString(e));
    if ((rc = copy_packed()) != RSI_OK) return rc;
  }
  if ((rc = flush()) != RSI_OK) { (void)ctx_sync(ctx); return rc; }
  e = ctx_sync(ctx);   // collects a launch error of the last format pass
  if (e != hipSuccess) return fail(ctx, RSI_ERR_HIP, std::string("track: ") + hipGetErrorString(e));
  return RSI_OK;
}

// d_v[0, n) as bedGraph lines of `chrom` into the sink.
int track_run(rsi_ctx* ctx, const int32_t* d_v, int64_t n, const char* chrom, int64_t pos0, int64_t slice_bases, TrackSink& sink,
              rsi_track_stats* stats) {
  const double t_begin = now_ms();
  rsi_track_stats S;
  memset(&S, 0, sizeof(S));
  if (stats) *stats = S;
  ctx->last_deflate = rsi_deflate_stats{};
  const bool bgzf = ctx->track_format == RSI_TRACK_BGZF;
  const int name_len = rsitrack::name_length(chrom);
  if (name_len < 0) return fail(ctx, RSI_ERR_BAD_ARG, "track: the name must have 1 to 255 bytes and no tab or newline");
  rsitrack::Plan plan;
  if (!rsitrack::plan(name_len, pos0, n, slice_bases, plan)) return fail(ctx, RSI_ERR_BAD_ARG, "track: bad length or coordinate offset");
  S.n = n;
  TrackIndexer X;
  if (ctx->track_index) {
    const int rc = track_index_admit(ctx, bgzf, pos0 + n);
    if (rc != RSI_OK) return rc;
    if (pos0 < 0) return fail(ctx, RSI_ERR_BAD_ARG, "track: an indexed track has no negative coordinates");
    X.ix = ctx->track_index; X.name.assign(chrom, (size_t)name_len); X.base = sink.base;
  }
  if (n == 0) { if (stats) *stats = S; return RSI_OK; }
  if (!d_v) return fail(ctx, RSI_ERR_BAD_ARG, "track: no values");
  HIPCHK(hipSetDevice(ctx->device));
  if (!ctx_enter(ctx)) return RSI_ERR_HIP;
  const TrackLayout L = track_layout(plan, bgzf);
  int rc = track_ensure(ctx, L);
  if (rc != RSI_OK) return rc;
  // a slice's lines end inside it: they span the windows of its plan.slice bases, one more where it does not start on a boundary
  if (X.on() && (rc = track_index_ensure(ctx, track_index_bytes(rsitbx::chunk_capacity(plan.slice / 16384 + 2), rsitbx::window_capacity(plan.slice / 16384 + 2)))) != RSI_OK) return rc;
  rsi_ctx::TrackWs& w = ctx->track;
  TrackBgzf z;
  if (bgzf) z.place(w.dev, L);
  char* d_text = static_cast<char*>(w.dev) + L.text;
  long long* d_starts = reinterpret_cast<long long*>(static_cast<char*>(w.dev) + L.starts);
  unsigned int* d_tiles = reinterpret_cast<unsigned int*>(static_cast<char*>(w.dev) + L.tiles);
  unsigned int* d_ltiles = reinterpret_cast<unsigned int*>(static_cast<char*>(w.dev) + L.ltiles);
  TrackState* d_st = reinterpret_cast<TrackState*>(static_cast<char*>(w.dev) + L.state);
  TrackState* h_st = static_cast<TrackState*>(w.pin_state);
  TrackName name;
  memset(&name, 0, sizeof(name));
  memcpy(name.s, chrom, (size_t)name_len);
  name.len = name_len;
  hipStream_t st = ctx->stream;

  h_st[1] = TrackState{-1, 0, 0, 0, 0, 0};
  const hipError_t e = hipMemcpyAsync(d_st, &h_st[1], sizeof(TrackState), hipMemcpyHostToDevice, st);
  if (e != hipSuccess) { (void)ctx_sync(ctx); return fail(ctx, RSI_ERR_HIP, std::string("track: hipMemcpyAsync: ") + hipGetErrorString(e)); }
  rc = track_slices(ctx, n, plan.slice, plan.text_cap, plan.max_line, d_st, d_text, sink, S, z, X,
      [&](int64_t b, int64_t end) {
        launch_track_starts(d_v, b, end, n, d_tiles, d_starts, d_st, st);
        launch_track_line_bytes(d_v, d_starts, d_st, pos0, name_len, end - b + 1, d_ltiles, st);
      },
      [](int64_t b, int64_t end) { return end - b + 1; },
      [&](int64_t, int64_t nlines) { launch_track_format(d_v, d_starts, d_ltiles, nlines, pos0, name, d_text, plan.text_cap, st); },
      // the lines a slice writes end in (b, end]: their last bases, which decide both record kinds, lie in [pos0 + b, pos0 + end)
      [&](int64_t b, int64_t end) { return rsitbx::windows_spanned(pos0 + b, pos0 + end); },
      [&](int64_t, int64_t nlines, int64_t nbytes, const TrackIndexOut& out) {
        launch_track_index(d_v, d_starts, d_ltiles, nlines, pos0, name_len, z.sizes, deflate_members(nbytes), out, st);
      });
  if (rc != RSI_OK) return rc;
  S.t_total_ms = now_ms() - t_begin;
  if (stats) *stats = S;
  ctx->last_deflate = z.D;
  return RSI_OK;
}

// the size of the sink's file as it was opened (appended to, or truncated): sink.base
bool sink_base(TrackSink& sink) {
  struct stat sb;
  if (::fstat(sink.fd, &sb) != 0) return false;
  sink.base = (int64_t)sb.st_size;
  return true;
}

int track_to_file(rsi_ctx* ctx, const int32_t* d_v, int64_t n, const char* chrom, const char* path, int append, rsi_track_stats* stats) {
  if (!path || !path[0]) return fail(ctx, RSI_ERR_BAD_ARG, "track: no path");
  if (rsitrack::name_length(chrom) < 0) return fail(ctx, RSI_ERR_BAD_ARG, "track: the name must have 1 to 255 bytes and no tab or newline");
  TrackSink sink;
  sink.fd = ::open(path, O_WRONLY | O_CREAT | (append ? O_APPEND : O_TRUNC), 0644);
  if (sink.fd < 0) return fail(ctx, RSI_ERR_INTERNAL, std::string("track: cannot open ") + path + ": " + strerror(errno));
  if (!sink_base(sink)) { const int err = errno; (void)::close(sink.fd); return fail(ctx, RSI_ERR_INTERNAL, std::string("track: cannot size ") + path + ": " + strerror(err)); }
  int rc = track_run(ctx, d_v, n, chrom, 0, 0, sink, stats);
  if (::close(sink.fd) != 0 && rc == RSI_OK) rc = fail(ctx, RSI_ERR_INTERNAL, std::string("track: write failed: ") + strerror(errno));
  return rc;
}

// values d_v[nb] of bins of m compacted bases as bedGraph lines of `chrom`, a line per piece of a bin, into the sink.  The table is
// rsitrack::bin_table's for a chromosome of n bases; which / median2: the value format (kernels.h, BinTrackSource).
int bin_track_run(rsi_ctx* ctx, const int32_t* d_v, int64_t nb, int m, int64_t n, const std::vector<int64_t>& cbreak,
                  const std::vector<int64_t>& cum, int64_t median2, int which, const char* chrom, int64_t slice_bins, TrackSink& sink,
                  rsi_track_stats* stats) {
  static_assert(rsitrack::kMaxBinRegions == kMaxRegions, "the bin track takes every chromosome the pipeline takes");
  const double t_begin = now_ms();
  rsi_track_stats S;
  memset(&S, 0, sizeof(S));
  if (stats) *stats = S;
  ctx->last_deflate = rsi_deflate_stats{};
  const bool bgzf = ctx->track_format == RSI_TRACK_BGZF;
  const int name_len = rsitrack::name_length(chrom);
  if (name_len < 0) return fail(ctx, RSI_ERR_BAD_ARG, "bin track: the name must have 1 to 255 bytes and no tab or newline");
  if (which != 0 && which != 1) return fail(ctx, RSI_ERR_BAD_ARG, "bin track: which must be 0 (bin median) or 1 (ratio to the chromosome's median)");
  if (which == 1 && median2 <= 0) return fail(ctx, RSI_ERR_BAD_ARG, "bin track: the chromosome's median is 0: no ratio");
  const int nreg = (int)cbreak.size();
  rsitrack::BinPlan plan;
  if (m < 1 || !rsitrack::bin_plan(name_len, n, nb, nreg, which, slice_bins, plan)) return fail(ctx, RSI_ERR_BAD_ARG, "bin track: bad bin count, bin size or region count");
  if (nb > (n - cum.back()) / m) return fail(ctx, RSI_ERR_BAD_ARG, "bin track: more bins than the kept bases hold");
  S.n = nb;
  TrackIndexer X;
  if (ctx->track_index) {
    const int rc = track_index_admit(ctx, bgzf, n);
    if (rc != RSI_OK) return rc;
    X.ix = ctx->track_index; X.name.assign(chrom, (size_t)name_len); X.base = sink.base;
  }
  // where the compacted position p lies on the chromosome (rsih::compact_table's rule, as the kernels')
  auto genomic = [&](int64_t p) { return p + cum[(size_t)(std::upper_bound(cbreak.begin(), cbreak.end(), p) - cbreak.begin())]; };
  // bins [b, end) hold slice_bins m kept bases and the removed regions between them: from the first one's base to the last one's
  auto bin_windows = [&](int64_t b, int64_t end) { return rsitbx::windows_spanned(genomic(b * m), genomic(end * m - 1) + 1); };
  if (nb == 0) { if (stats) *stats = S; return RSI_OK; }
  if (!d_v) return fail(ctx, RSI_ERR_BAD_ARG, "bin track: no values");
  HIPCHK(hipSetDevice(ctx->device));
  if (!ctx_enter(ctx)) return RSI_ERR_HIP;
  const TrackLayout L = track_layout(plan.text_cap, plan.max_pieces, plan.slice, plan.max_pieces, (size_t)2 * nreg + 1, bgzf);
  int rc = track_ensure(ctx, L);
  if (rc != RSI_OK) return rc;
  if (X.on()) {
    int64_t span = 0;
    for (int64_t b = 0; b < nb; b += plan.slice) span = std::max(span, bin_windows(b, std::min(nb, b + plan.slice)));
    if ((rc = track_index_ensure(ctx, track_index_bytes(rsitbx::chunk_capacity(span), rsitbx::window_capacity(span)))) != RSI_OK) return rc;
  }
  rsi_ctx::TrackWs& w = ctx->track;
  TrackBgzf z;
  if (bgzf) z.place(w.dev, L);
  char* d_text = static_cast<char*>(w.dev) + L.text;
  unsigned long long* d_pieces = reinterpret_cast<unsigned long long*>(static_cast<char*>(w.dev) + L.starts);
  unsigned int* d_tiles = reinterpret_cast<unsigned int*>(static_cast<char*>(w.dev) + L.tiles);
  unsigned int* d_ltiles = reinterpret_cast<unsigned int*>(static_cast<char*>(w.dev) + L.ltiles);
  TrackState* d_st = reinterpret_cast<TrackState*>(static_cast<char*>(w.dev) + L.state);
  long long* d_cbreak = reinterpret_cast<long long*>(static_cast<char*>(w.dev) + L.table);
  long long* d_cum = d_cbreak + nreg;
  TrackName name;
  memset(&name, 0, sizeof(name));
  memcpy(name.s, chrom, (size_t)name_len);
  name.len = name_len;
  hipStream_t st = ctx->stream;

  // the region table, once per call: cbreak[nreg] | cum[nreg + 1] (`table` outlives every wait of track_slices)
  std::vector<int64_t> table(cbreak);
  table.insert(table.end(), cum.begin(), cum.end());
  const hipError_t e = hipMemcpyAsync(d_cbreak, table.data(), table.size() * 8, hipMemcpyHostToDevice, st);
  if (e != hipSuccess) { (void)ctx_sync(ctx); return fail(ctx, RSI_ERR_HIP, std::string("bin track: hipMemcpyAsync: ") + hipGetErrorString(e)); }
  BinTrackSource src{d_v, d_pieces, d_cbreak, d_cum, nreg, m, 0, which, median2};
  rc = track_slices(ctx, nb, plan.slice, plan.text_cap, plan.max_line, d_st, d_text, sink, S, z, X,
      [&](int64_t b, int64_t end) {
        src.b0 = b;
        launch_bintrack_pieces(d_cbreak, d_cum, nreg, m, b, end, d_tiles, d_pieces, plan.max_pieces, d_st, st);
        launch_bintrack_line_bytes(src, d_st, name_len, end - b + nreg, d_ltiles, st);
      },
      [&](int64_t b, int64_t end) { return end - b + nreg; },
      [&](int64_t b, int64_t nlines) { src.b0 = b; launch_bintrack_format(src, d_ltiles, nlines, name, d_text, plan.text_cap, st); },
      bin_windows,
      [&](int64_t b, int64_t nlines, int64_t nbytes, const TrackIndexOut& out) {
        src.b0 = b;
        launch_bintrack_index(src, d_ltiles, nlines, name_len, z.sizes, deflate_members(nbytes), out, st);
      });
  if (rc != RSI_OK) return rc;
  S.t_total_ms = now_ms() - t_begin;
  if (stats) *stats = S;
  ctx->last_deflate = z.D;
  return RSI_OK;
}

// Region lines (`rsicnv depth -by`): a line "chrom start end mean" per (start, end, sum) triple into the sink, a
// slice of lines at a time.  W > 0: the windows of d_v[0, n), whose triples a slice's measuring passes make on the device
// (kernels_depth.hip; span: bases per workgroup of the sums).  W == 0: the host's triples, a slice's uploaded in front of its
// passes.  No state passes from slice to slice and nothing is indexed.  extra_launches: what the caller launched for the triples.
struct RegionTriples { std::vector<int64_t> start, end, sum; };
int region_track_run(rsi_ctx* ctx, const int32_t* d_v, int64_t n, int64_t W, int span, const RegionTriples* host, const char* chrom, int64_t pos0,
                     int64_t slice_lines, int64_t extra_launches, TrackSink& sink, rsi_track_stats* stats) {
  const double t_begin = now_ms();
  rsi_track_stats S;
  memset(&S, 0, sizeof(S));
  if (stats) *stats = S;
  ctx->last_deflate = rsi_deflate_stats{};
  ctx->depth.stats.launches = extra_launches;
  const bool bgzf = ctx->track_format == RSI_TRACK_BGZF;
  const int name_len = rsitrack::name_length(chrom);
  if (name_len < 0) return fail(ctx, RSI_ERR_BAD_ARG, "region track: the name must have 1 to 255 bytes and no tab or newline");
  if (pos0 < -(1ll << 62) || pos0 > (1ll << 62)) return fail(ctx, RSI_ERR_BAD_ARG, "region track: bad coordinate offset");
  if (W > 0 && n > 0) W = std::min(W, n);   // one window then, as for W = n
  const int64_t count = W > 0 ? rsidepth::window_count(n, W) : (int64_t)host->start.size();
  rsidepth::Plan plan;
  if (!rsidepth::plan(name_len, count, slice_lines, plan)) return fail(ctx, RSI_ERR_BAD_ARG, "region track: bad line count");
  S.n = count;
  if (count == 0) { if (stats) *stats = S; return RSI_OK; }
  if (W > 0 && (!d_v || span < 1 || span > kWindowSpan)) return fail(ctx, RSI_ERR_BAD_ARG, "region track: no values, or a span outside 1 .. 4096");
  HIPCHK(hipSetDevice(ctx->device));
  if (!ctx_enter(ctx)) return RSI_ERR_HIP;
  const TrackLayout L = track_layout(plan.text_cap, 0, 0, plan.slice, (size_t)3 * plan.slice, bgzf);
  int rc = track_ensure(ctx, L);
  if (rc != RSI_OK) return rc;
  rsi_ctx::TrackWs& w = ctx->track;
  TrackBgzf z;
  if (bgzf) z.place(w.dev, L);
  TrackIndexer X;   // off: these lines are not indexed
  char* d_text = static_cast<char*>(w.dev) + L.text;
  unsigned int* d_ltiles = reinterpret_cast<unsigned int*>(static_cast<char*>(w.dev) + L.ltiles);
  TrackState* d_st = reinterpret_cast<TrackState*>(static_cast<char*>(w.dev) + L.state);
  long long* d_start = reinterpret_cast<long long*>(static_cast<char*>(w.dev) + L.table);
  long long* d_end = d_start + plan.slice;
  long long* d_sum = d_end + plan.slice;
  const RegionTrackSource src{d_start, d_end, d_sum};
  TrackName name;
  memset(&name, 0, sizeof(name));
  memcpy(name.s, chrom, (size_t)name_len);
  name.len = name_len;
  hipStream_t st = ctx->stream;
  hipError_t up = hipSuccess;   // a slice's upload that failed: its line count is then out of range for nobody, so it is told here
  rc = track_slices(ctx, count, plan.slice, plan.text_cap, plan.max_line, d_st, d_text, sink, S, z, X,
      [&](int64_t b, int64_t end) {
        if (W > 0) {
          launch_depth_window_table(b, end, W, n, d_start, d_end, reinterpret_cast<unsigned long long*>(d_sum), st);
          launch_depth_windows(d_v, n, W, b, end, span, reinterpret_cast<unsigned long long*>(d_sum), st);
        } else {
          const size_t bytes = (size_t)(end - b) * 8;
          for (auto pr : {std::make_pair(d_start, &host->start), std::make_pair(d_end, &host->end), std::make_pair(d_sum, &host->sum)}) {
            const hipError_t e = hipMemcpyAsync(pr.first, pr.second->data() + b, bytes, hipMemcpyHostToDevice, st);
            if (e != hipSuccess && up == hipSuccess) up = e;
          }
        }
        launch_regiontrack_line_bytes(src, d_st, end - b, pos0, name_len, d_ltiles, st);
      },
      [](int64_t b, int64_t end) { return end - b; },
      [&](int64_t, int64_t nlines) { launch_regiontrack_format(src, d_ltiles, nlines, pos0, name, d_text, plan.text_cap, st); },
      [](int64_t, int64_t) { return (int64_t)0; },
      [](int64_t, int64_t, int64_t, const TrackIndexOut&) {});
  if (rc == RSI_OK && up != hipSuccess) rc = fail(ctx, RSI_ERR_HIP, std::string("region track: hipMemcpyAsync: ") + hipGetErrorString(up));
  if (rc != RSI_OK) return rc;
  // per slice: (the window table and sums,) the state, the line lengths, their scan, the format pass(, deflate and pack)
  ctx->depth.stats.launches = extra_launches + S.slices * ((W > 0 ? 2 : 0) + 4 + (bgzf ? 2 : 0));
  S.t_total_ms = now_ms() - t_begin;
  if (stats) *stats = S;
  ctx->last_deflate = z.D;
  return RSI_OK;
}

// The triples of explicit regions: summed on the device (depth.hip), written with their clipped coordinates -- or, with nothing
// left of them, with the ones given and a sum of 0
int region_triples(rsi_ctx* ctx, const int32_t* d_v, int64_t n, int nreg, const int64_t* start, const int64_t* end, int tile, RegionTriples& T) {
  for (int i = 0; i < nreg; ++i)
    if (start[i] < -(1ll << 62) || start[i] > (1ll << 62) || end[i] < -(1ll << 62) || end[i] > (1ll << 62))
      return fail(ctx, RSI_ERR_BAD_ARG, "region track: a coordinate beyond 2^62");
  std::vector<rsi_depth_region> rec((size_t)std::max(nreg, 1));
  HIPCHK(hipSetDevice(ctx->device));
  if (!ctx_enter(ctx)) return RSI_ERR_HIP;
  mailbox_reset(ctx);
  const int rc = depth_region_records(ctx, d_v, n, nreg, start, end, tile, rec.data());
  if (rc != RSI_OK) return rc;
  T.start.resize((size_t)nreg); T.end.resize((size_t)nreg); T.sum.resize((size_t)nreg);
  for (int i = 0; i < nreg; ++i) {
    rsidepth::written(start[i], end[i], n, T.start[(size_t)i], T.end[(size_t)i]);
    T.sum[(size_t)i] = rec[(size_t)i].sum;
  }
  return RSI_OK;
}

// windows (W > 0) or regions of d_v[0, n) into `path`
int region_track_to_file(rsi_ctx* ctx, const int32_t* d_v, int64_t n, const char* chrom, int64_t W, int nreg, const int64_t* start,
                         const int64_t* end, const char* path, int append, rsi_track_stats* stats) {
  if (!ctx) return fail(ctx, RSI_ERR_BAD_ARG, "null context");
  if (n < 0 || n >= (1ll << 31) || (n > 0 && !d_v)) return fail(ctx, RSI_ERR_BAD_ARG, "region track: bad array");
  if (!path || !path[0]) return fail(ctx, RSI_ERR_BAD_ARG, "region track: no path");
  if (rsitrack::name_length(chrom) < 0) return fail(ctx, RSI_ERR_BAD_ARG, "region track: the name must have 1 to 255 bytes and no tab or newline");
  RegionTriples T;
  if (W <= 0) { const int rc = region_triples(ctx, d_v, n, nreg, start, end, 0, T); if (rc != RSI_OK) return rc; }
  TrackSink sink;
  sink.fd = ::open(path, O_WRONLY | O_CREAT | (append ? O_APPEND : O_TRUNC), 0644);
  if (sink.fd < 0) return fail(ctx, RSI_ERR_INTERNAL, std::string("region track: cannot open ") + path + ": " + strerror(errno));
  int rc = region_track_run(ctx, d_v, n, W, kWindowSpan, W > 0 ? nullptr : &T, chrom, 0, 0, W > 0 ? 0 : ctx->depth.stats.launches, sink, stats);
  if (::close(sink.fd) != 0 && rc == RSI_OK) rc = fail(ctx, RSI_ERR_INTERNAL, std::string("region track: write failed: ") + strerror(errno));
  return rc;
}

}  // namespace

extern "C" {

int rsi_hot_write_window_track(rsi_ctx* ctx, const void* d_depth, int64_t n, const char* chrom, int64_t W, const char* path, int append,
                               rsi_track_stats* stats) {
  if (W < 1) return fail(ctx, RSI_ERR_BAD_ARG, "window track: the window must have at least one base");
  return region_track_to_file(ctx, static_cast<const int32_t*>(d_depth), n, chrom, W, 0, nullptr, nullptr, path, append, stats);
}

int rsi_hot_write_region_track(rsi_ctx* ctx, const void* d_depth, int64_t n, const char* chrom, int nreg, const int64_t* start,
                               const int64_t* end, const char* path, int append, rsi_track_stats* stats) {
  if (nreg < 0 || (nreg > 0 && (!start || !end))) return fail(ctx, RSI_ERR_BAD_ARG, "region track: bad region list");
  return region_track_to_file(ctx, static_cast<const int32_t*>(d_depth), n, chrom, 0, nreg, start, end, path, append, stats);
}

int64_t rsi_hot_debug_region_track(rsi_ctx* ctx, const int32_t* values, int64_t n, const char* chrom, int64_t W, int nreg, const int64_t* start,
                                   const int64_t* end, int span, int tile, int64_t slice_lines, int64_t pos0, char* out, int64_t cap,
                                   rsi_track_stats* stats) {
  if (!ctx) return fail(ctx, RSI_ERR_BAD_ARG, "null context");
  if (n < 0 || n >= (1ll << 31) - 4096 || (n > 0 && !values) || W < 0 || span < 0 || tile < 0 || slice_lines < 0 || nreg < 0 ||
      (W == 0 && nreg > 0 && (!start || !end)))
    return fail(ctx, RSI_ERR_BAD_ARG, "region track: bad argument");
  if (int rc = depth_upload(ctx, values, n)) return rc;
  RegionTriples T;
  if (W == 0) { const int rc = region_triples(ctx, ctx->in_depth.as<int32_t>(), n, nreg, start, end, tile, T); if (rc != RSI_OK) return rc; }
  std::string text;
  TrackSink sink;
  sink.text = &text;
  const int rc = region_track_run(ctx, ctx->in_depth.as<int32_t>(), n, W, span > 0 ? span : kWindowSpan, W > 0 ? nullptr : &T, chrom, pos0,
                                  slice_lines, W > 0 ? 0 : ctx->depth.stats.launches, sink, stats);
  if (rc != RSI_OK) return rc;
  if (out && (int64_t)text.size() <= cap) memcpy(out, text.data(), text.size());
  return (int64_t)text.size();
}


int rsi_hot_write_track(rsi_ctx* ctx, int which, const char* chrom, const char* path, int append, rsi_track_stats* stats) {
  if (!ctx) return fail(ctx, RSI_ERR_BAD_ARG, "null context");
  if (which != 0 && which != 1) return fail(ctx, RSI_ERR_BAD_ARG, "track: which must be 0 (raw depth) or 1 (GC-adjusted depth)");
  if (!ctx->last_depth || ctx->n <= 0) return fail(ctx, RSI_ERR_BAD_ARG, "track: this context has run no chromosome");
  const int32_t* d_v = ctx->last_depth;
  if (which == 1) {
    HIPCHK(hipSetDevice(ctx->device));
    if (!ctx_enter(ctx)) return RSI_ERR_HIP;
    const int rc = ensure_rd_gc(ctx);   // RSI_ERR_BAD_ARG after a -NOGC run
    if (rc != RSI_OK) return rc;
    d_v = ctx->rd_gc.as<int32_t>();
  }
  return track_to_file(ctx, d_v, ctx->n, chrom, path, append, stats);
}

int rsi_hot_write_track_device(rsi_ctx* ctx, const void* d_values, int64_t n, const char* chrom, const char* path, int append,
                               rsi_track_stats* stats) {
  if (!ctx) return fail(ctx, RSI_ERR_BAD_ARG, "null context");
  if (n < 0 || (n > 0 && !d_values)) return fail(ctx, RSI_ERR_BAD_ARG, "track: bad array");
  return track_to_file(ctx, static_cast<const int32_t*>(d_values), n, chrom, path, append, stats);
}

int64_t rsi_hot_debug_track(rsi_ctx* ctx, const int32_t* values, int64_t n, const char* chrom, int64_t pos0, int64_t slice_bases, char* out,
                            int64_t cap, rsi_track_stats* stats) {
  if (!ctx) return fail(ctx, RSI_ERR_BAD_ARG, "null context");
  if (n < 0 || (n > 0 && !values) || slice_bases < 0) return fail(ctx, RSI_ERR_BAD_ARG, "track: bad argument");
  if (n > 0) {
    HIPCHK(hipSetDevice(ctx->device));
    if (!ctx_enter(ctx)) return RSI_ERR_HIP;
    if (ctx->last_depth == ctx->in_depth.p) ctx->last_depth = nullptr;   // the last run's depth is about to be overwritten
    HIPCHK(ctx->in_depth.ensure((size_t)(n + 4) * 4));
    ctx->n_in = n;
    HIPCHK(hipMemcpyAsync(ctx->in_depth.p, values, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(CTX_SYNC());   // the caller's array is pageable: free again once this returns
  }
  std::string text;
  TrackSink sink;
  sink.text = &text;
  const int rc = track_run(ctx, ctx->in_depth.as<int32_t>(), n, chrom, pos0, slice_bases, sink, stats);
  if (rc != RSI_OK) return rc;
  if (out && (int64_t)text.size() <= cap) memcpy(out, text.data(), text.size());
  return (int64_t)text.size();
}

int rsi_hot_write_bin_track(rsi_ctx* ctx, int which, const char* chrom, const char* path, int append, rsi_track_stats* stats) {
  if (!ctx) return fail(ctx, RSI_ERR_BAD_ARG, "null context");
  if (which != 0 && which != 1) return fail(ctx, RSI_ERR_BAD_ARG, "bin track: which must be 0 (bin median) or 1 (ratio to the chromosome's median)");
  if (ctx->run_m <= 0) return fail(ctx, RSI_ERR_BAD_ARG, "bin track: this context holds no successful run");
  if (!path || !path[0]) return fail(ctx, RSI_ERR_BAD_ARG, "bin track: no path");
  if (rsitrack::name_length(chrom) < 0) return fail(ctx, RSI_ERR_BAD_ARG, "bin track: the name must have 1 to 255 bytes and no tab or newline");
  int64_t median2 = 0, ncompact = 0;
  if (!rsitrack::twice_median(ctx->run_rdmedian, median2)) return fail(ctx, RSI_ERR_INTERNAL, "bin track: the chromosome's median is no multiple of 0.5");
  if (which == 1 && median2 == 0) return fail(ctx, RSI_ERR_BAD_ARG, "bin track: the chromosome's median is 0: no ratio");
  std::vector<int64_t> cbreak, cum;
  if (!rsitrack::bin_table(ctx->noncode_pairs.data(), (int)(ctx->noncode_pairs.size() / 2), ctx->n, cbreak, cum, ncompact) || ncompact != ctx->ncompact)
    return fail(ctx, RSI_ERR_INTERNAL, "bin track: the run's removed regions do not give its compacted length");
  TrackSink sink;
  sink.fd = ::open(path, O_WRONLY | O_CREAT | (append ? O_APPEND : O_TRUNC), 0644);
  if (sink.fd < 0) return fail(ctx, RSI_ERR_INTERNAL, std::string("bin track: cannot open ") + path + ": " + strerror(errno));
  if (!sink_base(sink)) { const int err = errno; (void)::close(sink.fd); return fail(ctx, RSI_ERR_INTERNAL, std::string("bin track: cannot size ") + path + ": " + strerror(err)); }
  int rc = bin_track_run(ctx, ctx->binmed.as<int32_t>(), ctx->nb, ctx->run_m, ctx->n, cbreak, cum, median2, which, chrom, 0, sink, stats);
  if (::close(sink.fd) != 0 && rc == RSI_OK) rc = fail(ctx, RSI_ERR_INTERNAL, std::string("bin track: write failed: ") + strerror(errno));
  return rc;
}

int64_t rsi_hot_debug_bin_track(rsi_ctx* ctx, const int32_t* values, int64_t nb, int m, int64_t n, const int32_t* pairs, int npairs,
                                int64_t median2, int which, const char* chrom, int64_t slice_bins, char* out, int64_t cap,
                                rsi_track_stats* stats) {
  if (!ctx) return fail(ctx, RSI_ERR_BAD_ARG, "null context");
  if (nb < 0 || nb >= (1ll << 31) || (nb > 0 && !values) || m < 1 || n < 0 || slice_bins < 0 || median2 < 0 || median2 > (1ll << 33))
    return fail(ctx, RSI_ERR_BAD_ARG, "bin track: bad argument");
  if (npairs < 0 || npairs > kMaxRegions) return fail(ctx, RSI_ERR_BAD_ARG, "bin track: more than 4096 regions");
  std::vector<int64_t> cbreak, cum;
  int64_t ncompact = 0;
  if (!rsitrack::bin_table(pairs, npairs, n, cbreak, cum, ncompact))
    return fail(ctx, RSI_ERR_BAD_ARG, "bin track: regions must be sorted, inside [0, n) and apart by at least one kept base");
  if (nb > 0) {
    HIPCHK(hipSetDevice(ctx->device));
    if (!ctx_enter(ctx)) return RSI_ERR_HIP;
    ctx->run_m = 0;   // the last run's bin medians are about to be overwritten
    ctx->nb = 0;
    HIPCHK(ctx->binmed.ensure((size_t)nb * 4));
    HIPCHK(hipMemcpyAsync(ctx->binmed.p, values, (size_t)nb * 4, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(CTX_SYNC());   // the caller's array is pageable: free again once this returns
    ctx->nb = nb;
  }
  std::string text;
  TrackSink sink;
  sink.text = &text;
  const int rc = bin_track_run(ctx, ctx->binmed.as<int32_t>(), nb, m, n, cbreak, cum, median2, which, chrom, slice_bins, sink, stats);
  if (rc != RSI_OK) return rc;
  if (out && (int64_t)text.size() <= cap) memcpy(out, text.data(), text.size());
  return (int64_t)text.size();
}

int rsi_hot_set_track_format(rsi_ctx* ctx, int format) {
  if (!ctx) return fail(ctx, RSI_ERR_BAD_ARG, "null context");
  if (format != RSI_TRACK_TEXT && format != RSI_TRACK_BGZF) return fail(ctx, RSI_ERR_BAD_ARG, "track: the format must be RSI_TRACK_TEXT (0) or RSI_TRACK_BGZF (1)");
  ctx->track_format = format;
  return RSI_OK;
}

int rsi_hot_set_track_index(rsi_ctx* ctx, rsi_track_index* ix) {
  if (!ctx) return fail(ctx, RSI_ERR_BAD_ARG, "null context");
  ctx->track_index = ix;
  return RSI_OK;
}

rsi_track_index* rsi_track_index_create(void) { return new (std::nothrow) rsi_track_index(); }
void rsi_track_index_free(rsi_track_index* ix) { delete ix; }

int rsi_track_index_append(rsi_track_index* dst, const rsi_track_index* src, int64_t shift) {
  if (!dst || !src || dst == src) return fail(nullptr, RSI_ERR_BAD_ARG, "track index: two different indexes are needed");
  if (dst->append(*src, shift) != rsitbx::kOk) return fail(nullptr, RSI_ERR_BAD_ARG, dst->err);
  return RSI_OK;
}

int rsi_track_index_write_tbi(rsi_track_index* ix, const char* path) {
  if (!ix || !path || !path[0]) return fail(nullptr, RSI_ERR_BAD_ARG, "track index: no index or no path");
  if (!ix->write_tbi(path)) return fail(nullptr, RSI_ERR_INTERNAL, ix->err);
  return RSI_OK;
}

int rsi_track_index_counts(const rsi_track_index* ix, int64_t* nref, int64_t* nchunks, int64_t* nwindows) {
  if (!ix) return fail(nullptr, RSI_ERR_BAD_ARG, "track index: no index");
  int64_t r, c, w;
  ix->counts(r, c, w);
  if (nref) *nref = r;
  if (nchunks) *nchunks = c;
  if (nwindows) *nwindows = w;
  return RSI_OK;
}

int64_t rsi_track_index_debug_tbi(const rsi_track_index* ix, uint8_t* out, int64_t cap) {
  if (!ix) return fail(nullptr, RSI_ERR_BAD_ARG, "track index: no index");
  const std::string raw = ix->tbi();
  if (out && (int64_t)raw.size() <= cap) memcpy(out, raw.data(), raw.size());
  return (int64_t)raw.size();
}

int rsi_hot_last_deflate_stats(const rsi_ctx* ctx, rsi_deflate_stats* out) {
  if (!ctx || !out) return RSI_ERR_BAD_ARG;
  *out = ctx->last_deflate;
  return RSI_OK;
}

int rsi_bgzf_write_eof(const char* path) {
  if (!path || !path[0]) return fail(nullptr, RSI_ERR_BAD_ARG, "bgzf: no path");
  if (!rsitrack::append_bgzf_eof(path)) return fail(nullptr, RSI_ERR_INTERNAL, std::string("bgzf: cannot write ") + path + ": " + strerror(errno));
  return RSI_OK;
}

int64_t rsi_hot_debug_deflate(rsi_ctx* ctx, const uint8_t* text, int64_t len, uint8_t* out, int64_t cap, rsi_deflate_stats* stats) {
  if (!ctx) return fail(ctx, RSI_ERR_BAD_ARG, "null context");
  rsi_deflate_stats D{};
  if (stats) *stats = D;
  ctx->last_deflate = D;
  if (len < 0 || (len > 0 && !text)) return fail(ctx, RSI_ERR_BAD_ARG, "deflate: bad argument");
  if (len == 0) return 0;
  HIPCHK(hipSetDevice(ctx->device));
  if (!ctx_enter(ctx)) return RSI_ERR_HIP;
  // the track workspace of a slice of text, filled from the caller's bytes instead of a format pass; whole members but the last
  const int64_t chunk = std::min(len, rsitrack::kTextBytes / rsitrack::kMemberText * rsitrack::kMemberText);
  const TrackLayout L = track_layout(chunk, 0, 0, 0, 0, true);
  const int rc = track_ensure(ctx, L);
  if (rc != RSI_OK) return rc;
  rsi_ctx::TrackWs& w = ctx->track;
  TrackBgzf z;
  z.place(w.dev, L);
  char* d_text = static_cast<char*>(w.dev) + L.text;
  TrackState* d_st = reinterpret_cast<TrackState*>(static_cast<char*>(w.dev) + L.state);
  TrackState* h_st = static_cast<TrackState*>(w.pin_state);
  hipStream_t st = ctx->stream;
  std::string file;
  for (int64_t off = 0; off < len; off += chunk) {
    const int64_t nbytes = std::min(chunk, len - off);
    const int64_t members = rsitrack::members_of(nbytes);
    HIPCHK(hipMemcpyAsync(d_text, text + off, (size_t)nbytes, hipMemcpyHostToDevice, st));
    (void)hipEventRecord(w.ev[kEvF1], st);
    launch_deflate_bgzf(d_text, nbytes, z.slots, z.sizes, st);
    launch_bgzf_pack(z.slots, z.sizes, deflate_members(nbytes), z.packed, z.packed_cap, d_st, st);
    (void)hipEventRecord(w.ev[kEvD1], st);
    HIPCHK(hipMemcpyAsync(&h_st[0], d_st, sizeof(TrackState), hipMemcpyDeviceToHost, st));
    HIPCHK(CTX_SYNC());
    const int64_t bytes = h_st[0].packed, stored = h_st[0].stored;
    if (bytes <= 0 || bytes > nbytes + members * rsitrack::kMemberOverhead || stored < 0 || stored > members)
      return fail(ctx, RSI_ERR_INTERNAL, "deflate: a compressed size is out of range");
    HIPCHK(hipMemcpyAsync(w.pin[0], z.packed, (size_t)bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(CTX_SYNC());
    file.append(w.pin[0], (size_t)bytes);
    D.t_kernel_ms += elapsed_ms(w.ev[kEvF1], w.ev[kEvD1]);
    D.members += members;
    D.stored_members += stored;
    D.text_bytes += nbytes;
    D.file_bytes += bytes;
  }
  if (stats) *stats = D;
  ctx->last_deflate = D;
  if (out && (int64_t)file.size() <= cap) memcpy(out, file.data(), file.size());
  return (int64_t)file.size();
}

}  // extern "C"
