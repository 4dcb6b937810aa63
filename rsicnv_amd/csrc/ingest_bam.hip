// ingest_bam.hip -- the depth of one chromosome from a BAM (the pileup loop, samfunctions.cpp), built in
// HBM: BGZF inflation and record walk on host threads (bam_host.cpp) or, in rsi_hot_set_bam_read's device mode, on the device
// (bgzf_launch.h, kernels_bam.hip); the pileup and the difference-array scan are kernels (kernels_io.hip).  An
// armed load also keeps the pair table (RP / Q0 with no second pass) and the CIGARs (`stat` and `pin`, 6m); their
// entry points and debug hooks are here too.
#include "ingest_internal.h"
#include "inflate_core.h"
#include "bam_pairs_core.h"
#include "bam_pin_core.h"
#include "pin_host.h"

using namespace rsik;
using namespace rsip;
using namespace rsing;

namespace {

// ---- the pair table of an armed BAM load and what is computed from it ----
constexpr size_t kTableFirstCap = size_t(1) << 20;   // entries of the first allocation of the pair table (20 MB), of the pin table and of its pool; doubled when one fills up

PairTable pair_table(const rsi_ctx* ctx) {
  int32_t* b = ctx->pairs.tab.as<int32_t>();
  const size_t c = ctx->pairs.cap;
  return PairTable{b, b + c, b + 2 * c, b + 3 * c, reinterpret_cast<uint32_t*>(b + 4 * c)};
}
// Room for `need` entries: a larger table takes over the entries written so far, copied on the stream.
int pairs_reserve(rsi_ctx* ctx, size_t need) {
  rsi_ctx::Pairs& P = ctx->pairs;
  if (need <= P.cap) return RSI_OK;
  const size_t cap = std::max(need, P.cap ? 2 * P.cap : kTableFirstCap);
  DevBuf grown;
  HIPCHK(grown.ensure(cap * 20));
  for (int k = 0; k < 5 && P.n > 0; ++k)
    HIPCHK(hipMemcpyAsync(grown.as<int32_t>() + (size_t)k * cap, P.tab.as<int32_t>() + (size_t)k * P.cap, (size_t)P.n * 4, hipMemcpyDeviceToDevice, ctx->stream));
  if (P.tab.p) HIPCHK(hipStreamSynchronize(ctx->stream));    // the old table is freed below: nothing may still read or write it
  std::swap(P.tab.p, grown.p); std::swap(P.tab.cap, grown.cap);
  P.cap = cap;
  return RSI_OK;
}
hipEvent_t pairs_event(rsi_ctx* ctx) {
  rsi_ctx::Pairs& P = ctx->pairs;
  if (P.ev_next == P.events.size()) { hipEvent_t e = nullptr; (void)hipEventCreate(&e); P.events.push_back(e); }
  return P.events[P.ev_next++];
}
double pairs_elapsed(rsi_ctx* ctx, size_t first, size_t last) {   // summed time of the event pairs [first, last)
  double sum = 0;
  for (size_t k = first; k + 1 < last && k + 1 < ctx->pairs.events.size(); k += 2) sum += elapsed_ms(ctx->pairs.events[k], ctx->pairs.events[k + 1]);
  return sum;
}
// An armed load begins: an empty table, the words cleared, no predecessor.
int pairs_begin(rsi_ctx* ctx) {
  rsi_ctx::Pairs& P = ctx->pairs;
  P.n = 0; P.parity = 0; P.ev_next = 0; P.maxspan = 0; P.flags = 0;
  P.stats = rsi_pairs_stats{};
  if (int rc = pairs_reserve(ctx, 1)) return rc;
  HIPCHK(P.words.ensure(64));
  const int32_t init[kPairWords] = {0, 0, INT32_MIN, INT32_MIN};
  HIPCHK(copy_h2d(ctx, P.words.p, init, sizeof(init)));
  return RSI_OK;
}
// Beside a chunk's launch_bam_depth, same arguments: its records appended to the table.
int pairs_append(rsi_ctx* ctx, const void* data, const uint32_t* rec_off, int nrec, int tid) {
  rsi_ctx::Pairs& P = ctx->pairs;
  if (nrec <= 0) return RSI_OK;
  if (int rc = pairs_reserve(ctx, (size_t)P.n + (size_t)nrec)) return rc;
  const hipEvent_t a = pairs_event(ctx), b = pairs_event(ctx);
  HIPCHK(hipEventRecord(a, ctx->stream));
  launch_bam_pairs(data, rec_off, nrec, tid, (long long)P.n, pair_table(ctx), P.words.as<int32_t>(), P.parity, ctx->stream);
  HIPCHK(hipEventRecord(b, ctx->stream));
  P.n += nrec;
  P.parity ^= 1;
  return RSI_OK;
}
// Behind the load's last wait: the two reduced words are on the host (w), the table stands.
void pairs_end(rsi_ctx* ctx, const int32_t* w, int tid, int64_t tid_len) {
  rsi_ctx::Pairs& P = ctx->pairs;
  P.maxspan = w[0]; P.flags = (uint32_t)w[1];
  P.tid = tid; P.tid_len = tid_len;
  P.valid = true;
  P.stats.records = P.n; P.stats.table_bytes = P.n * 20; P.stats.maxspan = P.maxspan;
  P.stats.t_table_ms = pairs_elapsed(ctx, 0, P.ev_next);
}

// The insert-size sample over table[0, n): out = count, sum |isize|, sum of wrapped squares, S.
int pairs_sample(rsi_ctx* ctx, PairTable t, int64_t n, int64_t tid_len, int64_t out[4]) {
  rsi_ctx::Pairs& P = ctx->pairs;
  HIPCHK(P.ws.ensure(pair_sample_workspace_bytes((long long)n)));
  unsigned long long* d_out = reinterpret_cast<unsigned long long*>(P.ws.as<char>() + 64);   // inside the workspace's 256-byte head
  const size_t e0 = P.ev_next;
  const hipEvent_t a = pairs_event(ctx), b = pairs_event(ctx);
  HIPCHK(hipEventRecord(a, ctx->stream));
  launch_pair_sample(t, (long long)n, (long long)tid_len, P.ws.p, d_out, ctx->stream);
  HIPCHK(hipEventRecord(b, ctx->stream));
  unsigned long long h[4];
  HIPCHK(copy_d2h(ctx, h, d_out, sizeof(h)));
  HIPCHK(CTX_SYNC());
  out[0] = (int64_t)h[0]; out[1] = (int64_t)h[1]; out[2] = (int64_t)h[2]; out[3] = (int64_t)h[3] - 1;
  P.stats.sample_count = out[0]; P.stats.sample_abs = out[1]; P.stats.sample_sq = out[2]; P.stats.sample_stop = out[3];
  P.stats.t_sample_ms = pairs_elapsed(ctx, e0, e0 + 2);
  P.ev_next = e0;
  return RSI_OK;
}
// isize and isize_sd from the sums, with the very expressions of bam_pair_sample (bam_host.cpp): the integer sums are its
// double sums wherever those are exact (|sum| < 2^53).
rsih::PairSample pairs_sample_result(const int64_t sums[4]) {
  rsih::PairSample out;
  double isize = (double)sums[1];
  const double isize2 = (double)sums[2], isize_c = (double)sums[0];
  if (isize_c > 2) {
    isize /= isize_c;
    const double sd = sqrt((isize2 - isize_c * isize * isize) / isize_c);
    out.isize = (int)isize;
    out.isize_sd = (int)sd;
  }
  return out;
}
// The counts of the calls over table[0, n), ascending in pos: counts[4 * i ...] = q0_all, q0_q0, rp, entries examined.
int pairs_annotate(rsi_ctx* ctx, PairTable t, int64_t n, int maxspan, const std::vector<rsipairs::Call>& calls, int isize_mean, int isize_sd,
                   std::vector<uint32_t>& counts) {
  rsi_ctx::Pairs& P = ctx->pairs;
  counts.assign(calls.size() * 4, 0);
  P.stats.calls = (int64_t)calls.size(); P.stats.examined = 0; P.stats.t_annotate_ms = 0;
  if (calls.empty()) return RSI_OK;
  HIPCHK(P.calls.ensure(calls.size() * sizeof(rsipairs::Call)));
  HIPCHK(P.out.ensure(counts.size() * 4));
  HIPCHK(copy_h2d(ctx, P.calls.p, calls.data(), calls.size() * sizeof(rsipairs::Call)));
  const size_t e0 = P.ev_next;
  const hipEvent_t a = pairs_event(ctx), b = pairs_event(ctx);
  HIPCHK(hipEventRecord(a, ctx->stream));
  launch_pairs_annotate(t, (long long)n, maxspan, P.calls.p, (int)calls.size(), isize_mean, isize_sd, P.out.as<uint32_t>(), ctx->stream);
  HIPCHK(hipEventRecord(b, ctx->stream));
  HIPCHK(copy_d2h(ctx, counts.data(), P.out.p, counts.size() * 4));
  HIPCHK(CTX_SYNC());
  for (size_t i = 0; i < calls.size(); ++i) P.stats.examined += counts[4 * i + 3];
  P.stats.t_annotate_ms = pairs_elapsed(ctx, e0, e0 + 2);
  P.ev_next = e0;
  return RSI_OK;
}
// A caller's table in place of a BAM's (the debug hooks): whatever the context held is dropped.
int pairs_upload(rsi_ctx* ctx, int64_t n, const int32_t* const arrays[5]) {
  rsi_ctx::Pairs& P = ctx->pairs;
  P.valid = false; P.n = 0;
  P.stats = rsi_pairs_stats{};
  if (int rc = pairs_reserve(ctx, (size_t)std::max<int64_t>(n, 1))) return rc;
  for (int k = 0; k < 5 && n > 0; ++k)
    HIPCHK(hipMemcpyAsync(P.tab.as<int32_t>() + (size_t)k * P.cap, arrays[k], (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return RSI_OK;
}

// ---- the kept CIGARs of a load armed for `pin`, and what is computed from them ----
PinTable pin_table(const rsi_ctx* ctx) {
  int32_t* b = ctx->pin.tab.as<int32_t>();
  return PinTable{b, reinterpret_cast<uint32_t*>(b + ctx->pin.cap), ctx->pin.pool.as<uint32_t>()};
}
// Room for `need` reads and `pool_need` pool words: larger buffers take over what is written so far, copied on the stream.
int pin_reserve(rsi_ctx* ctx, size_t need, size_t pool_need) {
  rsi_ctx::Pin& Q = ctx->pin;
  if (need > Q.cap) {
    const size_t cap = std::max(need, Q.cap ? 2 * Q.cap : kTableFirstCap);
    DevBuf grown;
    HIPCHK(grown.ensure(cap * 8));
    for (int k = 0; k < 2 && Q.n > 0; ++k)
      HIPCHK(hipMemcpyAsync(grown.as<int32_t>() + (size_t)k * cap, Q.tab.as<int32_t>() + (size_t)k * Q.cap, (size_t)Q.n * 4, hipMemcpyDeviceToDevice, ctx->stream));
    if (Q.tab.p) HIPCHK(hipStreamSynchronize(ctx->stream));
    std::swap(Q.tab.p, grown.p); std::swap(Q.tab.cap, grown.cap);
    Q.cap = cap;
  }
  if (pool_need > Q.pool_cap) {
    const size_t cap = std::max(pool_need, Q.pool_cap ? 2 * Q.pool_cap : kTableFirstCap);
    if (cap >= (size_t(1) << 32)) return fail(ctx, RSI_ERR_UNSUPPORTED, "the CIGARs of this chromosome's reads take more than 2^32 words");
    DevBuf grown;
    HIPCHK(grown.ensure(cap * 4));
    if (Q.pool.p) {
      HIPCHK(hipMemcpyAsync(grown.p, Q.pool.p, (size_t)Q.cursor_h * 4, hipMemcpyDeviceToDevice, ctx->stream));
      HIPCHK(hipStreamSynchronize(ctx->stream));
    }
    std::swap(Q.pool.p, grown.p); std::swap(Q.pool.cap, grown.cap);
    Q.pool_cap = cap;
  }
  return RSI_OK;
}
// the cursor of the launches so far, on the host (waits for them)
int pin_read_cursor(rsi_ctx* ctx) {
  rsi_ctx::Pin& Q = ctx->pin;
  if (!Q.launched) return RSI_OK;
  uint32_t c = 0;
  HIPCHK(hipMemcpyAsync(&c, Q.cursor.p, 4, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  Q.t_table_ms += elapsed_ms(Q.ev[0], Q.ev[1]);
  if ((size_t)c > Q.pool_cap) return fail(ctx, RSI_ERR_INTERNAL, "the CIGAR pool was sized too small for a chunk");
  Q.cursor_h = c;
  Q.launched = false;
  return RSI_OK;
}
// the pool begins with one word 0, the empty CIGAR; the cursor stands behind it
int pin_reset(rsi_ctx* ctx) {
  rsi_ctx::Pin& Q = ctx->pin;
  Q.valid = Q.sampled = Q.launched = false; Q.n = 0; Q.cursor_h = 1; Q.t_table_ms = 0;
  Q.stats = rsi_pin_stats{};
  for (hipEvent_t& e : Q.ev) if (!e) HIPCHK(hipEventCreate(&e));
  if (int rc = pin_reserve(ctx, 1, 1)) return rc;
  HIPCHK(Q.cursor.ensure(64));
  const uint32_t one = 1, zero = 0;
  HIPCHK(copy_h2d(ctx, Q.cursor.p, &one, 4));
  HIPCHK(copy_h2d(ctx, Q.pool.p, &zero, 4));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return RSI_OK;
}
// Beside a chunk's pairs_append: the chunk's `bytes` bound its CIGAR words (4 n_cigar <= block_size of every record read).
int pin_append(rsi_ctx* ctx, const void* data, const uint32_t* rec_off, int nrec, size_t bytes) {
  rsi_ctx::Pin& Q = ctx->pin;
  if (nrec <= 0) return RSI_OK;
  if (int rc = pin_read_cursor(ctx)) return rc;
  if (int rc = pin_reserve(ctx, (size_t)Q.n + (size_t)nrec, (size_t)Q.cursor_h + (size_t)nrec + bytes / 4 + 1)) return rc;
  HIPCHK(hipEventRecord(Q.ev[0], ctx->stream));
  launch_bam_pin(data, rec_off, nrec, (long long)Q.n, pin_table(ctx), Q.cursor.as<unsigned int>(), (unsigned int)Q.pool_cap, ctx->stream);
  HIPCHK(hipEventRecord(Q.ev[1], ctx->stream));
  Q.n += nrec;
  Q.launched = true;
  return RSI_OK;
}
int pin_end(rsi_ctx* ctx) {
  rsi_ctx::Pin& Q = ctx->pin;
  if (int rc = pin_read_cursor(ctx)) return rc;
  Q.valid = true;
  Q.stats.records = Q.n; Q.stats.pool_words = Q.cursor_h; Q.stats.table_bytes = Q.n * 8 + (int64_t)Q.cursor_h * 4;
  Q.stats.t_table_ms = Q.t_table_ms;
  return RSI_OK;
}
// A caller's arrays in place of a BAM's (the debug hooks), behind pairs_upload.
int pin_upload(rsi_ctx* ctx, int64_t n, const int32_t* lq, const uint32_t* coff, const uint32_t* pool, int64_t npool) {
  rsi_ctx::Pin& Q = ctx->pin;
  if (int rc = pin_reset(ctx)) return rc;
  if (int rc = pin_reserve(ctx, (size_t)std::max<int64_t>(n, 1), (size_t)std::max<int64_t>(npool, 1))) return rc;
  if (n > 0) {
    HIPCHK(hipMemcpyAsync(Q.tab.p, lq, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(Q.tab.as<int32_t>() + Q.cap, coff, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
  }
  if (npool > 0) HIPCHK(hipMemcpyAsync(Q.pool.p, pool, (size_t)npool * 4, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  Q.n = n; Q.cursor_h = (uint32_t)npool;
  return RSI_OK;
}
// The depth sample over table[0, n) (behind pairs_sample on the same table, whose workspace it reads).  rd / drd: when given,
// the last stretch's arrays from its start on, rd_cap entries at the most.
int pin_sample(rsi_ctx* ctx, PairTable t, PinTable p, int64_t n, int64_t tid_len, int32_t* rd_out, int32_t* drd_out, int64_t rd_cap) {
  rsi_ctx::Pin& Q = ctx->pin;
  Q.sampled = false;
  int64_t sums[4];
  if (int rc = pairs_sample(ctx, t, n, tid_len, sums)) return rc;
  HIPCHK(Q.rdc.ensure((size_t)kPinRdcWords * 4));
  HIPCHK(Q.drd.ensure((size_t)kPinRdcWords * 4));
  HIPCHK(Q.scan.ensure((size_t)scan_tiles(kPinRdcWords) * 4 + 64));
  HIPCHK(Q.state.ensure(64));
  HIPCHK(hipEventRecord(Q.ev[0], ctx->stream));
  launch_pin_sample(t, p, (long long)n, (long long)tid_len, ctx->pairs.ws.p, Q.rdc.as<int32_t>(), Q.scan.as<int32_t>(), Q.state.p, ctx->stream);
  HIPCHK(hipEventRecord(Q.ev[1], ctx->stream));
  rsipin::SampleState st;
  HIPCHK(copy_d2h(ctx, &st, Q.state.p, sizeof(st)));
  HIPCHK(CTX_SYNC());
  Q.stats.t_sample_ms = elapsed_ms(Q.ev[0], Q.ev[1]);
  if (st.count <= 0) return fail(ctx, RSI_ERR_UNSUPPORTED, "no read from position 10000000 on passes the sample's filters");
  if (st.flags & rsipin::kGrows) return fail(ctx, RSI_ERR_UNSUPPORTED, "a sampled read ends more than 1000900 bases behind its stretch's start");
  const int l_qseq = rsipinh::l_qseq_of(st.lq_sum, st.count);
  if (l_qseq < 1) return fail(ctx, RSI_ERR_UNSUPPORTED, "the sampled reads have no sequence (read length " + std::to_string(l_qseq) + ")");
  const int64_t len = (int64_t)st.pos_end - st.pos_start, q = l_qseq / 4;
  if (len + q > rsipin::kRdcSize) return fail(ctx, RSI_ERR_UNSUPPORTED, "the sample's read length does not fit its depth array");
  const int lo = (int)q, hi = (int)std::max<int64_t>(len - q, q);
  HIPCHK(hipMemsetAsync(Q.drd.p, 0, (size_t)std::max<int64_t>(len, 1) * 4, ctx->stream));
  HIPCHK(hipEventRecord(Q.ev[0], ctx->stream));
  launch_pin_sample_drd(Q.rdc.as<int32_t>(), Q.drd.as<int32_t>(), lo, hi, l_qseq, ctx->stream);
  HIPCHK(hipEventRecord(Q.ev[1], ctx->stream));
  std::vector<int32_t> rd((size_t)std::max<int64_t>(len, 1)), drd(rd.size());
  HIPCHK(copy_d2h(ctx, rd.data(), Q.rdc.p, rd.size() * 4));
  HIPCHK(copy_d2h(ctx, drd.data(), Q.drd.p, drd.size() * 4));
  HIPCHK(CTX_SYNC());
  Q.stats.t_sample_ms += elapsed_ms(Q.ev[0], Q.ev[1]);
  const rsipinh::SampleStats s = rsipinh::sample_stats(rd.data(), drd.data(), (int)len, l_qseq);
  Q.stats.sample_reads = st.count; Q.stats.pos_start = st.pos_start; Q.stats.pos_end = st.pos_end;
  Q.stats.l_qseq = s.l_qseq; Q.stats.rd = s.rd; Q.stats.rd_sd = s.rd_sd; Q.stats.drd = s.drd; Q.stats.drd_sd = s.drd_sd;
  for (int64_t k = 0; k < std::min<int64_t>(rd_cap, len); ++k) { if (rd_out) rd_out[k] = rd[(size_t)k]; if (drd_out) drd_out[k] = drd[(size_t)k]; }
  Q.sampled = true;
  return RSI_OK;
}
// The breakpoints of the calls over table[0, n), ascending in pos.
int pin_calls(rsi_ctx* ctx, PairTable t, PinTable p, int64_t n, int maxspan, int64_t tid_len, int m, int l_qseq, double drd_sd, int ncalls,
              const int32_t* start, const int32_t* end, const int32_t* type, int32_t* new_start, int32_t* new_end, int32_t* sc1, int32_t* sc2) {
  rsi_ctx::Pin& Q = ctx->pin;
  const int r_len = rsipin::r_len_of(m, l_qseq);
  Q.stats.r_len = r_len; Q.stats.breakpoints = 0; Q.stats.t_windows_ms = 0;
  std::vector<rsipin::Bp> bps;
  std::vector<int> owner;
  for (int i = 0; i < ncalls; ++i) {
    new_start[i] = start[i]; new_end[i] = end[i]; sc1[i] = sc2[i] = 0;
    if (!rsipin::call_pinned(start[i], end[i], type[i])) continue;
    rsipin::Bp b[2];
    rsipin::bps_of(start[i], end[i], type[i], b);
    bps.push_back(b[0]); bps.push_back(b[1]);
    owner.push_back(i);
  }
  if (bps.empty()) return RSI_OK;
  if (l_qseq < 1) return fail(ctx, RSI_ERR_BAD_ARG, "read length below 1");
  if (r_len > kPinMaxRlen)
    return fail(ctx, RSI_ERR_UNSUPPORTED, "a window of " + std::to_string(r_len) + " bases on each side does not fit the workgroup's LDS (at most " +
                                              std::to_string(kPinMaxRlen) + ")");
  HIPCHK(Q.bps.ensure(bps.size() * sizeof(rsipin::Bp)));
  HIPCHK(Q.out.ensure(bps.size() * 8));
  HIPCHK(copy_h2d(ctx, Q.bps.p, bps.data(), bps.size() * sizeof(rsipin::Bp)));
  HIPCHK(hipEventRecord(Q.ev[0], ctx->stream));
  launch_pin_windows(t, p, (long long)n, maxspan, (long long)tid_len, Q.bps.p, (int)bps.size(), r_len, l_qseq, drd_sd, Q.out.as<int32_t>(), ctx->stream);
  HIPCHK(hipEventRecord(Q.ev[1], ctx->stream));
  std::vector<int32_t> res(bps.size() * 2);
  HIPCHK(copy_d2h(ctx, res.data(), Q.out.p, res.size() * 4));
  HIPCHK(CTX_SYNC());
  Q.stats.t_windows_ms = elapsed_ms(Q.ev[0], Q.ev[1]);
  Q.stats.breakpoints = (int64_t)bps.size();
  for (size_t c = 0; c < owner.size(); ++c) {
    const int i = owner[c];
    const int32_t* r = res.data() + 4 * c;
    sc1[i] = r[1]; sc2[i] = r[3];
    new_start[i] = rsipin::moved(start[i], r_len, r[0], r[1]);
    new_end[i] = rsipin::moved(end[i], r_len, r[2], r[3]);
  }
  return RSI_OK;
}

// rsi_hot_load_depth_bam's chunks in RSI_BAM_READ_DEVICE mode.  Per chunk the host walks member headers, copies
// the deflate payloads into a pinned buffer and builds the member table; upload and inflate (bgzf_launch.h) run on a stream of
// their own (istream), so the next chunk is inflated while the current chunk's records are found (guess, walk, stitch) and piled
// up on ctx->stream.  A chunk's members inflate to text_dev[b] + kBamLead; the unfinished record at the end of the chunk before
// is moved, device to device, right in front of them, so the chunk's stream is contiguous and begins with a record.
constexpr size_t kBamLead = (size_t(8) << 20) + 64;          // room for a carried record of up to 8 MB (and the guess kernel's word reads)
constexpr size_t kBamCarryMax = size_t(8) << 20;
constexpr size_t kBamChunkDefault = size_t(32) << 20, kBamChunkMin = size_t(64) << 10;
static_assert(kBamCarryMax + kBamChunkDefault + kMemberMax <= (size_t)kBamMaxSegs * RSI_BAM_SEGMENT, "a chunk's segments fit the record finder's buffers");
static_assert(kBamLead + kBamChunkDefault + kMemberMax + 64 <= kTextChunk, "a chunk fits text_dev");

int bam_chunks_device(rsi_ctx* ctx, const char* bam_path, const rsih::BamFile& bam, const std::vector<std::pair<std::string, int64_t>>& refs,
                      uint64_t voff, int tid, int64_t n, int minq, int min_baseq, int32_t* d_diff, BamDepthStats* d_stats, rsi_bam_stats* st) {
  rsi_ctx::BamDev& D = ctx->bamdev;
  rsi_bam_read_stats& rs = ctx->last_bam_read;
  rs.mode = RSI_BAM_READ_DEVICE;
  const size_t chunk = std::min(kBamChunkDefault, std::max(kBamChunkMin, ctx->bam_chunk ? ctx->bam_chunk : kBamChunkDefault));
  const size_t ccap = chunk + 4 * kMemberMax;
  if (!D.istream) HIPCHK(hipStreamCreateWithFlags(&D.istream, hipStreamNonBlocking));
  for (int b = 0; b < 2; ++b) {
    for (hipEvent_t& e : D.ev[b]) if (!e) HIPCHK(hipEventCreate(&e));
    if (!D.find[b]) HIPCHK(hipEventCreate(&D.find[b]));
    HIPCHK(D.cpin[b].ensure(ccap)); HIPCHK(D.cdev[b].ensure(ccap));
  }
  HIPCHK(D.wpin.ensure(128)); HIPCHK(D.wdev.ensure(128));
  HIPCHK(D.guess.ensure((size_t)kBamMaxSegs * 4)); HIPCHK(D.segout.ensure((size_t)kBamMaxSegs * sizeof(BamSegOut)));
  HIPCHK(D.lists.ensure((size_t)kBamMaxSegs * kBamListCap * 4)); HIPCHK(D.rec.ensure((size_t)kBamMaxSegs * kBamListCap * 4));
  std::vector<int32_t> reflen(refs.size());
  for (size_t r = 0; r < refs.size(); ++r) reflen[r] = (int32_t)std::min<int64_t>(std::max<int64_t>(refs[r].second, 0), INT32_MAX);
  HIPCHK(D.reflen.ensure(reflen.size() * 4));
  HIPCHK(hipMemcpy(D.reflen.p, reflen.data(), reflen.size() * 4, hipMemcpyHostToDevice));
  // whatever way the load ends, nothing of it is left running on the context's buffers
  struct Drain { rsi_ctx* c; ~Drain() { (void)hipStreamSynchronize(c->bamdev.istream); (void)hipStreamSynchronize(c->stream); } } drain{ctx};

  struct Chunk { size_t added = 0; bool eof = false; std::vector<uint64_t> at; } ch[2];
  bool used[2] = {false, false};
  uint64_t coff = voff >> 16;            // next member to take
  std::string perr;
  // the members of the next chunk into buffer b: payloads and table uploaded, inflate queued, status read back, on istream
  auto prepare = [&](int b) -> int {
    Chunk& c = ch[b];
    c.added = 0; c.eof = false; c.at.clear();
    std::vector<InflateBlock> tab;
    uint8_t* cp = D.cpin[b].as<uint8_t>();
    size_t comp = 0;
    while (c.added < chunk) {
      rsih::BgzfBlock blk;
      std::string e2;
      if (!bam.block_at(coff, blk, e2)) {
        if (e2.empty() && coff < bam.size()) e2 = "truncated BGZF block";
        if (!e2.empty()) { perr = e2 + " at file offset " + std::to_string((unsigned long long)coff) + " of " + bam_path; return RSI_ERR_BAD_ARG; }
        c.eof = true;
        break;
      }
      if (blk.isize > kMemberMax) { perr = "BGZF: ISIZE above 65536 in the block at file offset " + std::to_string((unsigned long long)coff) + " of " + bam_path; return RSI_ERR_BAD_ARG; }
      const uint32_t clen = blk.csize - blk.hdr - 8;
      if (!tab.empty() && comp + clen > ccap) break;
      const uint8_t* m = bam.bytes() + blk.coff;
      memcpy(cp + comp, m + blk.hdr, clen);
      uint32_t crc;
      memcpy(&crc, m + blk.csize - 8, 4);
      tab.push_back(InflateBlock{(long long)comp, (long long)(kBamLead + c.added), clen, blk.isize, crc, 0});
      c.at.push_back(coff);
      comp += clen; c.added += blk.isize; coff += blk.csize;
      st->bytes_compressed += blk.csize;
    }
    if (tab.empty()) return RSI_OK;
    rs.members += (int64_t)tab.size();
    BgzfLaunch& inflate = D.inflate[b];
    if (inflate.reserve(tab.size()) != hipSuccess) { perr = "out of memory for the BGZF member table"; return RSI_ERR_HIP; }
    hipStream_t s = D.istream;
    hipError_t e = used[b] ? hipStreamWaitEvent(s, D.ev[b][3], 0) : hipSuccess;   // text_dev[b]'s chunk before is piled up
    if (e == hipSuccess) e = hipEventRecord(D.ev[b][0], s);
    if (e == hipSuccess) e = inflate.queue(tab, cp, comp, D.cdev[b].p, ctx->text_dev[b].p, -1, s, D.ev[b][1]);   // ev[b][1]: the uploads end, the inflate begins
    if (e == hipSuccess) e = hipEventRecord(D.ev[b][2], s);
    if (e != hipSuccess) { perr = std::string("BAM device read: ") + hipGetErrorString(e); return RSI_ERR_HIP; }
    return RSI_OK;
  };

  size_t skip = (size_t)(voff & 0xffff); // bytes of the first member in front of the first record
  size_t carry = 0;                      // bytes of the unfinished record in front of the current chunk's members
  int cur = 0;
  if (int rc = prepare(0)) return fail(ctx, rc, perr);
  for (;;) {
    Chunk& c = ch[cur];
    const int other = cur ^ 1;
    const bool more = !c.eof;
    if (more) if (int rc = prepare(other)) return fail(ctx, rc, perr);
    if (!c.at.empty()) {
      const double tq = now_ms();
      HIPCHK(event_wait(D.ev[cur][2]));
      st->t_wait_ms += now_ms() - tq;
      rs.t_upload_ms += elapsed_ms(D.ev[cur][0], D.ev[cur][1]);
      const double t_inflate = elapsed_ms(D.ev[cur][1], D.ev[cur][2]);
      rs.t_inflate_ms += t_inflate; st->t_inflate_ms += t_inflate;
      const BgzfLaunch::Result r = D.inflate[cur].result();
      if (!r.ok)
        return fail(ctx, RSI_ERR_BAD_ARG, "BGZF: the block at file offset " + std::to_string(r.member < c.at.size() ? (unsigned long long)c.at[r.member] : 0ull) + " of " + bam_path +
                                              " is bad: " + rsinf::err_name(r.error));
      ++rs.chunks;
      st->bytes_inflated += (int64_t)c.added;
    }
    if (skip > c.added) return fail(ctx, RSI_ERR_BAD_ARG, "the first record's offset lies behind its BGZF block");
    const size_t base = kBamLead - carry + skip, total = carry + c.added - skip;
    skip = 0;
    const uint8_t* data = ctx->text_dev[cur].as<uint8_t>() + base;
    BamFindReport rep{};
    if (bam_segments((long long)total) > kBamMaxSegs) return fail(ctx, RSI_ERR_INTERNAL, "BAM device read: a chunk has more segments than the record finder takes");
    if (total > 0) {
      char* w = D.wdev.as<char>() + 64 * cur;
      BamFindReport* d_rep = reinterpret_cast<BamFindReport*>(w);
      HIPCHK(hipEventRecord(D.find[0], ctx->stream));
      { Timer t(ctx, "bam_guess"); launch_bam_guess(data, (long long)total, (int)reflen.size(), D.reflen.as<int32_t>(), D.guess.as<uint32_t>(), ctx->stream); }
      { Timer t(ctx, "bam_walk"); launch_bam_walk(data, (long long)total, tid, D.guess.as<uint32_t>(), D.segout.as<BamSegOut>(), D.lists.as<uint32_t>(), ctx->stream); }
      { Timer t(ctx, "bam_stitch"); launch_bam_stitch(data, (long long)total, tid, D.guess.as<uint32_t>(), D.segout.as<BamSegOut>(), D.lists.as<uint32_t>(), D.rec.as<uint32_t>(), d_rep, ctx->stream); }
      HIPCHK(hipEventRecord(D.find[1], ctx->stream));
      HIPCHK(hipMemcpyAsync(D.wpin.as<char>() + 64 * cur, d_rep, sizeof(BamFindReport), hipMemcpyDeviceToHost, ctx->stream));
      { const double tq = now_ms(); HIPCHK(CTX_SYNC()); st->t_wait_ms += now_ms() - tq; }
      memcpy(&rep, D.wpin.as<char>() + 64 * cur, sizeof(rep));
      const double t_find = elapsed_ms(D.find[0], D.find[1]);
      rs.t_find_ms += t_find; st->t_walk_ms += t_find;
      rs.segments += bam_segments((long long)total); rs.guessed += rep.guessed; rs.rewalked += rep.rewalked; rs.passed += rep.passed;
      st->records += rep.seen; st->on_chrom += rep.listed;
      if (rep.flags & rsibam::kBad) return fail(ctx, RSI_ERR_BAD_ARG, "malformed BAM record");
      if (rep.end > total || rep.listed > (uint32_t)kBamMaxSegs * kBamListCap) return fail(ctx, RSI_ERR_INTERNAL, "BAM device read: the record finder's report is out of range");
      if (rep.listed) { Timer t(ctx, "bam_depth"); launch_bam_depth(data, D.rec.as<uint32_t>(), (int)rep.listed, tid, minq, min_baseq, (long long)n, d_diff, d_stats, ctx->stream); }
      if (ctx->pairs.armed) if (int rc = pairs_append(ctx, data, D.rec.as<uint32_t>(), (int)rep.listed, tid)) return rc;
      if (ctx->pin.armed) if (int rc = pin_append(ctx, data, D.rec.as<uint32_t>(), (int)rep.listed, (size_t)rep.end)) return rc;
    }
    const bool finished = (rep.flags & rsibam::kBeyond) || !more;
    carry = finished ? 0 : total - rep.end;
    if (carry > kBamCarryMax) return fail(ctx, RSI_ERR_UNSUPPORTED, "a BAM record is longer than 8 MB");
    if (carry) HIPCHK(hipMemcpyAsync(ctx->text_dev[other].as<uint8_t>() + kBamLead - carry, data + rep.end, carry, hipMemcpyDeviceToDevice, ctx->stream));
    HIPCHK(hipEventRecord(D.ev[cur][3], ctx->stream));
    used[cur] = true;
    if (finished) break;
    cur = other;
  }
  return RSI_OK;
}
// rsi_hot_run_bam and rsi_hot_run_bam_dfasta, likewise
int run_bam(rsi_ctx* ctx, const rsi_params* p, const char* bam_path, const char* chrom, int minq, int min_baseq, const uint8_t* fasta,
            const void* d_fasta, int64_t n, rsi_result** out, rsi_bam_stats* stats) {
  ExcludeOneShot one_shot(ctx);
  if (!ctx || !p || !bam_path || !chrom || (!fasta && !d_fasta) || !out) return fail(ctx, RSI_ERR_BAD_ARG, "null argument");
  rsi_bam_stats local;
  rsi_bam_stats* st = stats ? stats : &local;
  ctx->ktimes.clear(); ctx->event_next = 0;
  int rc = rsi_hot_load_depth_bam(ctx, bam_path, chrom, minq, min_baseq, st);
  if (rc != RSI_OK) return rc;
  if (st->n != n) return fail(ctx, RSI_ERR_BAD_ARG, "reference and target not same size (loaddata.cpp:284-287)");
  if (fasta && (rc = upload_fasta(ctx, fasta, n)) != RSI_OK) return rc;
  return rsi_hot_run_device(ctx, p, ctx->in_depth.p, fasta ? ctx->in_fasta.p : d_fasta, n, out);
}
}  // namespace

extern "C" {

int rsi_hot_load_depth_bam(rsi_ctx* ctx, const char* bam_path, const char* chrom, int minq, int min_baseq, rsi_bam_stats* stats) {
  rsi_bam_stats local;
  rsi_bam_stats* st = stats ? stats : &local;
  memset(st, 0, sizeof(*st));
  if (!ctx || !bam_path || !chrom) return fail(ctx, RSI_ERR_BAD_ARG, "null argument");
  ctx->last_bam_read = rsi_bam_read_stats{};
  const double t0 = now_ms();
  HIPCHK(hipSetDevice(ctx->device));
  std::string err;
  rsih::BamFile bam;
  if (!bam.open(bam_path, err)) return fail(ctx, RSI_ERR_BAD_ARG, err);
  std::vector<std::pair<std::string, int64_t>> refs;
  uint64_t voff = 0;
  if (!bam.read_header(refs, voff, err)) return fail(ctx, RSI_ERR_BAD_ARG, err);
  int tid = -1;
  for (size_t r = 0; r < refs.size(); ++r) if (refs[r].first == chrom) tid = (int)r;
  if (tid < 0) return fail(ctx, RSI_ERR_BAD_ARG, std::string("chromosome not in the BAM header: ") + chrom);
  const int64_t n = refs[(size_t)tid].second;
  if (n <= 0 || n >= (1ll << 31) - 4096) return fail(ctx, RSI_ERR_BAD_ARG, "chromosome length must be in (0, 2^31)");
  st->tid = tid; st->n = n;
  uint64_t idx_off = 0;
  if (rsih::bai_first_offset(std::string(bam_path) + ".bai", tid, idx_off)) { voff = idx_off; st->indexed = 1; }

  if (!ctx_enter(ctx)) return RSI_ERR_HIP;

  mailbox_reset(ctx);
  HIPCHK(ctx->in_depth.ensure((size_t)(n + 4) * 4));
  int32_t* d_diff = ctx->in_depth.as<int32_t>();     // difference array first, scanned in place into the depth
  HIPCHK(hipMemsetAsync(d_diff, 0, (size_t)(n + 1) * 4, ctx->stream));
  ctx->n_in = n;
  if (int rc = ctx_staging(ctx)) return rc;
  constexpr size_t kMaxRec = kTextChunk / 36 + 16;   // a record is at least 36 bytes
  const size_t stats_off = 2 * kMaxRec * 4, scan_off = stats_off + 256;
  HIPCHK(ctx->text_wg.ensure(scan_off + (size_t)scan_tiles(n) * 4 + 64));
  uint8_t* wsb = ctx->text_wg.as<uint8_t>();
  BamDepthStats* d_stats = reinterpret_cast<BamDepthStats*>(wsb + stats_off);
  HIPCHK(hipMemsetAsync(d_stats, 0, sizeof(BamDepthStats), ctx->stream));
  ctx->pairs.valid = false;              // whatever table the context held was the load before's
  if (ctx->pairs.armed) if (int rc = pairs_begin(ctx)) return rc;
  ctx->pin.valid = ctx->pin.sampled = false;
  if (ctx->pin.armed) if (int rc = pin_reset(ctx)) return rc;

  // behind the last chunk, in either mode: the difference array scanned into the depth, the pileup's counts
  auto finish = [&]() -> int {
    { Timer t(ctx, "depth_scan"); launch_inclusive_scan_i32(d_diff, (long long)n, reinterpret_cast<int32_t*>(wsb + scan_off), ctx->stream); }
    BamDepthStats hs;
    HIPCHK(hipMemcpyAsync(&hs, d_stats, sizeof(hs), hipMemcpyDeviceToHost, ctx->stream));
    int32_t pw[kPairWords] = {0, 0, 0, 0};
    if (ctx->pairs.armed) HIPCHK(hipMemcpyAsync(pw, ctx->pairs.words.p, sizeof(pw), hipMemcpyDeviceToHost, ctx->stream));
    { const double tq = now_ms(); HIPCHK(hipStreamSynchronize(ctx->stream)); st->t_wait_ms += now_ms() - tq; }
    st->used = (int64_t)hs.used; st->runs = (int64_t)hs.runs; st->malformed = (int64_t)hs.malformed;
    if (ctx->pairs.armed) pairs_end(ctx, pw, tid, n);
    if (ctx->pin.armed) if (int rc = pin_end(ctx)) return rc;
    st->t_total_ms = now_ms() - t0;
    return RSI_OK;
  };
  if (ctx->bam_read == RSI_BAM_READ_DEVICE) {
    if (int rc = bam_chunks_device(ctx, bam_path, bam, refs, voff, tid, n, minq, min_baseq, d_diff, d_stats, st)) return rc;
    return finish();
  }

  hipEvent_t done[2] = {nullptr, nullptr};
  for (int b = 0; b < 2; ++b) if (hipEventCreateWithFlags(&done[b], hipEventDisableTiming) != hipSuccess) return fail(ctx, RSI_ERR_HIP, "hipEventCreate failed");
  struct EvGuard { hipEvent_t* e; ~EvGuard() { for (int b = 0; b < 2; ++b) if (e[b]) (void)hipEventDestroy(e[b]); } } evguard{done};
  bool used[2] = {false, false};
  std::vector<uint32_t> rec_off[2];
  rec_off[0].reserve(kMaxRec / 8); rec_off[1].reserve(kMaxRec / 8);
  const unsigned nthreads = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));

  // Pipeline over chunks of inflated bytes: while the host walks the records of chunk k and hands them to the device,
  // the inflate threads already fill the other buffer with chunk k+1.  The inflated data of a chunk starts at kReserve,
  // so that the unfinished record at the end of chunk k can be parked right in front of chunk k+1 without waiting.
  constexpr size_t kReserve = size_t(8) << 20;
  struct Chunk {
    std::vector<rsih::BgzfBlock> blocks;
    std::vector<size_t> at;
    // speculative record walk of each block, done by the thread that inflated it, as if the block began on a record
    // boundary (htslib and samtools flush before a record that would not fit, so normally it does): offsets of the
    // records of `tid` that lie wholly inside the block, how many records were seen, where the walk stopped, and
    // whether it met a read beyond `tid` (the end of the chromosome in a sorted file)
    struct BlockWalk { std::vector<uint32_t> offs; uint32_t seen = 0; size_t stop = 0; bool beyond = false, bad = false; };
    std::vector<BlockWalk> walks;
    size_t end = kReserve;     // end of the inflated data in the buffer
    bool eof = false, failed = false;
    std::string err;
    double t_inflate = 0;
    std::thread worker;
  } chunk[2];
  uint64_t coff = voff >> 16;            // next block to inflate
  auto prepare = [&](int b) -> bool {    // choose the blocks of the next chunk and start inflating them into buffer b
    Chunk& c = chunk[b];
    c.blocks.clear(); c.at.clear(); c.end = kReserve; c.eof = false; c.failed = false; c.err.clear();
    for (;;) {
      rsih::BgzfBlock blk;
      std::string e2;
      if (!bam.block_at(coff, blk, e2)) { if (!e2.empty()) { c.failed = true; c.err = e2; return false; } c.eof = true; break; }
      if (c.end + blk.isize > kTextChunk) break;
      c.blocks.push_back(blk); c.at.push_back(c.end);
      c.end += blk.isize; coff += blk.csize;
      st->bytes_compressed += blk.csize;
    }
    if (c.blocks.empty() && !c.eof) { c.failed = true; c.err = "a BGZF block does not fit the staging buffer"; return false; }
    uint8_t* buf = reinterpret_cast<uint8_t*>(ctx->text_pin[b]);
    c.walks.assign(c.blocks.size(), Chunk::BlockWalk());
    c.worker = std::thread([&c, buf, &bam, nthreads, tid]() {
      const double ti = now_ms();
      std::atomic<size_t> next(0);
      std::mutex emu;
      auto work = [&]() {
        for (;;) {
          const size_t k = next.fetch_add(1);
          if (k >= c.blocks.size()) break;
          std::string e2;
          if (!bam.inflate(c.blocks[k], buf + c.at[k], e2)) { std::lock_guard<std::mutex> lk(emu); c.failed = true; c.err = e2; continue; }
          Chunk::BlockWalk& w = c.walks[k];
          size_t p = c.at[k];
          const size_t lim = c.at[k] + c.blocks[k].isize;
          while (p + 8 <= lim) {
            const uint32_t bs = (uint32_t)buf[p] | ((uint32_t)buf[p + 1] << 8) | ((uint32_t)buf[p + 2] << 16) | ((uint32_t)buf[p + 3] << 24);
            if (bs < 32) { w.bad = true; break; }          // not a record start after all (or a broken file): the checker decides
            if (p + 4 + (size_t)bs > lim) break;
            const int32_t rtid = (int32_t)((uint32_t)buf[p + 4] | ((uint32_t)buf[p + 5] << 8) | ((uint32_t)buf[p + 6] << 16) | ((uint32_t)buf[p + 7] << 24));
            ++w.seen;
            if (rtid == tid) w.offs.push_back((uint32_t)(p - c.at[k]));
            else if (rtid > tid || rtid < 0) { w.beyond = true; break; }
            p += 4 + (size_t)bs;
          }
          w.stop = p;
        }
      };
      std::vector<std::thread> th;
      const unsigned nt = (unsigned)std::min<size_t>(nthreads, c.blocks.size());
      for (unsigned t = 1; t < nt; ++t) th.emplace_back(work);
      work();
      for (auto& t : th) t.join();
      c.t_inflate = now_ms() - ti;
    });
    return true;
  };
  struct JoinGuard { Chunk* c; ~JoinGuard() { for (int b = 0; b < 2; ++b) if (c[b].worker.joinable()) c[b].worker.join(); } } joinguard{chunk};

  size_t skip = (size_t)(voff & 0xffff); // bytes of the first block that precede the first record
  size_t carry = 0;                      // bytes of an unfinished record parked in front of the current chunk's data
  bool finished = false;
  int cur = 0;
  if (!prepare(0)) return fail(ctx, RSI_ERR_BAD_ARG, chunk[0].err);
  while (!finished) {
    Chunk& c = chunk[cur];
    c.worker.join();
    if (c.failed) return fail(ctx, RSI_ERR_BAD_ARG, c.err);
    st->t_inflate_ms += c.t_inflate;
    st->bytes_inflated += (int64_t)(c.end - kReserve);
    const int other = cur ^ 1;
    // the other buffer is free once the device has taken its previous chunk: start the next inflate right away
    { const double tq = now_ms(); if (used[other]) { HIPCHK(hipEventSynchronize(done[other])); used[other] = false; } st->t_wait_ms += now_ms() - tq; }
    bool more = false;
    if (!c.eof) { if (!prepare(other)) return fail(ctx, RSI_ERR_BAD_ARG, chunk[other].err); more = true; }
    // ---- record boundaries; the BAM is coordinate sorted, so reading ends with the first read beyond `tid` ----
    uint8_t* buf = reinterpret_cast<uint8_t*>(ctx->text_pin[cur]);
    const double tw = now_ms();
    std::vector<uint32_t>& offs = rec_off[cur];
    offs.clear();
    const size_t start = kReserve - carry + skip;   // `skip` only applies to the very first chunk (no carry there)
    skip = 0;
    size_t p = start;
    const size_t have = c.end;
    size_t kb = 0;                       // first block that starts at or after p
    while (p + 4 <= have && !finished) {
      while (kb < c.blocks.size() && c.at[kb] < p) ++kb;
      if (kb < c.blocks.size() && c.at[kb] == p && !c.walks[kb].bad) {
        // the block does begin on a record boundary: its thread has walked it already
        const Chunk::BlockWalk& w = c.walks[kb];
        const uint32_t base = (uint32_t)(p - start);
        for (uint32_t o : w.offs) offs.push_back(base + o);
        st->records += w.seen; st->on_chrom += (int64_t)w.offs.size();
        if (w.beyond) { finished = true; p = w.stop; break; }
        if (w.stop == p) {               // not even one whole record in this block: walk it the plain way below
        } else { p = w.stop; ++kb; continue; }
      }
      const uint32_t bs = (uint32_t)buf[p] | ((uint32_t)buf[p + 1] << 8) | ((uint32_t)buf[p + 2] << 16) | ((uint32_t)buf[p + 3] << 24);
      if (bs < 32) return fail(ctx, RSI_ERR_BAD_ARG, "malformed BAM record");
      if (p + 4 + bs > have) break;
      const int32_t rtid = (int32_t)((uint32_t)buf[p + 4] | ((uint32_t)buf[p + 5] << 8) | ((uint32_t)buf[p + 6] << 16) | ((uint32_t)buf[p + 7] << 24));
      ++st->records;
      if (rtid == tid) { offs.push_back((uint32_t)(p - start)); ++st->on_chrom; }
      else if (rtid > tid || rtid < 0) { finished = true; break; }
      p += 4 + (size_t)bs;
    }
    if (c.eof) finished = true;
    st->t_walk_ms += now_ms() - tw;
    const size_t len = p;                // end of the whole records examined
    if (!offs.empty()) {
      uint32_t* d_off = reinterpret_cast<uint32_t*>(wsb + (size_t)cur * kMaxRec * 4);
      HIPCHK(hipMemcpyAsync(ctx->text_dev[cur].p, buf + start, len - start, hipMemcpyHostToDevice, ctx->stream));
      HIPCHK(hipMemcpyAsync(d_off, offs.data(), offs.size() * 4, hipMemcpyHostToDevice, ctx->stream));
      { Timer t(ctx, "bam_depth"); launch_bam_depth(ctx->text_dev[cur].p, d_off, (int)offs.size(), tid, minq, min_baseq, (long long)n, d_diff, d_stats, ctx->stream); }
      if (ctx->pairs.armed) if (int rc = pairs_append(ctx, ctx->text_dev[cur].p, d_off, (int)offs.size(), tid)) return rc;
      if (ctx->pin.armed) if (int rc = pin_append(ctx, ctx->text_dev[cur].p, d_off, (int)offs.size(), len - start)) return rc;
      HIPCHK(hipEventRecord(done[cur], ctx->stream));
      used[cur] = true;
    }
    carry = finished ? 0 : have - len;
    if (carry > kReserve) return fail(ctx, RSI_ERR_UNSUPPORTED, "a BAM record is longer than 8 MB");
    if (carry && more) memcpy(ctx->text_pin[other] + (kReserve - carry), buf + len, carry);   // in front of the data being inflated there
    if (!more) finished = true;
    cur = other;
  }
  return finish();
}

int rsi_hot_set_bam_read(rsi_ctx* ctx, int mode, size_t chunk_bytes) {
  if (!ctx) return fail(ctx, RSI_ERR_BAD_ARG, "null context");
  if (mode != RSI_BAM_READ_HOST && mode != RSI_BAM_READ_DEVICE) return fail(ctx, RSI_ERR_BAD_ARG, "BAM read mode must be RSI_BAM_READ_HOST or RSI_BAM_READ_DEVICE");
  ctx->bam_read = mode;
  ctx->bam_chunk = chunk_bytes;
  return RSI_OK;
}
int rsi_hot_last_bam_read_stats(const rsi_ctx* ctx, rsi_bam_read_stats* out) {
  if (!ctx || !out) return RSI_ERR_BAD_ARG;
  *out = ctx->last_bam_read;
  return RSI_OK;
}

int rsi_hot_set_bam_pairs(rsi_ctx* ctx, int on) {
  if (!ctx) return fail(ctx, RSI_ERR_BAD_ARG, "null context");
  ctx->pairs.armed = on != 0;
  return RSI_OK;
}
int rsi_hot_last_pairs_stats(const rsi_ctx* ctx, rsi_pairs_stats* out) {
  if (!ctx || !out) return RSI_ERR_BAD_ARG;
  *out = ctx->pairs.valid ? ctx->pairs.stats : rsi_pairs_stats{};
  return RSI_OK;
}

int rsi_result_annotate_device(rsi_ctx* ctx, rsi_result* r) {
  if (!ctx || !r) return fail(ctx, RSI_ERR_BAD_ARG, "null argument");
  rsi_ctx::Pairs& P = ctx->pairs;
  if (!P.valid) return fail(ctx, RSI_ERR_BAD_ARG, "no pair table: the context's last BAM load was not armed (rsi_hot_set_bam_pairs)");
  if (r->stats.n != P.tid_len) return fail(ctx, RSI_ERR_BAD_ARG, "the pair table the context holds is not of the result's chromosome");
  if (P.flags & rsipairs::kUnsorted) return fail(ctx, RSI_ERR_UNSUPPORTED, "BAM not sorted by position");
  if (P.flags & rsipairs::kOverrun) return fail(ctx, RSI_ERR_BAD_ARG, "malformed BAM record (name / CIGAR overrun the record)");
  HIPCHK(hipSetDevice(ctx->device));
  if (!ctx_enter(ctx)) return RSI_ERR_HIP;
  mailbox_reset(ctx);
  int64_t sums[4];
  if (int rc = pairs_sample(ctx, pair_table(ctx), P.n, P.tid_len, sums)) return rc;
  const rsih::PairSample ps = pairs_sample_result(sums);
  P.stats.isize = ps.isize; P.stats.isize_sd = ps.isize_sd;
  std::vector<rsipairs::Call> calls;
  rsipairs::Windows win;
  for (const rsi_call& c : r->lists[0]) calls.push_back(win.next(c.start, c.end, c.type));
  std::vector<uint32_t> counts;
  if (int rc = pairs_annotate(ctx, pair_table(ctx), P.n, P.maxspan, calls, ps.isize, ps.isize_sd, counts)) return rc;
  r->rp.clear(); r->q0.clear();
  for (size_t i = 0; i < calls.size(); ++i) {
    const double q0_all = (double)counts[4 * i], q0_q0 = (double)counts[4 * i + 1];
    r->rp.push_back((int32_t)counts[4 * i + 2]);
    r->q0.push_back(q0_q0 / (q0_all + 0.00001));
  }
  return RSI_OK;
}

int rsi_hot_debug_pair_sample(rsi_ctx* ctx, int64_t n, const int32_t* pos, const int32_t* rend, const int32_t* mpos, const int32_t* isize,
                              const int32_t* info, int64_t tid_len, int64_t* out) {
  if (!ctx || !out || n < 0 || n >= (1ll << 31) || (n > 0 && (!pos || !rend || !mpos || !isize || !info))) return fail(ctx, RSI_ERR_BAD_ARG, "bad argument");
  HIPCHK(hipSetDevice(ctx->device));
  if (!ctx_enter(ctx)) return RSI_ERR_HIP;
  mailbox_reset(ctx);
  const int32_t* const arrays[5] = {pos, rend, mpos, isize, info};
  if (int rc = pairs_upload(ctx, n, arrays)) return rc;
  return pairs_sample(ctx, pair_table(ctx), n, tid_len, out);
}

int rsi_hot_debug_pair_annotate(rsi_ctx* ctx, int64_t n, const int32_t* pos, const int32_t* rend, const int32_t* mpos, const int32_t* isize,
                                const int32_t* info, int ncalls, const int32_t* start, const int32_t* end, const int32_t* type,
                                int isize_mean, int isize_sd, uint32_t* rp_out, uint32_t* q0all_out, uint32_t* q0q0_out) {
  if (!ctx || n < 0 || n >= (1ll << 31) || (n > 0 && (!pos || !rend || !mpos || !isize || !info)) || ncalls < 0 ||
      (ncalls > 0 && (!start || !end || !type || !rp_out || !q0all_out || !q0q0_out)))
    return fail(ctx, RSI_ERR_BAD_ARG, "bad argument");
  int64_t maxspan = 0;
  for (int64_t i = 0; i < n; ++i) {
    if (i > 0 && pos[i] < pos[i - 1]) return fail(ctx, RSI_ERR_UNSUPPORTED, "BAM not sorted by position");
    maxspan = std::max(maxspan, (int64_t)rend[i] - (int64_t)pos[i]);
  }
  HIPCHK(hipSetDevice(ctx->device));
  if (!ctx_enter(ctx)) return RSI_ERR_HIP;
  mailbox_reset(ctx);
  const int32_t* const arrays[5] = {pos, rend, mpos, isize, info};
  if (int rc = pairs_upload(ctx, n, arrays)) return rc;
  std::vector<rsipairs::Call> calls;
  rsipairs::Windows win;
  for (int i = 0; i < ncalls; ++i) calls.push_back(win.next(start[i], end[i], type[i]));
  std::vector<uint32_t> counts;
  if (int rc = pairs_annotate(ctx, pair_table(ctx), n, (int)std::min<int64_t>(maxspan, INT32_MAX), calls, isize_mean, isize_sd, counts)) return rc;
  for (int i = 0; i < ncalls; ++i) { q0all_out[i] = counts[4 * (size_t)i]; q0q0_out[i] = counts[4 * (size_t)i + 1]; rp_out[i] = counts[4 * (size_t)i + 2]; }
  return RSI_OK;
}

// ---- `stat` and `pin` ----
namespace {
// the refusals every entry point over a BAM's table shares
int table_usable(rsi_ctx* ctx) {
  const rsi_ctx::Pairs& P = ctx->pairs;
  if (!P.valid) return fail(ctx, RSI_ERR_BAD_ARG, "no pair table: the context's last BAM load was not armed (rsi_hot_set_bam_pairs)");
  if (P.flags & rsipairs::kUnsorted) return fail(ctx, RSI_ERR_UNSUPPORTED, "BAM not sorted by position");
  if (P.flags & rsipairs::kOverrun) return fail(ctx, RSI_ERR_BAD_ARG, "malformed BAM record (name / CIGAR overrun the record)");
  return RSI_OK;
}
int pin_usable(rsi_ctx* ctx) {
  if (int rc = table_usable(ctx)) return rc;
  if (!ctx->pin.valid || ctx->pin.n != ctx->pairs.n) return fail(ctx, RSI_ERR_BAD_ARG, "no CIGAR table: the context's last BAM load was not armed (rsi_hot_set_bam_pin)");
  return RSI_OK;
}
int debug_tables(rsi_ctx* ctx, int64_t n, const int32_t* const arrays[5], const int32_t* lq, const uint32_t* coff, const uint32_t* pool, int64_t npool,
                 int64_t* maxspan) {
  if (n < 0 || n >= (1ll << 31) || npool < 1 || npool >= (1ll << 32) || !pool || (n > 0 && (!arrays[0] || !arrays[1] || !arrays[2] || !arrays[3] || !arrays[4] || !lq || !coff)))
    return fail(ctx, RSI_ERR_BAD_ARG, "bad argument");
  *maxspan = 0;
  for (int64_t i = 0; i < n; ++i) {
    if (i > 0 && arrays[0][i] < arrays[0][i - 1]) return fail(ctx, RSI_ERR_UNSUPPORTED, "BAM not sorted by position");
    if ((int64_t)coff[i] >= npool || (int64_t)coff[i] + 1 + (int64_t)pool[coff[i]] > npool) return fail(ctx, RSI_ERR_BAD_ARG, "a CIGAR lies outside the pool");
    *maxspan = std::max(*maxspan, (int64_t)arrays[1][i] - (int64_t)arrays[0][i]);
  }
  HIPCHK(hipSetDevice(ctx->device));
  if (!ctx_enter(ctx)) return RSI_ERR_HIP;
  mailbox_reset(ctx);
  if (int rc = pairs_upload(ctx, n, arrays)) return rc;
  return pin_upload(ctx, n, lq, coff, pool, npool);
}
}  // namespace

int rsi_hot_set_bam_pin(rsi_ctx* ctx, int on) {
  if (!ctx) return fail(ctx, RSI_ERR_BAD_ARG, "null context");
  ctx->pin.armed = on != 0;
  if (on) ctx->pairs.armed = true;       // the CIGARs lie beside the pair table's entries
  return RSI_OK;
}
int rsi_hot_last_pin_stats(const rsi_ctx* ctx, rsi_pin_stats* out) {
  if (!ctx || !out) return RSI_ERR_BAD_ARG;
  *out = ctx->pin.valid ? ctx->pin.stats : rsi_pin_stats{};
  return RSI_OK;
}

int rsi_hot_stat_calls(rsi_ctx* ctx, int ncalls, const int32_t* start, const int32_t* end, const int32_t* type, const int32_t* p1e, const int32_t* p2e,
                       int32_t* isize_io, int32_t* isize_sd_io, int32_t* rp, double* q0) {
  if (!ctx || ncalls < 0 || !isize_io || !isize_sd_io || (ncalls > 0 && (!start || !end || !type || !p1e || !p2e || !rp || !q0)))
    return fail(ctx, RSI_ERR_BAD_ARG, "bad argument");
  if (int rc = table_usable(ctx)) return rc;
  rsi_ctx::Pairs& P = ctx->pairs;
  HIPCHK(hipSetDevice(ctx->device));
  if (!ctx_enter(ctx)) return RSI_ERR_HIP;
  mailbox_reset(ctx);
  int64_t sums[4];
  if (int rc = pairs_sample(ctx, pair_table(ctx), P.n, P.tid_len, sums)) return rc;
  const rsih::PairSample ps = pairs_sample_result(sums);
  P.stats.isize = ps.isize; P.stats.isize_sd = ps.isize_sd;
  if (sums[0] > 2) { *isize_io = ps.isize; *isize_sd_io = ps.isize_sd; }    // (isize_c > 2: else bamstat_st keeps what it had)
  std::vector<rsipairs::Call> calls((size_t)ncalls);
  for (int i = 0; i < ncalls; ++i) {
    const int32_t b = std::min(start[i], end[i]), e = std::max(start[i], end[i]);
    calls[(size_t)i] = rsipairs::Call{b, e, type[i], e - b + 1, p1e[i], p2e[i]};
  }
  std::vector<uint32_t> counts;
  if (int rc = pairs_annotate(ctx, pair_table(ctx), P.n, P.maxspan, calls, *isize_io, *isize_sd_io, counts)) return rc;
  for (int i = 0; i < ncalls; ++i) {
    const double q0_all = (double)counts[4 * (size_t)i], q0_q0 = (double)counts[4 * (size_t)i + 1];
    rp[i] = (int32_t)counts[4 * (size_t)i + 2];
    q0[i] = q0_q0 / (q0_all + 0.00001);
  }
  return RSI_OK;
}

int rsi_hot_pin_sample(rsi_ctx* ctx, rsi_pin_stats* out) {
  if (!ctx) return fail(ctx, RSI_ERR_BAD_ARG, "null context");
  if (int rc = pin_usable(ctx)) return rc;
  HIPCHK(hipSetDevice(ctx->device));
  if (!ctx_enter(ctx)) return RSI_ERR_HIP;
  mailbox_reset(ctx);
  const int rc = pin_sample(ctx, pair_table(ctx), pin_table(ctx), ctx->pairs.n, ctx->pairs.tid_len, nullptr, nullptr, 0);
  if (out) *out = ctx->pin.stats;
  return rc;
}

int rsi_hot_pin_calls(rsi_ctx* ctx, int m, int ncalls, const int32_t* start, const int32_t* end, const int32_t* type, int32_t* new_start,
                      int32_t* new_end, int32_t* sc1, int32_t* sc2) {
  if (!ctx || ncalls < 0 || (ncalls > 0 && (!start || !end || !type || !new_start || !new_end || !sc1 || !sc2))) return fail(ctx, RSI_ERR_BAD_ARG, "bad argument");
  if (int rc = pin_usable(ctx)) return rc;
  if (!ctx->pin.sampled) return fail(ctx, RSI_ERR_BAD_ARG, "no sample: rsi_hot_pin_sample comes first");
  HIPCHK(hipSetDevice(ctx->device));
  if (!ctx_enter(ctx)) return RSI_ERR_HIP;
  mailbox_reset(ctx);
  return pin_calls(ctx, pair_table(ctx), pin_table(ctx), ctx->pairs.n, ctx->pairs.maxspan, ctx->pairs.tid_len, m, ctx->pin.stats.l_qseq,
                   ctx->pin.stats.drd_sd, ncalls, start, end, type, new_start, new_end, sc1, sc2);
}

int rsi_hot_debug_pin_sample(rsi_ctx* ctx, int64_t n, const int32_t* pos, const int32_t* rend, const int32_t* mpos, const int32_t* isize,
                             const int32_t* info, const int32_t* lq, const uint32_t* coff, const uint32_t* pool, int64_t npool, int64_t tid_len,
                             rsi_pin_stats* out, int32_t* rd, int32_t* drd, int64_t rd_cap) {
  if (!ctx || !out) return fail(ctx, RSI_ERR_BAD_ARG, "bad argument");
  const int32_t* const arrays[5] = {pos, rend, mpos, isize, info};
  int64_t maxspan = 0;
  if (int rc = debug_tables(ctx, n, arrays, lq, coff, pool, npool, &maxspan)) return rc;
  const int rc = pin_sample(ctx, pair_table(ctx), pin_table(ctx), n, tid_len, rd, drd, rd_cap);
  *out = ctx->pin.stats;
  return rc;
}

int rsi_hot_debug_pin_calls(rsi_ctx* ctx, int64_t n, const int32_t* pos, const int32_t* rend, const int32_t* mpos, const int32_t* isize,
                            const int32_t* info, const int32_t* lq, const uint32_t* coff, const uint32_t* pool, int64_t npool, int64_t tid_len,
                            int m, int l_qseq, double drd_sd, int ncalls, const int32_t* start, const int32_t* end, const int32_t* type,
                            int32_t* new_start, int32_t* new_end, int32_t* sc1, int32_t* sc2) {
  if (!ctx || ncalls < 0 || (ncalls > 0 && (!start || !end || !type || !new_start || !new_end || !sc1 || !sc2))) return fail(ctx, RSI_ERR_BAD_ARG, "bad argument");
  const int32_t* const arrays[5] = {pos, rend, mpos, isize, info};
  int64_t maxspan = 0;
  if (int rc = debug_tables(ctx, n, arrays, lq, coff, pool, npool, &maxspan)) return rc;
  return pin_calls(ctx, pair_table(ctx), pin_table(ctx), n, (int)std::min<int64_t>(maxspan, INT32_MAX), tid_len, m, l_qseq, drd_sd, ncalls, start, end, type,
                   new_start, new_end, sc1, sc2);
}

int rsi_bam_references(const char* bam_path, char* names, int names_cap, int64_t* lengths, int max_refs) {
  if (!bam_path) return RSI_ERR_BAD_ARG;
  std::string err;
  rsih::BamFile bam;
  std::vector<std::pair<std::string, int64_t>> refs;
  uint64_t voff = 0;
  if (!bam.open(bam_path, err) || !bam.read_header(refs, voff, err)) { set_global_error(err); return RSI_ERR_BAD_ARG; }
  std::string all;
  for (size_t r = 0; r < refs.size(); ++r) {
    if (r) all += '\n';
    all += refs[r].first;
    if (lengths && (int)r < max_refs) lengths[r] = refs[r].second;
  }
  if (names && names_cap > 0) { strncpy(names, all.c_str(), (size_t)names_cap - 1); names[names_cap - 1] = 0; }
  return (int)refs.size();
}

int rsi_hot_run_bam(rsi_ctx* ctx, const rsi_params* p, const char* bam_path, const char* chrom, int minq, int min_baseq,
                    const uint8_t* fasta, int64_t n, rsi_result** out, rsi_bam_stats* stats) {
  return run_bam(ctx, p, bam_path, chrom, minq, min_baseq, fasta, nullptr, n, out, stats);
}
int rsi_hot_run_bam_dfasta(rsi_ctx* ctx, const rsi_params* p, const char* bam_path, const char* chrom, int minq, int min_baseq,
                           const void* d_fasta, int64_t n, rsi_result** out, rsi_bam_stats* stats) {
  return run_bam(ctx, p, bam_path, chrom, minq, min_baseq, nullptr, d_fasta, n, out, stats);
}

}  // extern "C"
