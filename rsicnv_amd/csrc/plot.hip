// plot.hip -- the numbers of planned gnuplot figures from a depth array in HBM, behind include/rsi_hot.h: a
// rsi_plot_batch (plot_plan.h) is filled without the array crossing PCIe.  Quartiles, sums and counts of every body and
// neighbourhood, and the array's median, are geno's (pipeline.hip: geno_run); the running mean's window sums, the queried values and
// the expansion of a run's compacted depth are kernels_plot.hip's.  The text is written on the host (plot_host.cpp).
#include "pipeline_internal.h"
#include "geno_host.h"
#include "plot_plan.h"

using namespace rsik;
using namespace rsip;

namespace rsip {

void plot_free(rsi_ctx* ctx) {
  for (hipEvent_t& e : ctx->plot.ev) { if (e) (void)hipEventDestroy(e); e = nullptr; }
}

}  // namespace rsip

namespace {

constexpr int64_t kPlotWorkspace = int64_t(64) << 20;   // what a batch's tables and results may take, geno's share included

inline size_t up256(size_t x) { return (x + 255) & ~size_t(255); }

// what the kernels rely on, checked before anything is uploaded: every index inside the array, the window ends of blocks 0 and 2
// ascending
bool plan_fits(const rsiplot::Plan& P, int64_t n) {
  if (P.a0 < 0 || P.a1 < P.a0 || P.a1 > n || P.b0 < 0 || P.b1 < P.b0 || P.b1 > n) return false;
  if (P.nref != (P.a1 - P.a0) + (P.b1 - P.b0) || P.nref < 1) return false;
  if (P.c1 < 0 || P.c2 < P.c1 || P.c2 >= n) return false;
  if (P.band < 1 || P.band > P.nref || (P.band & 1) == 0) return false;
  if (P.rows[0] < 0 || P.rows[1] < 0 || P.rows[2] < 0 || (int64_t)P.q.size() != (int64_t)P.rows[0] + P.rows[1] + P.rows[2] + 2) return false;
  size_t k = 0;
  for (int b = 0; b < 4; ++b) {
    const int cnt = b < 3 ? P.rows[b] : 2;
    int last = 0;
    for (int r = 0; r < cnt; ++r, ++k) {
      const rsiplot::Query& q = P.q[k];
      if (q.depth < -1 || q.depth >= n || q.ref < -1 || q.ref >= P.nref) return false;
      if (b == 1) continue;
      if (q.ref < 0) return false;
      if ((b == 0 || b == 2) && q.ref < last) return false;
      last = q.ref;
    }
  }
  return true;
}

// bytes of a batch's share of the workspace that call P adds (the kernels' tables and results, geno's histograms and records)
int64_t plan_cost(const rsiplot::Plan& P, int tile) {
  const int64_t nq = (int64_t)P.q.size(), nbody = (int64_t)P.c2 - P.c1 + 1;
  return 2 * (int64_t)(geno_hist_bytes(4, 1) + sizeof(GenoState) + sizeof(GenoOut)) + ((nbody + P.nref) / rsigeno::kDefaultTile + 3) * (int64_t)sizeof(GenoTile) +
         (int64_t)sizeof(PlotJob) + ((int64_t)P.nref / tile + 1) * 8 + nq * 36;
}

// A batch filled from d_depth[n]; what the three entry points share.  The caller has entered the context and reset the mailbox.
int plot_fill(rsi_ctx* ctx, const int32_t* d_depth, int64_t n, int tile, int64_t workspace, rsi_plot_batch* b) {
  rsi_ctx::Plot& W = ctx->plot;
  rsi_plot_stats& S = W.stats;
  const double t0 = now_ms();
  b->is_filled = false;
  b->chrom_median = 0;
  b->filled.assign(b->plans.size(), rsiplot::Filled{});
  if (b->n != n) return fail(ctx, RSI_ERR_BAD_ARG, "plot: the batch was planned for an array of another length");
  if (tile == 0) tile = kPlotDefaultTile;
  if (tile < 1 || tile > kPlotMaxTile || workspace < 0) return fail(ctx, RSI_ERR_BAD_ARG, "plot: a tile holds 1 .. 4096 values");
  if (workspace == 0) workspace = kPlotWorkspace;
  std::vector<size_t> todo;
  for (size_t i = 0; i < b->plans.size(); ++i) {
    if (b->plans[i].refusal != rsiplot::kOk) continue;
    if (!plan_fits(b->plans[i], n)) return fail(ctx, RSI_ERR_INTERNAL, "plot: a plan the kernels cannot take");
    todo.push_back(i);
  }
  if (todo.empty()) { b->is_filled = true; return RSI_OK; }   // nothing allocated, nothing launched
  hipStream_t st = ctx->stream;
  {   // the array's median (plot::RDmed, plotcnv.cpp:625): one more job, over all of it
    std::vector<rsigeno::Ranges> all(1);
    all[0].body.a = 0; all[0].body.b = n;
    rsi_geno_record rec;
    if (int rc = geno_run(ctx, d_depth, 4, n, all, 0, 0.0, &rec)) return rc;
    b->chrom_median = rec.body_q[1];
    S.launches += ctx->geno.stats.launches;
    S.bytes_up += ctx->geno.stats.tiles * (int64_t)sizeof(GenoTile);
    S.bytes_down += (int64_t)sizeof(GenoOut) + 4;
    mailbox_reset(ctx);
  }
  std::vector<rsigeno::Ranges> lines;
  std::vector<rsi_geno_record> recs;
  std::vector<PlotJob> jobs;
  std::vector<int32_t> qdepth, qref, value;
  std::vector<int64_t> wsum;
  for (size_t at = 0; at < todo.size();) {
    // as many calls as fit the workspace, at least one
    size_t stop = at;
    int64_t cost = 0;
    while (stop < todo.size() && (stop == at || cost + plan_cost(b->plans[todo[stop]], tile) <= workspace)) cost += plan_cost(b->plans[todo[stop++]], tile);
    const int nj = (int)(stop - at);
    lines.assign((size_t)nj, rsigeno::Ranges{});
    jobs.assign((size_t)nj, PlotJob{});
    qdepth.clear(); qref.clear();
    int64_t ntiles = 0;
    for (int k = 0; k < nj; ++k) {
      const rsiplot::Plan& P = b->plans[todo[at + (size_t)k]];
      rsigeno::Ranges& r = lines[(size_t)k];
      r.body.a = P.c1; r.body.b = (int64_t)P.c2 + 1; r.left.a = P.a0; r.left.b = P.a1; r.right.a = P.b0; r.right.b = P.b1;
      PlotJob& j = jobs[(size_t)k];
      j.a0 = P.a0; j.la = P.a1 - P.a0; j.b0 = P.b0; j.lb = P.b1 - P.b0; j.band = P.band;
      j.nq0 = P.rows[0]; j.nq1 = P.rows[1]; j.nq2 = P.rows[2];
      j.q0 = (long long)qdepth.size(); j.tile0 = (int32_t)ntiles; j.pad = 0;
      ntiles += ((int64_t)P.nref + tile - 1) / tile;
      for (const rsiplot::Query& q : P.q) { qdepth.push_back(q.depth); qref.push_back(q.ref); }
    }
    if (ntiles >= 0x7fffffff) return fail(ctx, RSI_ERR_UNSUPPORTED, "plot: more than 2^31 tiles in one batch");
    const int64_t nq = (int64_t)qdepth.size();
    recs.resize((size_t)nj);
    if (int rc = geno_run(ctx, d_depth, 4, n, lines, 0, b->chrom_median, recs.data())) return rc;
    S.launches += ctx->geno.stats.launches;
    S.bytes_up += ctx->geno.stats.tiles * (int64_t)sizeof(GenoTile);
    S.bytes_down += 2 * (int64_t)nj * (int64_t)sizeof(GenoOut) + 4;
    mailbox_reset(ctx);
    // the batch's share of the workspace: jobs | tile sums | qdepth | qref | window ends | values | window sums
    const size_t o_jobs = 0, o_tsum = o_jobs + up256((size_t)nj * sizeof(PlotJob)), o_qd = o_tsum + up256((size_t)ntiles * 8),
                 o_qr = o_qd + up256((size_t)nq * 4), o_ends = o_qr + up256((size_t)nq * 4), o_val = o_ends + up256((size_t)nq * 16),
                 o_ws = o_val + up256((size_t)nq * 4), total = o_ws + up256((size_t)nq * 8);
    HIPCHK(W.ws.ensure(total));   // (at most the workspace, but for a single call beyond it)
    S.bytes = (int64_t)(W.ws.cap + W.full.cap + W.pairs.cap);
    uint8_t* base = W.ws.as<uint8_t>();
    const PlotJob* d_jobs = reinterpret_cast<const PlotJob*>(base + o_jobs);
    long long* d_tsum = reinterpret_cast<long long*>(base + o_tsum);
    const int32_t* d_qd = reinterpret_cast<const int32_t*>(base + o_qd);
    const int32_t* d_qr = reinterpret_cast<const int32_t*>(base + o_qr);
    long long* d_ends = reinterpret_cast<long long*>(base + o_ends);
    int32_t* d_val = reinterpret_cast<int32_t*>(base + o_val);
    long long* d_ws = reinterpret_cast<long long*>(base + o_ws);
    HIPCHK(copy_h2d(ctx, base + o_jobs, jobs.data(), (size_t)nj * sizeof(PlotJob)));
    HIPCHK(copy_h2d(ctx, base + o_qd, qdepth.data(), (size_t)nq * 4));
    HIPCHK(copy_h2d(ctx, base + o_qr, qref.data(), (size_t)nq * 4));
    HIPCHK(hipMemsetAsync(d_ends, 0, (size_t)nq * 16, st));
    { Timer t(ctx, "plot_tile_sums"); launch_plot_tile_sums(d_depth, d_jobs, nj, (int)ntiles, tile, d_tsum, st); }
    { Timer t(ctx, "plot_tile_scan"); launch_plot_tile_scan(d_jobs, nj, tile, d_tsum, st); }
    { Timer t(ctx, "plot_window_ends"); launch_plot_window_ends(d_depth, d_jobs, nj, (int)ntiles, tile, d_tsum, d_qr, d_ends, st); }
    { Timer t(ctx, "plot_gather"); launch_plot_gather(d_depth, d_qd, d_qr, d_ends, nq, d_val, d_ws, st); }
    value.resize((size_t)nq); wsum.resize((size_t)nq);
    HIPCHK(copy_d2h(ctx, value.data(), d_val, (size_t)nq * 4));
    HIPCHK(copy_d2h(ctx, wsum.data(), d_ws, (size_t)nq * 8));
    HIPCHK(CTX_SYNC());
    mailbox_reset(ctx);
    for (int k = 0; k < nj; ++k) {
      const size_t i = todo[at + (size_t)k];
      const rsiplot::Plan& P = b->plans[i];
      rsiplot::Filled& F = b->filled[i];
      const size_t q0 = (size_t)jobs[(size_t)k].q0, cnt = P.q.size();
      F.value.assign(value.begin() + (ptrdiff_t)q0, value.begin() + (ptrdiff_t)(q0 + cnt));
      F.wsum.assign(wsum.begin() + (ptrdiff_t)q0, wsum.begin() + (ptrdiff_t)(q0 + cnt));
      const rsi_geno_record& r = recs[(size_t)k];
      for (int q = 0; q < 3; ++q) { F.body_q[q] = r.body_q[q]; F.ref_q[q] = r.flank_q[q]; }
      F.ref_sum = r.flank_sum;
    }
    S.launches += 4; S.batches += 1; S.tiles += ntiles; S.calls += nj; S.queries += nq;
    S.bytes_up += (int64_t)nj * (int64_t)sizeof(PlotJob) + nq * 8;
    S.bytes_down += nq * 12;
    at = stop;
  }
  b->is_filled = true;
  S.ms += now_ms() - t0;
  return RSI_OK;
}

void stats_begin(rsi_ctx* ctx) {
  const int64_t held = ctx->plot.stats.bytes;
  ctx->plot.stats = rsi_plot_stats{};
  ctx->plot.stats.bytes = held;
}

// The compacted array d_src[ncompact] (storage 1 or 4) expanded by `pairs` into ctx->plot.full[n]: rsi_plot_expand's checks, then
// the kernel.
int plot_expand(rsi_ctx* ctx, const void* d_src, int storage, int64_t ncompact, const int32_t* pairs, int npairs, int64_t n) {
  rsi_ctx::Plot& W = ctx->plot;
  if (ncompact < 0 || n < ncompact || n <= 0 || npairs < 0) return fail(ctx, RSI_ERR_BAD_ARG, "plot: cannot expand the depth");
  std::vector<int32_t> se((size_t)npairs * 2 + 1);
  std::vector<long long> before((size_t)npairs + 1);
  int64_t removed = 0;
  for (int k = 0; k < npairs; ++k) {
    const int32_t s = pairs[2 * k], e = pairs[2 * k + 1];
    if (s < 0 || e < s || e >= n || (k > 0 && s <= pairs[2 * k - 1])) return fail(ctx, RSI_ERR_BAD_ARG, "plot: cannot expand the depth: bad regions");
    se[(size_t)k] = s; se[(size_t)npairs + (size_t)k] = e; before[(size_t)k] = removed;
    removed += (int64_t)e - s + 1;
  }
  if (ncompact + removed != n) return fail(ctx, RSI_ERR_BAD_ARG, "plot: cannot expand the depth: the regions do not add up");   // loaddata.cpp:149-153
  for (hipEvent_t& e : W.ev) if (!e) HIPCHK(hipEventCreate(&e));
  const size_t o_before = up256((size_t)npairs * 8);
  HIPCHK(W.pairs.ensure(o_before + up256((size_t)npairs * 8) + 256));
  HIPCHK(W.full.ensure((size_t)(n + 4) * 4));
  W.stats.bytes = (int64_t)(W.ws.cap + W.full.cap + W.pairs.cap);
  if (npairs) {
    HIPCHK(copy_h2d(ctx, W.pairs.p, se.data(), (size_t)npairs * 8));
    HIPCHK(copy_h2d(ctx, W.pairs.as<uint8_t>() + o_before, before.data(), (size_t)npairs * 8));
  }
  (void)hipEventRecord(W.ev[0], ctx->stream);
  { Timer t(ctx, "plot_expand"); launch_plot_expand(d_src, storage, W.pairs.as<int32_t>(), W.pairs.as<int32_t>() + npairs,
                                                    reinterpret_cast<const long long*>(W.pairs.as<uint8_t>() + o_before), npairs, W.full.as<int32_t>(), n, ctx->stream); }
  (void)hipEventRecord(W.ev[1], ctx->stream);
  W.stats.launches += 1;
  W.stats.bytes_up += (int64_t)npairs * 16;
  return RSI_OK;
}

}  // namespace

extern "C" {

int rsi_hot_plot_depth(rsi_ctx* ctx, const void* d_depth, int64_t n, rsi_plot_batch* b) {
  if (!ctx || !b || !d_depth || n <= 0 || n >= (1ll << 31) - 4096) return fail(ctx, RSI_ERR_BAD_ARG, "plot: bad argument");
  HIPCHK(hipSetDevice(ctx->device));
  if (!ctx_enter(ctx)) return RSI_ERR_HIP;
  mailbox_reset(ctx);
  stats_begin(ctx);
  return plot_fill(ctx, static_cast<const int32_t*>(d_depth), n, 0, 0, b);
}

int rsi_hot_plot_run(rsi_ctx* ctx, const rsi_result* res, rsi_plot_batch* b) {
  if (!ctx || !res || !b) return fail(ctx, RSI_ERR_BAD_ARG, "plot: bad argument");
  if (!ctx->run_m || ctx->ncompact <= 0 || !(ctx->rdc_is_bytes ? ctx->rdc8.p : ctx->rdc.p) || res->stats.n != ctx->n || res->stats.n_compact != ctx->ncompact)
    return fail(ctx, RSI_ERR_BAD_ARG, "plot: the context does not hold this result's compacted depth (another run, a failed one, or a debug hook came after it)");
  HIPCHK(hipSetDevice(ctx->device));
  if (!ctx_enter(ctx)) return RSI_ERR_HIP;
  mailbox_reset(ctx);
  stats_begin(ctx);
  bool any = false;
  for (const rsiplot::Plan& P : b->plans) any = any || P.refusal == rsiplot::kOk;
  if (!any) return plot_fill(ctx, nullptr, ctx->n, 0, 0, b);   // nothing to fill: no expansion either
  const double t0 = now_ms();
  if (int rc = plot_expand(ctx, ctx->rdc_is_bytes ? ctx->rdc8.p : ctx->rdc.p, ctx->rdc_is_bytes ? 1 : 4, ctx->ncompact, ctx->noncode_pairs.data(),
                           (int)(ctx->noncode_pairs.size() / 2), ctx->n))
    return rc;
  const int rc = plot_fill(ctx, ctx->plot.full.as<int32_t>(), ctx->n, 0, 0, b);
  if (rc == RSI_OK) {   // (the fill has waited for the stream: both events have happened)
    ctx->plot.stats.expand_ms = elapsed_ms(ctx->plot.ev[0], ctx->plot.ev[1]);
    ctx->plot.stats.ms = now_ms() - t0;
  }
  return rc;
}

int rsi_hot_last_plot_stats(const rsi_ctx* ctx, rsi_plot_stats* out) {
  if (!ctx || !out) return RSI_ERR_BAD_ARG;
  *out = ctx->plot.stats;
  return RSI_OK;
}

int rsi_hot_debug_plot(rsi_ctx* ctx, const int32_t* depth, int64_t n, int tile, int64_t workspace_bytes, rsi_plot_batch* b) {
  if (!b || n <= 0 || tile < 0 || workspace_bytes < 0) return fail(ctx, RSI_ERR_BAD_ARG, "plot: bad argument");
  if (int rc = depth_upload(ctx, depth, n)) return rc;
  stats_begin(ctx);
  return plot_fill(ctx, ctx->in_depth.as<int32_t>(), n, tile, workspace_bytes, b);
}

int rsi_hot_debug_plot_expand(rsi_ctx* ctx, const int32_t* rdc, int64_t ncompact, int storage, const int32_t* regions, int npairs, int32_t* out, int64_t n) {
  if (!ctx || !out || ncompact < 0 || (ncompact > 0 && !rdc) || (storage != 1 && storage != 4) || npairs < 0 || (npairs > 0 && !regions) || n <= 0 ||
      n >= (1ll << 31) - 4096)
    return fail(ctx, RSI_ERR_BAD_ARG, "plot: bad argument");
  std::vector<uint8_t> bytes;
  if (storage == 1) {
    bytes.resize((size_t)ncompact);
    for (int64_t i = 0; i < ncompact; ++i) {
      if (rdc[i] < 0 || rdc[i] > 255) return fail(ctx, RSI_ERR_BAD_ARG, "byte storage holds depths of 0 .. 255");
      bytes[(size_t)i] = (uint8_t)rdc[i];
    }
  }
  HIPCHK(hipSetDevice(ctx->device));
  if (!ctx_enter(ctx)) return RSI_ERR_HIP;
  mailbox_reset(ctx);
  stats_begin(ctx);
  HIPCHK(ctx->plot.ws.ensure((size_t)(ncompact + 4) * (size_t)storage));
  if (ncompact) HIPCHK(hipMemcpyAsync(ctx->plot.ws.p, storage == 1 ? static_cast<const void*>(bytes.data()) : static_cast<const void*>(rdc), (size_t)ncompact * (size_t)storage,
                                      hipMemcpyHostToDevice, ctx->stream));
  if (int rc = plot_expand(ctx, ctx->plot.ws.p, storage, ncompact, regions, npairs, n)) return rc;
  HIPCHK(hipMemcpyAsync(out, ctx->plot.full.p, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(CTX_SYNC());
  return RSI_OK;
}

}  // extern "C"
