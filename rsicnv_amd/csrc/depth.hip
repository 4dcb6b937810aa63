// depth.hip -- `rsicnv depth` behind include/rsi_hot.h: the summary and distribution of a per-base depth array in
// HBM (kernels_depth.hip), the records of explicit regions (geno's tile table and min / max kernels, kernels_geno.hip), the
// context's loaded array, and their test hooks.  The window and region tracks are track.hip's: they go through its slices.
#include "pipeline_internal.h"
#include "geno_host.h"
#include "depth_host.h"

using namespace rsik;
using namespace rsip;

namespace rsip {

void depth_free(rsi_ctx* ctx) {
  for (hipEvent_t& e : ctx->depth.ev) { if (e) (void)hipEventDestroy(e); e = nullptr; }
}

int depth_region_records(rsi_ctx* ctx, const int32_t* d_depth, int64_t n, int64_t nreg, const int64_t* start, const int64_t* end, int tile,
                         rsi_depth_region* out) {
  rsi_ctx::Depth& D = ctx->depth;
  const int64_t bytes_held = D.stats.bytes;
  D.stats = rsi_depth_stats{};
  D.stats.bytes = bytes_held;
  if (nreg <= 0) return RSI_OK;
  if (nreg > (1 << 29)) return fail(ctx, RSI_ERR_UNSUPPORTED, "depth: more than 2^29 regions in one call");
  for (int64_t i = 0; i < nreg; ++i) memset(&out[i], 0, sizeof(out[i]));
  if (n <= 0) return RSI_OK;   // nothing is left of any region
  const double t0 = now_ms();
  // geno's table: a line's body is the clipped region, its flanks stay empty, so its tiles carry job 2 i
  std::vector<rsigeno::Ranges> lines((size_t)nreg);
  for (int64_t i = 0; i < nreg; ++i) {
    int64_t a, b;
    rsidepth::clip(start[i], end[i], n, a, b);
    lines[(size_t)i].body.a = a; lines[(size_t)i].body.b = b;
  }
  std::vector<rsigeno::Tile> tiles;
  if (!rsigeno::build_tiles(lines, n, tile > 0 ? tile : rsigeno::kDefaultTile, tiles)) return fail(ctx, RSI_ERR_INTERNAL, "depth: a clipped region lies outside the array");
  if (tiles.size() >= (size_t)0x7fffffff) return fail(ctx, RSI_ERR_UNSUPPORTED, "depth: more than 2^31 tiles in one call");
  for (rsigeno::Tile& t : tiles) t.job >>= 1;
  static_assert(sizeof(rsigeno::Tile) == sizeof(GenoTile), "one tile layout for the host table and the kernels");
  const int njobs = (int)nreg, ntiles = (int)tiles.size();
  HIPCHK(D.tiles.ensure(std::max<size_t>(tiles.size(), 1) * sizeof(GenoTile)));
  HIPCHK(D.state.ensure((size_t)njobs * sizeof(GenoState) + 256));
  D.stats.bytes = (int64_t)(D.acc.cap + D.dist.cap + D.tiles.cap + D.state.cap);
  hipStream_t st = ctx->stream;
  if (ntiles) HIPCHK(copy_h2d(ctx, D.tiles.p, tiles.data(), tiles.size() * sizeof(GenoTile)));
  GenoState* d_st = D.state.as<GenoState>();
  unsigned int* d_bits = reinterpret_cast<unsigned int*>(D.state.as<uint8_t>() + (size_t)njobs * sizeof(GenoState));
  { Timer t(ctx, "depth_regions"); launch_geno_init32(d_st, njobs, d_bits, st); launch_geno_minmax32(d_depth, D.tiles.as<GenoTile>(), ntiles, d_st, st); }
  std::vector<GenoState> got((size_t)njobs);
  HIPCHK(copy_d2h(ctx, got.data(), d_st, (size_t)njobs * sizeof(GenoState)));
  HIPCHK(CTX_SYNC());
  for (int64_t i = 0; i < nreg; ++i) {
    const GenoState& g = got[(size_t)i];
    if (g.n == 0) continue;
    out[i].n = g.n; out[i].sum = (int64_t)g.sum; out[i].min = g.vmin; out[i].max = g.vmax;
  }
  D.stats.launches = 1 + (ntiles ? 1 : 0);
  D.stats.workgroups = ntiles;
  D.stats.ms = now_ms() - t0;
  return RSI_OK;
}

}  // namespace rsip

namespace {

// What rsi_hot_depth_summary and its hook share; the caller has entered the context and reset the mailbox.
int depth_summary_run(rsi_ctx* ctx, const int32_t* d_depth, int64_t n, int64_t span, rsi_depth_summary* out, int64_t* dist, int dist_cap) {
  rsi_ctx::Depth& D = ctx->depth;
  const int64_t bytes_held = D.stats.bytes;
  D.stats = rsi_depth_stats{};
  D.stats.bytes = bytes_held;
  memset(out, 0, sizeof(*out));
  out->n = n;
  const int nbins = dist ? std::min(dist_cap, kDepthBins) : 0;
  for (int k = 0; k < nbins; ++k) dist[k] = 0;
  if (n == 0) return RSI_OK;
  const double t0 = now_ms();
  for (hipEvent_t& e : D.ev) if (!e) HIPCHK(hipEventCreate(&e));
  HIPCHK(D.acc.ensure(sizeof(DepthAcc)));
  HIPCHK(D.dist.ensure((size_t)kDepthBins * 4));
  D.stats.bytes = (int64_t)(D.acc.cap + D.dist.cap + D.tiles.cap + D.state.cap);
  hipStream_t st = ctx->stream;
  DepthAcc acc{0ull, 0ull, 0ull, INT32_MAX, INT32_MIN};
  HIPCHK(copy_h2d(ctx, D.acc.p, &acc, sizeof(acc)));
  HIPCHK(hipMemsetAsync(D.dist.p, 0, (size_t)kDepthBins * 4, st));
  (void)hipEventRecord(D.ev[0], st);
  { Timer t(ctx, "depth_summary"); launch_depth_summary(d_depth, n, span, D.acc.as<DepthAcc>(), D.dist.as<unsigned int>(), st); }
  (void)hipEventRecord(D.ev[1], st);
  std::vector<unsigned int> bins((size_t)nbins);
  HIPCHK(copy_d2h(ctx, &acc, D.acc.p, sizeof(acc)));
  if (nbins) HIPCHK(copy_d2h(ctx, bins.data(), D.dist.p, (size_t)nbins * 4));
  HIPCHK(CTX_SYNC());
  D.stats.kernel_ms = elapsed_ms(D.ev[0], D.ev[1]);
  D.stats.launches = 1;
  D.stats.workgroups = (n + span - 1) / span;
  D.stats.ms = now_ms() - t0;
  out->negative = (int64_t)acc.negative;
  if (acc.negative) return fail(ctx, RSI_ERR_BAD_ARG, "negative depth: " + std::to_string(acc.negative) + " of " + std::to_string(n) + " values are below 0");
  out->sum = (int64_t)acc.sum;
  out->over = (int64_t)acc.over;
  out->min = acc.vmin; out->max = acc.vmax;
  for (int k = 0; k < nbins; ++k) dist[k] = bins[(size_t)k];
  return RSI_OK;
}

}  // namespace

namespace rsip {

// host values[n] into the context's input depth buffer, as rsi_hot_debug_track does; what every depth hook begins with
int depth_upload(rsi_ctx* ctx, const int32_t* values, int64_t n) {
  if (!ctx) return fail(ctx, RSI_ERR_BAD_ARG, "null context");
  if (n < 0 || n >= (1ll << 31) - 4096 || (n > 0 && !values)) return fail(ctx, RSI_ERR_BAD_ARG, "depth: bad array");
  HIPCHK(hipSetDevice(ctx->device));
  if (!ctx_enter(ctx)) return RSI_ERR_HIP;
  mailbox_reset(ctx);
  if (ctx->last_depth == ctx->in_depth.p) ctx->last_depth = nullptr;   // the last run's depth is about to be overwritten
  ctx->n_in = 0;
  if (n == 0) return RSI_OK;
  HIPCHK(ctx->in_depth.ensure((size_t)(n + 4) * 4));
  HIPCHK(hipMemcpyAsync(ctx->in_depth.p, values, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(CTX_SYNC());   // the caller's array is pageable: free again once this returns
  ctx->n_in = n;
  return RSI_OK;
}

}  // namespace rsip

extern "C" {

int rsi_hot_loaded_depth(rsi_ctx* ctx, const void** d_depth, int64_t* n) {
  if (!ctx || !d_depth || !n) return fail(ctx, RSI_ERR_BAD_ARG, "null argument");
  if (!ctx->in_depth.p || ctx->n_in <= 0) return fail(ctx, RSI_ERR_BAD_ARG, "depth: the context's input buffer holds no loaded depth");
  *d_depth = ctx->in_depth.p;
  *n = ctx->n_in;
  return RSI_OK;
}

int rsi_hot_depth_summary(rsi_ctx* ctx, const void* d_depth, int64_t n, rsi_depth_summary* out, int64_t* dist, int dist_cap) {
  if (!ctx || !out || n < 0 || n >= (1ll << 31) || (n > 0 && !d_depth) || dist_cap < 0) return fail(ctx, RSI_ERR_BAD_ARG, "depth: bad argument");
  HIPCHK(hipSetDevice(ctx->device));
  if (!ctx_enter(ctx)) return RSI_ERR_HIP;
  mailbox_reset(ctx);
  return depth_summary_run(ctx, static_cast<const int32_t*>(d_depth), n, kDepthSpan, out, dist, dist_cap);
}

int rsi_hot_depth_regions(rsi_ctx* ctx, const void* d_depth, int64_t n, int nreg, const int64_t* start, const int64_t* end, rsi_depth_region* out) {
  if (!ctx || n < 0 || n >= (1ll << 31) || (n > 0 && !d_depth) || nreg < 0 || (nreg > 0 && (!start || !end || !out)))
    return fail(ctx, RSI_ERR_BAD_ARG, "depth: bad argument");
  HIPCHK(hipSetDevice(ctx->device));
  if (!ctx_enter(ctx)) return RSI_ERR_HIP;
  mailbox_reset(ctx);
  return depth_region_records(ctx, static_cast<const int32_t*>(d_depth), n, nreg, start, end, 0, out);
}

int rsi_hot_last_depth_stats(const rsi_ctx* ctx, rsi_depth_stats* out) {
  if (!ctx || !out) return RSI_ERR_BAD_ARG;
  *out = ctx->depth.stats;
  return RSI_OK;
}

int rsi_hot_debug_depth_summary(rsi_ctx* ctx, const int32_t* values, int64_t n, int64_t span, rsi_depth_summary* out, int64_t* dist, int dist_cap) {
  if (!out || span < 0 || dist_cap < 0) return fail(ctx, RSI_ERR_BAD_ARG, "depth: bad argument");
  if (int rc = depth_upload(ctx, values, n)) return rc;
  return depth_summary_run(ctx, ctx->in_depth.as<int32_t>(), n, span > 0 ? span : kDepthSpan, out, dist, dist_cap);
}

int rsi_hot_debug_depth_regions(rsi_ctx* ctx, const int32_t* values, int64_t n, int tile, int nreg, const int64_t* start, const int64_t* end,
                                rsi_depth_region* out) {
  if (tile < 0 || nreg < 0 || (nreg > 0 && (!start || !end || !out))) return fail(ctx, RSI_ERR_BAD_ARG, "depth: bad argument");
  if (int rc = depth_upload(ctx, values, n)) return rc;
  return depth_region_records(ctx, ctx->in_depth.as<int32_t>(), n, nreg, start, end, tile, out);
}

}  // extern "C"
