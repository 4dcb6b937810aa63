// ingest.hip -- the depth of one chromosome from a text file (load_data_from_text, loaddata.cpp:496-517),
// built in HBM: the file's chunks come from the chunk source (chunk_source.h), plain, gzip or BGZF, and are
// parsed by kernels_io.hip; the sequential fallback loop.  Also rsi_hot_inflate_bgzf, the run entry points that load a text or
// take a device depth, and the exclude-BED reader.  What the other ingest units use of it: ingest_internal.h.
#include "chunk_source.h"
#include "ingest_internal.h"
#include "text_rules.h"

using namespace rsik;
using namespace rsip;
using namespace rsing;

namespace rsing {

// The sequential parse loop (the reference's rules in the reference's order), used when the device
// cannot prove that positions are strictly increasing.  named: "RNAME pos depth" lines of one chromosome (the genome
// reader's fallback): the name token and the blanks around it go first, lines without one are skipped.  cols (named cohort
// lines, "RNAME pos d1 ... dK"): the 1-based depth columns to keep; sample j's array is rd[j * stride, ...), and a column is
// what `iss >> pos >> d1 >> ... >> dc` leaves in dc (0 once an extraction has failed).  bed (named bedGraph lines, "RNAME start
// end d"): each line is read as the lines "RNAME p d", p = start + 1 .. end, in order; "track" and "browser"
// lines are skipped.  Every extraction is text_rules.h's, the device kernels' own.
void parse_depth_text_host(const char* p, size_t sz, int64_t size, std::vector<int32_t>& rd, rsi_text_stats* st, bool named,
                           const std::vector<int32_t>* cols, int64_t stride, bool bed) {
  const char* end = p + sz;
  auto blank = [](char c) { return rsitxt::is_blank((unsigned char)c); };
  // `iss >> v` on [q, e) into an int (i32) or a long long (bedGraph start and end)
  auto parse_int = [](const char*& q, const char* e, long long& v, bool i64 = false) {
    long long k = 0;
    const bool ok = i64 ? rsitxt::extract_i64(q, k, (long long)(e - q), v) : rsitxt::extract_i32(q, k, (long long)(e - q), v);
    q += k;
    return ok;
  };
  std::vector<long long> vals(cols ? (size_t)*std::max_element(cols->begin(), cols->end()) : 0);
  const char* q = p;
  while (q < end) {
    const char* eol = (const char*)memchr(q, '\n', (size_t)(end - q));
    if (!eol) eol = end;
    if (eol > q && *q != '#') {
      const char* c = q;
      const char* name = q;
      bool data = true;
      if (named) {
        while (c < eol && blank(*c)) ++c;
        name = c;
        while (c < eol && !blank(*c)) ++c;
        data = c > name;
      }
      if (bed && data) {
        const size_t nl = (size_t)(c - name);
        if ((nl == 5 && memcmp(name, "track", 5) == 0) || (nl == 7 && memcmp(name, "browser", 7) == 0)) data = false;
      }
      long long start = 0, stop = 0, d = 0;
      if (bed && data && parse_int(c, eol, start, true) && parse_int(c, eol, stop, true)) {
        parse_int(c, eol, d);
        const long long a = std::max(start, 0ll), b = stop;
        if (b > a) {   // positions a + 1 .. b; the first one >= size ends the file (loaddata.cpp:514)
          const long long hi = std::min(b, (long long)size - 1);
          if (hi > a) {
            std::fill(rd.begin() + a, rd.begin() + hi, (int32_t)d);
            st->lines += hi - a; st->stored += hi - a;
          }
          if (b >= size) { ++st->lines; ++st->beyond; break; }
        }
      }
      long long pos = 0;
      if (!bed && data) {   // a failed pos is 0 or clamped (INT_MIN: skipped, INT_MAX: the end) and leaves d at 0
        const bool ok = parse_int(c, eol, pos);
        const char* after_pos = c;
        if (ok) parse_int(c, eol, d);
        if (pos >= 1) {
          ++st->lines;
          if (pos >= size) { ++st->beyond; break; }       // loaddata.cpp:514
          if (cols) {
            bool good = true;
            for (long long& v : vals) { v = 0; if (good) good = parse_int(after_pos, eol, v); }
            for (size_t j = 0; j < cols->size(); ++j) rd[(size_t)j * (size_t)stride + (size_t)pos - 1] = (int32_t)vals[(size_t)(*cols)[j] - 1];
          } else {
            rd[(size_t)pos - 1] = (int32_t)d;
          }
          ++st->stored;
        }
      }
    }
    q = eol + 1;
  }
}

// The context's two chunk buffers, pinned and in HBM: the staging of the text and BAM loaders, kept from load to load
int ctx_staging(rsi_ctx* ctx) {
  if (ctx->text_pin_cap < kTextChunk) {
    for (int b = 0; b < 2; ++b) {
      if (ctx->text_pin[b]) (void)hipHostFree(ctx->text_pin[b]);
      ctx->text_pin[b] = nullptr;
      if (hipHostMalloc(reinterpret_cast<void**>(&ctx->text_pin[b]), kTextChunk, hipHostMallocDefault) != hipSuccess)
        return fail(ctx, RSI_ERR_INTERNAL, "out of pinned host memory for the staging buffers");
    }
    ctx->text_pin_cap = kTextChunk;
  }
  HIPCHK(ctx->text_dev[0].ensure(kTextChunk));
  HIPCHK(ctx->text_dev[1].ensure(kTextChunk));
  return RSI_OK;
}

// The sequence of a run that loaded its depth itself: the host's bytes go to the context's buffer; a device pointer (the
// _dfasta entry points) is used where it is
int upload_fasta(rsi_ctx* ctx, const uint8_t* fasta, int64_t n) {
  HIPCHK(ctx->in_fasta.ensure((size_t)n + 64));
  HIPCHK(hipMemcpyAsync(ctx->in_fasta.p, fasta, (size_t)n, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return RSI_OK;
}

}  // namespace rsing

namespace {
// rsi_hot_run_text and rsi_hot_run_text_dfasta: exactly one of fasta (host) and d_fasta (HBM) is set
int run_text(rsi_ctx* ctx, const rsi_params* p, const char* depth_path, const uint8_t* fasta, const void* d_fasta, int64_t n, rsi_result** out,
             rsi_text_stats* stats) {
  ExcludeOneShot one_shot(ctx);
  if (!ctx || !p || !depth_path || (!fasta && !d_fasta) || !out) return fail(ctx, RSI_ERR_BAD_ARG, "null argument");
  ctx->ktimes.clear(); ctx->event_next = 0;
  int rc = rsi_hot_load_depth_text(ctx, depth_path, n, stats);
  if (rc != RSI_OK) return rc;
  if (fasta && (rc = upload_fasta(ctx, fasta, n)) != RSI_OK) return rc;
  return rsi_hot_run_device(ctx, p, ctx->in_depth.p, fasta ? ctx->in_fasta.p : d_fasta, n, out);
}
}  // namespace

extern "C" {

int rsi_hot_load_depth_text(rsi_ctx* ctx, const char* path, int64_t n, rsi_text_stats* stats) {
  rsi_text_stats local;
  rsi_text_stats* st = stats ? stats : &local;
  memset(st, 0, sizeof(*st));
  if (!ctx || !path) return fail(ctx, RSI_ERR_BAD_ARG, "null argument");
  ctx->last_inflate = rsi_inflate_stats{};
  if (n <= 0 || n >= (1ll << 31) - 4096) return fail(ctx, RSI_ERR_BAD_ARG, "chromosome length must be in (0, 2^31)");
  const double t0 = now_ms();
  HIPCHK(hipSetDevice(ctx->device));
  ChunkSource src;
  struct StatsOut { rsi_ctx* c; const ChunkSource& s; ~StatsOut() { c->last_inflate = s.st; } } stats_out{ctx, src};   // every return
  if (int rc = src.open_(path)) return fail(ctx, rc, src.err);
  st->bytes = src.file_size;
  if (!ctx_enter(ctx)) return RSI_ERR_HIP;
  mailbox_reset(ctx);
  HIPCHK(ctx->in_depth.ensure((size_t)(n + 4) * 4));
  HIPCHK(hipMemsetAsync(ctx->in_depth.p, 0, (size_t)n * 4, ctx->stream));
  ctx->n_in = n;
  if (int rc = ctx_staging(ctx)) return rc;
  src.borrow(ctx->text_pin[0], ctx->text_pin[1], ctx->text_dev[0].p, ctx->text_dev[1].p, kTextChunk);
  if (src.format == 1) src.carry_max = kTextChunk / 2;   // no room past the chunk in text_dev: the tail and a member fit in it
  const int max_wg = text_parse_workgroups((long long)kTextChunk);
  HIPCHK(ctx->text_wg.ensure((size_t)max_wg * 16 * 2 + 256));   // (first, max) per workgroup, two chunks in flight, + stats
  uint8_t* wgbase = ctx->text_wg.as<uint8_t>();
  TextParseStats* d_stats = reinterpret_cast<TextParseStats*>(wgbase + (size_t)max_wg * 32);
  HIPCHK(hipMemsetAsync(d_stats, 0, sizeof(TextParseStats), ctx->stream));
  std::vector<long long> wg_host[2];
  wg_host[0].resize((size_t)max_wg * 2); wg_host[1].resize((size_t)max_wg * 2);

  // Double buffering: while the device parses chunk k the source fills the other buffer with chunk k+1 (text and gzip:
  // read on the host once chunk k-1 there is through; BGZF: inflated on the device behind chunk k's parse).
  bool unsorted = false;
  long long run_max = -1;      // largest position seen in the chunks checked so far
  int inflight_wgs[2] = {0, 0};
  bool used[2] = {false, false};
  hipEvent_t done[2] = {nullptr, nullptr};
  for (int b = 0; b < 2; ++b) if (hipEventCreateWithFlags(&done[b], hipEventDisableTiming) != hipSuccess) return fail(ctx, RSI_ERR_HIP, "hipEventCreate failed");
  struct EvGuard { hipEvent_t* e; ~EvGuard() { for (int b = 0; b < 2; ++b) if (e[b]) (void)hipEventDestroy(e[b]); } } evguard{done};
  auto retire = [&](int b) {   // a parsed chunk: its buffer is free again, and the cross-workgroup order is checked
    if (!used[b]) return hipSuccess;
    const hipError_t e = hipEventSynchronize(done[b]);
    const long long* f = wg_host[b].data();
    const long long* m = f + inflight_wgs[b];
    for (int w = 0; w < inflight_wgs[b]; ++w) {
      if (f[w] < 0) continue;
      if (run_max >= 0 && f[w] <= run_max) unsorted = true;
      run_max = m[w] > run_max ? m[w] : run_max;
    }
    used[b] = false;
    return e;
  };
  for (int cur = 0;; cur ^= 1) {
    HIPCHK(retire(cur));
    if (int rc = src.fill(cur, ctx->stream)) return fail(ctx, rc, src.err);
    if (src.len[cur] == 0) break;
    if (src.format == 1) {   // the inflate's report comes back with the one wait per chunk, which also ends the chunk before
      HIPCHK(CTX_SYNC());
      HIPCHK(retire(cur ^ 1));
      if (int rc = src.cut(cur)) return fail(ctx, rc, src.err);
    }
    const int nwg = text_parse_workgroups((long long)src.len[cur]);
    long long* d_first = reinterpret_cast<long long*>(wgbase + (size_t)cur * max_wg * 16);
    long long* d_max = d_first + nwg;
    HIPCHK(src.upload(cur, ctx->stream));
    { Timer t(ctx, "parse_depth_text"); launch_parse_depth_text(ctx->text_dev[cur].p, (long long)src.len[cur], (long long)n, ctx->in_depth.as<int32_t>(), d_first, d_max, d_stats, ctx->stream); }
    HIPCHK(hipMemcpyAsync(wg_host[cur].data(), d_first, (size_t)nwg * 16, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipEventRecord(done[cur], ctx->stream));
    inflight_wgs[cur] = nwg;
    used[cur] = true;
  }
  for (int b = 0; b < 2; ++b) HIPCHK(retire(b));
  if (src.format != 0) st->bytes = src.st.text_bytes;
  TextParseStats hs;
  HIPCHK(hipMemcpyAsync(&hs, d_stats, sizeof(hs), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  st->lines = (int64_t)hs.lines; st->stored = (int64_t)hs.stored; st->beyond = (int64_t)hs.beyond;
  if (hs.unsorted || unsorted) {
    // order-dependent rules in play: redo the file with the sequential loop
    st->fallback = 1; st->lines = st->stored = st->beyond = 0;
    std::vector<int32_t> rd((size_t)n, 0);
    std::vector<char> all;
    if (int rc = src.host_range(0, st->bytes, all)) return fail(ctx, rc, src.err);
    parse_depth_text_host(all.data(), all.size(), n, rd, st);
    HIPCHK(hipMemcpyAsync(ctx->in_depth.p, rd.data(), (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
  }
  st->t_total_ms = now_ms() - t0;
  if (ctx->timing) { double tot = 0; for (const KernelTime& k : ctx->ktimes) tot += elapsed_ms(k.a, k.b); st->t_parse_kernel_ms = tot; }
  return RSI_OK;
}

int rsi_hot_last_inflate_stats(const rsi_ctx* ctx, rsi_inflate_stats* out) {
  if (!ctx || !out) return RSI_ERR_BAD_ARG;
  *out = ctx->last_inflate;
  return RSI_OK;
}

int64_t rsi_hot_inflate_bgzf(rsi_ctx* ctx, const uint8_t* comp, int64_t comp_len, uint8_t* out, int64_t out_cap, rsi_inflate_stats* stats) {
  if (!ctx || comp_len < 0 || out_cap < 0 || (!comp && comp_len) || (!out && out_cap)) return fail(ctx, RSI_ERR_BAD_ARG, "null argument");
  rsi_inflate_stats st{};
  st.format = 1; st.compressed_bytes = comp_len;
  std::vector<InflateBlock> tab;
  std::vector<int64_t> starts;   // member offsets (messages)
  int64_t text = 0;
  for (int64_t p = 0; p < comp_len;) {   // the member headers, on the host
    rsinf::Member m;
    const std::string bad = bgzf_member_error(comp + p, (size_t)(comp_len - p), p, m);
    if (!bad.empty()) return fail(ctx, RSI_ERR_BAD_ARG, bad);
    tab.push_back(InflateBlock{(long long)(p + m.hdr), (long long)text, m.clen, m.isize, m.crc, 0});
    starts.push_back(p);
    text += m.isize; p += m.bsize;
    st.eof_block = m.isize == 0;
  }
  st.blocks = (int64_t)tab.size(); st.text_bytes = text;
  if (text > out_cap) return fail(ctx, RSI_ERR_BAD_ARG, "rsi_hot_inflate_bgzf: out_cap is smaller than the text (" + std::to_string(text) + " bytes)");
  HIPCHK(hipSetDevice(ctx->device));
  if (!ctx_enter(ctx)) return RSI_ERR_HIP;
  constexpr int64_t kBatch = int64_t(256) << 20;   // text bytes per launch
  DevBuf dcomp, dtext;
  BgzfLaunch& launch = ctx->inflate;
  hipEvent_t ea = nullptr, eb = nullptr;
  if (hipEventCreate(&ea) != hipSuccess || hipEventCreate(&eb) != hipSuccess) return fail(ctx, RSI_ERR_HIP, "hipEventCreate failed");
  struct EvGuard { hipEvent_t a, b; ~EvGuard() { (void)hipEventDestroy(a); (void)hipEventDestroy(b); } } evguard{ea, eb};
  for (size_t i = 0; i < tab.size();) {
    size_t j = i;
    const int64_t t0 = tab[i].out, cbase = tab[i].coff;
    while (j < tab.size() && (j == i || tab[j].out + tab[j].isize - t0 <= kBatch)) ++j;
    const int64_t t1 = tab[j - 1].out + tab[j - 1].isize, c1 = tab[j - 1].coff + tab[j - 1].clen;
    std::vector<InflateBlock> part(tab.begin() + (ptrdiff_t)i, tab.begin() + (ptrdiff_t)j);
    for (InflateBlock& B : part) { B.coff -= cbase; B.out -= t0; }
    HIPCHK(dcomp.ensure((size_t)(c1 - cbase) + 16));
    HIPCHK(dtext.ensure((size_t)(t1 - t0) + 16));
    HIPCHK(launch.reserve(part.size()));
    HIPCHK(launch.queue(part, comp + cbase, (size_t)(c1 - cbase), dcomp.p, dtext.p, -1, ctx->stream, ea, eb));
    if (t1 > t0) HIPCHK(hipMemcpyAsync(out + t0, dtext.p, (size_t)(t1 - t0), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(CTX_SYNC());
    const BgzfLaunch::Result r = launch.result();
    st.t_inflate_kernel_ms += r.kernel_ms;
    if (!r.ok) {
      const size_t k = i + r.member;
      const int64_t at = k < starts.size() ? starts[k] : -1;
      ctx->last_inflate = st;
      return fail(ctx, RSI_ERR_BAD_ARG, "BGZF: the member at compressed offset " + std::to_string(at) + " is bad: " + rsinf::err_name(r.error));
    }
    i = j;
  }
  ctx->last_inflate = st;
  if (stats) *stats = st;
  return text;
}

int rsi_hot_run_text(rsi_ctx* ctx, const rsi_params* p, const char* depth_path, const uint8_t* fasta, int64_t n, rsi_result** out,
                     rsi_text_stats* stats) {
  return run_text(ctx, p, depth_path, fasta, nullptr, n, out, stats);
}
int rsi_hot_run_text_dfasta(rsi_ctx* ctx, const rsi_params* p, const char* depth_path, const void* d_fasta, int64_t n, rsi_result** out,
                            rsi_text_stats* stats) {
  return run_text(ctx, p, depth_path, nullptr, d_fasta, n, out, stats);
}

int rsi_hot_run_depth_device(rsi_ctx* ctx, const rsi_params* p, const void* d_depth, const uint8_t* fasta, int64_t n, rsi_result** out) {
  ExcludeOneShot one_shot(ctx);
  if (!ctx || !p || !d_depth || !fasta || !out) return fail(ctx, RSI_ERR_BAD_ARG, "null argument");
  if (n <= 0) return fail(ctx, RSI_ERR_BAD_ARG, "empty chromosome");
  if (!ctx_enter(ctx)) return RSI_ERR_HIP;
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(ctx->in_fasta.ensure((size_t)n + 64));
  HIPCHK(hipMemcpyAsync(ctx->in_fasta.p, fasta, (size_t)n, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(CTX_SYNC());
  return rsi_hot_run_device(ctx, p, d_depth, ctx->in_fasta.p, n, out);
}

// Exclusion masks as BED files (include/rsi_hot.h): host only.  Every line that is not blank, a comment or a track / browser
// line must be a good BED line, whichever sequence it names: a typo in a mask file is reported, never skipped.
int rsi_exclude_read_bed(const char* path, const char* chrom, int64_t n, int64_t* start, int64_t* end, int cap) {
  if (!path || !chrom || n < 0) { set_global_error("rsi_exclude_read_bed: bad argument"); return RSI_ERR_BAD_ARG; }
  gzFile gz = gzopen(path, "rb");
  if (!gz) { set_global_error(std::string("cannot open the exclusion BED file ") + path); return RSI_ERR_BAD_ARG; }
  const std::string want(chrom);
  auto same_name = [&](const std::string& x) {   // read_fasta's rule, in either direction
    return x == want || "chr" + x == want || x == "chr" + want;
  };
  auto coord = [](const std::string& t, long long* v) {   // a whole token of digits that fits a long long
    if (t.empty() || t.size() > 19) return false;
    for (char c : t) if (c < '0' || c > '9') return false;
    errno = 0;
    *v = strtoll(t.c_str(), nullptr, 10);
    return errno == 0;
  };
  std::vector<std::pair<int64_t, int64_t>> iv;
  std::string line, bad;
  std::vector<char> buf(1 << 16);
  long long lineno = 0;
  bool more = true;
  while (more && bad.empty()) {
    line.clear();
    bool got = false;
    for (;;) {   // one line, however long
      if (!gzgets(gz, buf.data(), (int)buf.size())) { more = false; break; }
      got = true;
      line += buf.data();
      if (!line.empty() && line.back() == '\n') break;
    }
    if (!got) break;
    ++lineno;
    while (!line.empty() && (line.back() == '\n' || line.back() == '\r')) line.pop_back();
    std::string tok[3];
    int nt = 0;
    for (size_t i = 0; i < line.size() && nt < 3;) {
      while (i < line.size() && (line[i] == ' ' || line[i] == '\t')) ++i;
      const size_t b = i;
      while (i < line.size() && line[i] != ' ' && line[i] != '\t') ++i;
      if (i > b) tok[nt++] = line.substr(b, i - b);
    }
    if (nt == 0 || tok[0][0] == '#' || tok[0] == "track" || tok[0] == "browser") continue;
    long long a = 0, b = 0;
    const std::string where = std::string(path) + ": line " + std::to_string(lineno) + ": ";
    if (nt < 3) bad = where + "fewer than three fields";
    else if (!coord(tok[1], &a) || !coord(tok[2], &b)) bad = where + "start and end must be non-negative integers";
    else if (b <= a) bad = where + "end <= start";
    else if (same_name(tok[0])) iv.push_back({(int64_t)a, (int64_t)b});
  }
  int zerr = 0;
  const char* zmsg = gzerror(gz, &zerr);
  if (bad.empty() && zerr != Z_OK && zerr != Z_STREAM_END) bad = std::string(path) + ": " + (zmsg ? zmsg : "read error");
  gzclose(gz);
  if (!bad.empty()) { set_global_error(bad); return RSI_ERR_BAD_ARG; }
  normalize_intervals(iv, n);
  if (iv.size() > (size_t)0x7fffffff) { set_global_error(std::string(path) + ": too many intervals"); return RSI_ERR_UNSUPPORTED; }
  if (start && end) for (size_t i = 0; i < iv.size() && (int64_t)i < (int64_t)cap; ++i) { start[i] = iv[i].first; end[i] = iv[i].second; }
  return (int)iv.size();
}

}  // extern "C"
