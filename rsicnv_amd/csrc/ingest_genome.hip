// ingest_genome.hip -- the whole-genome depth reader, rsi_genome_text and its C entry points (cohort files 6c,
// bedGraph 6d, a BGZF bedGraph read by index 6i).  Its chunks come from the chunk source (chunk_source.h).
// Whole-genome depth text ("RNAME pos depth", every chromosome in one file): a streaming reader that hands over each
// chromosome's depth, resident in HBM, once its last line has been parsed, so that the caller can run it while the next one
// is being parsed.  Per chunk of the file: one transfer, the boundary pass (kernels_io.hip, k_text_name_bounds), ONE small
// read-back (the chunk's name changes and the counts of the chromosomes closed in the chunk before), then parse launches
// over the chunk's segments -- each new name resolved to a depth buffer by the host in between.  Every chromosome's lines
// give what its slice (its lines without the name) gives through rsi_hot_load_depth_text: same rules, same order proof
// (per chromosome), same fallback to the sequential loop (over that chromosome's bytes only).
#include "chunk_source.h"
#include "ingest_internal.h"
#include <memory>
#include <unordered_set>

using namespace rsik;
using namespace rsip;
using namespace rsing;

struct rsi_genome_text {
  struct Chrom { std::string name; int slot = -1; int64_t n = 0, start = 0, end = 0; double t0 = 0; bool report = true; };
  struct Pending { hipEvent_t a, b; bool parse; };
  int device = 0;
  hipStream_t stream = nullptr;
  hipEvent_t sync_ev = nullptr;
  std::string err;
  std::vector<std::string> ref_names;
  std::vector<int64_t> ref_len;
  int max_resident = 1;
  size_t chunk = 0;
  unsigned bound_cap = 0, seg_cap = 0;
  char* pin[2] = {nullptr, nullptr};
  DevBuf text_dev[2], dread, dsegs, dwg;
  PinBuf hread, hsegs;
  size_t slots_bytes = 0;                // dread / hread: GenomeSlotStats[max_resident], then the count, then NameBound[bound_cap]
  std::unique_ptr<DevBuf[]> slot_buf;
  std::vector<int> slot_state;           // 0 free, 1 the reader's, 2 handed to the caller
  std::vector<Chrom> awaiting;           // closed, their counts not read back yet (first-appearance order)
  std::vector<rsi_genome_chrom> ready;   // complete, in order; handed out from the front
  size_t ready_head = 0;
  Chrom open;
  bool open_valid = false;
  std::unordered_set<std::string> seen;  // every name met so far (contiguity)
  std::vector<int64_t> slot_n;           // length of the chromosome in each depth buffer
  int cur = 0;
  bool active = false, prefetched = false, done = false, failed = false;
  std::vector<NameBound> bounds;
  std::vector<std::string> bnames;
  size_t cursor = 0, seg_used = 0;
  long long range_start = 0;
  std::vector<Pending> timed;
  std::vector<hipEvent_t> ev_free;
  double ms_bound = 0, ms_parse = 0;
  ChunkSource src;                       // the file, its chunks in pin[b] / text_dev[b], their cuts and offsets
  DevBuf dnames;                         // BGZF: the boundary entries' names (launch_gather_names) and their pinned copy
  PinBuf hnames;
  hipStream_t istream = nullptr;         // BGZF: the next chunk's uploads and inflate run here, beside the parse of this one
  hipEvent_t iev = nullptr;              // ... recorded behind them; the boundary pass of that chunk waits for it
  // cohort files (rsi_genome_text_open_samples): the selected depth columns, in the caller's order (sample j = cols[j]); a depth
  // buffer holds every sample of its chromosome, sample j at j * genome_sample_stride(n), and is allocated once at its full size
  bool samples = false;
  // bedGraph files (rsi_genome_bedgraph_open): the interval passes, and the run list they hand long runs to
  bool bed = false;
  DevBuf druns;                          // unsigned long long count (256 bytes), then BedRun[run_cap]
  unsigned run_cap = 0;
  std::vector<int32_t> cols{1};
  GenomeSampleCols scols{};              // the kernel's view: ascending columns and their samples
  size_t sample_slot_bytes = 0;          // ncols * stride(longest .fai length) * 4

  int ncols() const { return (int)cols.size(); }
  int64_t sample_stride(int slot) const { return samples ? genome_sample_stride(slot_n[(size_t)slot]) : 0; }

  ~rsi_genome_text() {
    if (stream && sync_ev) (void)stream_wait(stream, sync_ev);   // nothing may still write the buffers freed below (deadline as every wait)
    if (istream && iev) (void)stream_wait(istream, iev);
    if (iev) (void)hipEventDestroy(iev);
    if (istream) (void)hipStreamDestroy(istream);
    for (auto& t : timed) { ev_free.push_back(t.a); ev_free.push_back(t.b); }
    for (hipEvent_t e : ev_free) (void)hipEventDestroy(e);
    for (int b = 0; b < 2; ++b) if (pin[b]) (void)hipHostFree(pin[b]);
    if (sync_ev) (void)hipEventDestroy(sync_ev);
    if (stream) (void)hipStreamDestroy(stream);
  }
  int fail_(int code, const std::string& m) { err = m; failed = true; set_global_error(m); return code; }
  int hip_(hipError_t e, const char* what) { return e == hipSuccess ? RSI_OK : fail_(RSI_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e)); }
  GenomeSlotStats* h_slots() { return hread.as<GenomeSlotStats>(); }
  unsigned* h_count() { return reinterpret_cast<unsigned*>(hread.as<char>() + slots_bytes); }
  NameBound* h_bounds() { return reinterpret_cast<NameBound*>(hread.as<char>() + slots_bytes + 16); }
  unsigned* d_count() { return reinterpret_cast<unsigned*>(dread.as<char>() + slots_bytes); }
  NameBound* d_bounds() { return reinterpret_cast<NameBound*>(dread.as<char>() + slots_bytes + 16); }

  hipEvent_t event() {
    if (!ev_free.empty()) { hipEvent_t e = ev_free.back(); ev_free.pop_back(); return e; }
    hipEvent_t e = nullptr;
    return hipEventCreate(&e) == hipSuccess ? e : nullptr;
  }
  // every wait: the project's deadline (stream_wait) and the launch errors of the chain in front of it
  int wait() {
    hipError_t e = stream_wait(stream, sync_ev);
    const hipError_t launch = take_launch_error();
    if (e == hipSuccess) e = launch;
    if (e == hipErrorLaunchTimeOut) return fail_(RSI_ERR_HIP, "genome text: a wait gave up after 60 s with kernels still queued");
    if (e != hipSuccess) return hip_(e, "genome text");
    for (const Pending& t : timed) {
      (t.parse ? ms_parse : ms_bound) += elapsed_ms(t.a, t.b);
      ev_free.push_back(t.a); ev_free.push_back(t.b);
    }
    timed.clear();
    seg_used = 0;   // the segment tables' transfers are through
    return RSI_OK;
  }

  int find_ref(const std::string& x) const {   // read_fasta's rule (readref.cpp): name == X || name == "chr" + X
    for (size_t i = 0; i < ref_names.size(); ++i) if (ref_names[i] == x || ref_names[i] == "chr" + x) return (int)i;
    return -1;
  }

  // The next chunk into buffer b.  BGZF: the tail of the chunk before moves device to device and the next members are
  // inflated behind it, on istream: text_dev[b]'s chunk before was parsed before the last wait, so the inflate overlaps the
  // parse launches of the chunk in text_dev[b ^ 1] (which it only reads, for the tail).  start_chunk cuts it once the
  // inflate's report is back.
  int fill(int b) {
    if (int rc = src.fill(b, istream)) return fail_(rc, src.err);
    return src.format == 1 ? hip_(hipEventRecord(iev, istream), "hipEventRecord") : RSI_OK;
  }

  // counts of the closed chromosomes are in hread: hand them over (in order), the unsorted ones through the sequential loop
  int finalize_awaiting() {
    for (Chrom& c : awaiting) {
      rsi_genome_chrom o;
      memset(&o, 0, sizeof(o));
      o.slot = c.slot; o.n = c.n;
      snprintf(o.name, sizeof(o.name), "%s", c.name.c_str());
      o.stats.bytes = c.end - c.start;
      if (c.slot >= 0) {
        const GenomeSlotStats& S = h_slots()[c.slot];
        o.d_depth = slot_buf[(size_t)c.slot].p;
        o.stats.lines = (int64_t)S.lines; o.stats.stored = (int64_t)S.stored; o.stats.beyond = (int64_t)S.beyond;
        if (S.unsorted) {   // order-dependent rules in play: this chromosome's bytes through the sequential loop
          o.stats.fallback = 1; o.stats.lines = o.stats.stored = o.stats.beyond = 0;
          std::vector<char> text;
          if (int rc = src.host_range(c.start, c.end, text)) return fail_(rc, src.err);
          const int64_t stride = samples ? genome_sample_stride(c.n) : c.n;
          std::vector<int32_t> rd((size_t)(samples ? ncols() * stride : c.n), 0);
          parse_depth_text_host(text.data(), text.size(), c.n, rd, &o.stats, true, samples ? &cols : nullptr, stride, bed);
          if (int rc = hip_(hipMemcpyAsync(slot_buf[(size_t)c.slot].p, rd.data(), rd.size() * 4, hipMemcpyHostToDevice, stream), "hipMemcpyAsync")) return rc;
          if (int rc = wait()) return rc;
        }
      }
      o.stats.t_total_ms = now_ms() - c.t0;
      ready.push_back(o);
    }
    awaiting.clear();
    return RSI_OK;
  }
  int sync_counts() {   // read the depth buffers' counts back (only when no chunk read-back is coming to carry them)
    if (int rc = hip_(hipMemcpyAsync(hread.p, dread.p, slots_bytes, hipMemcpyDeviceToHost, stream), "hipMemcpyAsync")) return rc;
    if (int rc = wait()) return rc;
    return finalize_awaiting();
  }

  void close_open(int64_t end_off) {
    if (!open_valid) return;
    open.end = end_off;
    if (open.report) awaiting.push_back(open);
    open_valid = false;
  }

  // The boundary pass over the chunk in buffer b and its one read-back.  BGZF: the pass runs over all the inflated text, the
  // unfinished last line too, and the read-back also brings the inflate's report; the source cuts the chunk there and the
  // entries behind the cut are dropped.  More name changes than the list holds: the chunk is cut shorter at a line end, the
  // rest given back to the source for the next chunk, and the pass repeats.  The names come from the pinned text, or for
  // BGZF back from the device (launch_gather_names, 4096 at a time).
  int start_chunk(int b) {
    const bool in_hbm = src.format == 1;   // BGZF: the text exists only in text_dev[b]
    if (in_hbm) { if (int rc = hip_(hipStreamWaitEvent(stream, iev, 0), "hipStreamWaitEvent")) return rc; }   // the chunk's inflate (fill)
    else if (int rc = hip_(src.upload(b, stream), "hipMemcpyAsync")) return rc;
    const size_t first = std::min<size_t>(bound_cap, 4096);
    for (bool once = true;; once = false) {
      if (int rc = hip_(hipMemsetAsync(d_count(), 0, 16, stream), "hipMemsetAsync")) return rc;
      hipEvent_t a = event(), e = event();
      if (a) (void)hipEventRecord(a, stream);
      launch_text_name_bounds(text_dev[b].p, (long long)src.len[b], d_bounds(), d_count(), bound_cap, stream, bed);
      if (a && e) { (void)hipEventRecord(e, stream); timed.push_back({a, e, false}); }
      if (int rc = hip_(hipMemcpyAsync(hread.p, dread.p, slots_bytes + 16 + first * sizeof(NameBound), hipMemcpyDeviceToHost, stream), "hipMemcpyAsync")) return rc;
      if (int rc = wait()) return rc;
      if (once) if (int rc = src.cut(b)) return fail_(rc, src.err);
      if (*h_count() <= bound_cap) break;
      const long long len = (long long)src.len[b];
      long long c = 0;
      if (!in_hbm) c = (long long)src.line_cut(b, (size_t)len / 2);   // the last line end in the first half
      else {   // the first listed line start in the second half, else the last one in the first half
        long long hi = -1;
        for (size_t i = 0; i < first; ++i) {
          const long long l = h_bounds()[i].line;
          if (l <= 0 || l >= len) continue;
          if (2 * l >= len) hi = hi < 0 ? l : std::min(hi, l);
          else c = std::max(c, l);
        }
        if (hi > 0) c = hi;
      }
      if (c <= 0) return fail_(RSI_ERR_INTERNAL, "genome text: no line end to cut a chunk shorter at");
      if (int rc = src.give_back(b, (size_t)c)) return fail_(rc, src.err);
    }
    const unsigned k = *h_count();
    if (k > first) {
      if (int rc = hip_(hipMemcpyAsync(h_bounds() + first, d_bounds() + first, (k - first) * sizeof(NameBound), hipMemcpyDeviceToHost, stream), "hipMemcpyAsync")) return rc;
      if (int rc = wait()) return rc;
    }
    if (int rc = finalize_awaiting()) return rc;
    constexpr unsigned kWin = 4096;
    if (in_hbm) {
      if (int rc = hip_(dnames.ensure((size_t)kWin * 256), "hipMalloc")) return rc;
      if (int rc = hip_(hnames.ensure((size_t)kWin * 256), "hipHostMalloc")) return rc;
    }
    std::vector<std::pair<NameBound, std::string>> named;
    for (unsigned w0 = 0; w0 < k; w0 += kWin) {
      const unsigned w1 = std::min(k, w0 + kWin);
      if (in_hbm) {
        launch_gather_names(text_dev[b].p, d_bounds(), w0, w1, dnames.as<char>(), stream);
        if (int rc = hip_(hipMemcpyAsync(hnames.p, dnames.p, (size_t)(w1 - w0) * 256, hipMemcpyDeviceToHost, stream), "hipMemcpyAsync")) return rc;
        if (int rc = wait()) return rc;
      }
      for (unsigned i = w0; i < w1; ++i) {
        const NameBound& nb = h_bounds()[i];
        if (nb.line >= (long long)src.len[b]) continue;   // BGZF: behind the cut, parsed with the next chunk
        if (nb.len >= (int)sizeof(rsi_genome_chrom::name)) return fail_(RSI_ERR_UNSUPPORTED, "genome text: a chromosome name is longer than 255 bytes");
        const char* name = in_hbm ? hnames.as<char>() + (size_t)(i - w0) * 256 : src.pin[b] + nb.name;
        named.emplace_back(nb, std::string(name, (size_t)nb.len));
      }
    }
    std::sort(named.begin(), named.end(), [](const std::pair<NameBound, std::string>& x, const std::pair<NameBound, std::string>& y) { return x.first.line < y.first.line; });
    bounds.clear(); bnames.clear();
    for (auto& x : named) { bounds.push_back(x.first); bnames.push_back(std::move(x.second)); }
    cursor = 0; range_start = 0;
    return RSI_OK;
  }

  // Parse launches over the chunk from range_start on.  1: the chunk is through; 2: stopped at a new chromosome for want of a
  // free depth buffer (range_start / cursor point at it); < 0: error.
  int issue(int b) {
    const char* d_text = static_cast<const char*>(text_dev[b].p);
    for (;;) {
      const long long begin = range_start;
      long long end = (long long)src.len[b];
      GenomeSeg* segs = hsegs.as<GenomeSeg>() + seg_used;
      int nseg = 0;
      auto seg_of_open = [&](long long start) {
        const bool buf = open_valid && open.slot >= 0;
        return GenomeSeg{start, buf ? open.n : 0, buf ? slot_buf[(size_t)open.slot].as<int32_t>() : nullptr, buf ? open.slot : -1, 0};
      };
      segs[nseg++] = seg_of_open(begin);
      bool stalled = false;
      while (cursor < bounds.size()) {
        const NameBound& B = bounds[cursor];
        const std::string& name = bnames[cursor];
        if (open_valid && name == open.name) { ++cursor; continue; }   // the chunk's first data line, continuing the chromosome
        if (seen.count(name))
          return fail_(RSI_ERR_BAD_ARG, "genome text: the lines of chromosome " + name + " are not contiguous: it comes back at byte " +
                                              std::to_string(src.foff[b] + B.line) + " after other chromosomes");
        const bool filtered = name.find("MT") != std::string::npos || name.find('.') != std::string::npos;   // the BAM walk's filter
        const int ref = filtered ? -1 : find_ref(name);
        int slot = -1;
        if (ref >= 0) {
          for (int s = 0; s < max_resident; ++s) if (slot_state[(size_t)s] == 0) { slot = s; break; }
          if (slot < 0) {   // the open chromosome is complete at B: parse up to there, hand it over, resume here once a buffer is free
            close_open(src.foff[b] + B.line);
            end = B.line; stalled = true;
            break;
          }
        }
        if (nseg == kMaxGenomeSegs) { end = B.line; break; }
        close_open(src.foff[b] + B.line);
        open = Chrom();
        open.name = name; open.start = src.foff[b] + B.line; open.t0 = now_ms(); open.report = !filtered;
        open_valid = true;
        seen.insert(name);
        if (ref >= 0) {
          const int64_t n = ref_len[(size_t)ref];
          if (n <= 0 || n >= (1ll << 31) - 4096) return fail_(RSI_ERR_BAD_ARG, "chromosome length must be in (0, 2^31): " + name);
          DevBuf& d = slot_buf[(size_t)slot];
          const size_t bytes = samples ? (size_t)ncols() * (size_t)genome_sample_stride(n) * 4 : (size_t)(n + 4) * 4;
          if (int rc = hip_(d.ensure(samples ? sample_slot_bytes : bytes), "hipMalloc")) return rc;
          if (int rc = hip_(hipMemsetAsync(d.p, 0, bytes, stream), "hipMemsetAsync")) return rc;
          if (int rc = hip_(hipMemsetAsync(dread.as<GenomeSlotStats>() + slot, 0, sizeof(GenomeSlotStats), stream), "hipMemsetAsync")) return rc;
          slot_state[(size_t)slot] = 1;
          open.slot = slot; open.n = n; slot_n[(size_t)slot] = n;
        }
        if (segs[nseg - 1].start == B.line) segs[nseg - 1] = seg_of_open(B.line);
        else segs[nseg++] = seg_of_open(B.line);
        ++cursor;
      }
      if (end > begin) {
        GenomeSeg* d_segs = dsegs.as<GenomeSeg>() + seg_used;
        if (int rc = hip_(hipMemcpyAsync(d_segs, segs, (size_t)nseg * sizeof(GenomeSeg), hipMemcpyHostToDevice, stream), "hipMemcpyAsync")) return rc;
        seg_used += (size_t)nseg;
        hipEvent_t a = event(), e = event();
        if (a) (void)hipEventRecord(a, stream);
        if (bed) if (int rc = hip_(hipMemsetAsync(druns.p, 0, sizeof(unsigned long long), stream), "hipMemsetAsync")) return rc;
        launch_parse_genome(bed ? GenomeFormat::kBedgraph : samples ? GenomeFormat::kSamples : GenomeFormat::kText, d_text, begin, end, d_segs,
                            nseg, dread.as<GenomeSlotStats>(), dwg.as<long long>(), &scols,
                            bed ? reinterpret_cast<BedRun*>(druns.as<char>() + 256) : nullptr, druns.as<unsigned long long>(), run_cap, stream);
        if (a && e) { (void)hipEventRecord(e, stream); timed.push_back({a, e, true}); }
      }
      range_start = end;
      if (stalled) return 2;
      if (cursor == bounds.size() && end == (long long)src.len[b]) return 1;
    }
  }

  // one step: a chunk started, parsed as far as the depth buffers allow, the next one read from the file meanwhile
  int advance() {
    if (!active) {
      if (!prefetched) if (int rc = fill(cur)) return rc;
      prefetched = false;
      if (src.len[cur] == 0) {   // end of the file
        close_open(src.foff[cur]);
        if (int rc = sync_counts()) return rc;
        done = true;
        return RSI_OK;
      }
      if (int rc = start_chunk(cur)) return rc;
      active = true;
    }
    const int r = issue(cur);
    if (r < 0) return r;
    if (r == 1) {   // while the device parses this chunk, the next one comes off the disk
      active = false;
      if (int rc = fill(cur ^ 1)) return rc;
      prefetched = true;
      cur ^= 1;
      return RSI_OK;
    }
    if (!awaiting.empty()) return sync_counts();   // stalled: hand over what is complete, so that the caller can release
    return fail_(RSI_ERR_BAD_ARG, "genome text: every depth buffer (max_resident = " + std::to_string(max_resident) +
                                      ") is held by the caller: release one before asking for the next chromosome");
  }
};

namespace {

// rsi_genome_text_open (cols == nullptr), rsi_genome_text_open_samples and rsi_genome_bedgraph_open (bed)
rsi_genome_text* genome_text_open(const char* fn, int device, const char* path, int nref, const char* const* names, const int64_t* lengths,
                                  const int32_t* cols, int ncols, int max_resident, size_t chunk_bytes, int* status, bool bed = false,
                                  const char* index_path = nullptr) {
  int st_local = 0;
  int* st = status ? status : &st_local;
  *st = RSI_OK;
  try {
    if (!path || nref < 0 || (nref > 0 && (!names || !lengths)) || max_resident < 1) { set_global_error(std::string(fn) + ": bad argument"); *st = RSI_ERR_BAD_ARG; return nullptr; }
    if (chunk_bytes != 0 && (chunk_bytes < 64 || chunk_bytes > (size_t(1) << 30))) { set_global_error(std::string(fn) + ": chunk_bytes must be 0 or in [64, 2^30]"); *st = RSI_ERR_BAD_ARG; return nullptr; }
    std::unique_ptr<rsi_genome_text> g(new rsi_genome_text());
    auto bad = [&](int code) { *st = code; return nullptr; };
    if (cols) {   // 1-based, distinct, 1..64 of them
      if (ncols < 1 || ncols > kMaxGenomeSamples) { set_global_error(std::string(fn) + ": ncols must be in [1, 64]"); return bad(RSI_ERR_BAD_ARG); }
      std::vector<std::pair<int32_t, int32_t>> order;
      for (int j = 0; j < ncols; ++j) order.emplace_back(cols[j], j);
      std::sort(order.begin(), order.end());
      for (int i = 0; i < ncols; ++i)
        if (order[(size_t)i].first < 1 || (i && order[(size_t)i].first == order[(size_t)i - 1].first)) {
          set_global_error(std::string(fn) + ": the depth columns must be distinct and 1-based");
          return bad(RSI_ERR_BAD_ARG);
        }
      g->samples = true;
      g->cols.assign(cols, cols + ncols);
      g->scols.n = ncols;
      for (int i = 0; i < ncols; ++i) { g->scols.col[i] = order[(size_t)i].first; g->scols.j[i] = order[(size_t)i].second; }
    }
    g->device = device; g->max_resident = max_resident; g->bed = bed;
    g->chunk = chunk_bytes ? chunk_bytes : kTextChunk;
    for (int i = 0; i < nref; ++i) { g->ref_names.emplace_back(names[i] ? names[i] : ""); g->ref_len.push_back(lengths[i]); }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { set_global_error("no HIP device: rsicnv_amd has no CPU fallback"); return bad(RSI_ERR_NO_DEVICE); }
    if (device < 0 || device >= ndev) { set_global_error(std::string(fn) + ": no such device"); return bad(RSI_ERR_BAD_ARG); }
    if (hipSetDevice(device) != hipSuccess) { set_global_error("hipSetDevice failed"); return bad(RSI_ERR_HIP); }
    drain_stale_errors();
    if (g->samples) {   // every depth buffer is allocated at the longest sequence's size: at least two must fit
      int64_t longest = 1;
      for (int64_t n : g->ref_len) if (n > 0 && n < (1ll << 31) - 4096) longest = std::max(longest, n);
      const size_t bytes = (size_t)ncols * (size_t)genome_sample_stride(longest) * 4;
      g->sample_slot_bytes = bytes;
      const size_t alloc = bytes + bytes / 8 + 256;   // what DevBuf::ensure asks for
      size_t free_b = 0, total_b = 0;
      if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { set_global_error("hipMemGetInfo failed"); return bad(RSI_ERR_HIP); }
      const size_t usable = free_b - free_b / 8;      // an eighth stays for the contexts that run the chromosomes
      const size_t fit = usable / alloc;
      if (fit < 2) {
        set_global_error(std::string(fn) + ": " + std::to_string(ncols) + " samples of the longest sequence (" + std::to_string(longest) +
                         " bases) need " + std::to_string(alloc) + " bytes of device memory per depth buffer and two buffers at least (" +
                         std::to_string(2 * alloc) + " bytes), but only " + std::to_string(usable) + " of " + std::to_string(free_b) +
                         " free bytes are usable: select fewer samples");
        return bad(RSI_ERR_UNSUPPORTED);
      }
      g->max_resident = (int)std::min<size_t>((size_t)max_resident, fit);
    }
    if (int rc = g->src.open_(path)) { set_global_error(g->src.err); return bad(rc); }
    if (index_path) if (int rc = g->src.open_range(index_path, g->ref_names)) { set_global_error(g->src.err); return bad(rc); }
    if (g->src.format == 1) {
      g->chunk = std::max(g->chunk, kBgzfMinChunk);   // whole members per chunk
      if (hipStreamCreateWithFlags(&g->istream, hipStreamNonBlocking) != hipSuccess ||
          hipEventCreateWithFlags(&g->iev, hipEventDisableTiming) != hipSuccess) { set_global_error("genome text: stream / event creation failed"); return bad(RSI_ERR_HIP); }
    }
    if (hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&g->sync_ev, hipEventDisableTiming) != hipSuccess) { set_global_error("genome text: stream / event creation failed"); return bad(RSI_ERR_HIP); }
    // name changes per chunk: every 64 bytes of text at most before the chunk is cut shorter (start_chunk)
    g->bound_cap = (unsigned)std::max<size_t>(1024, g->chunk / 64);
    g->seg_cap = 2 * g->bound_cap + 2 * kMaxGenomeSegs;
    g->slots_bytes = ((size_t)max_resident * sizeof(GenomeSlotStats) + 255) & ~size_t(255);
    const size_t read_bytes = g->slots_bytes + 16 + (size_t)g->bound_cap * sizeof(NameBound);
    for (int b = 0; b < 2; ++b)
      if (hipHostMalloc(reinterpret_cast<void**>(&g->pin[b]), g->chunk, hipHostMallocDefault) != hipSuccess) { g->pin[b] = nullptr; set_global_error("out of pinned host memory for the text staging"); return bad(RSI_ERR_INTERNAL); }
    // BGZF: a chunk may run one member past `chunk` (the text carried in front of it is shorter than `chunk`)
    const size_t text_cap = g->chunk + (g->src.format == 1 ? kMemberMax : 0);
    if (g->text_dev[0].ensure(text_cap) != hipSuccess || g->text_dev[1].ensure(text_cap) != hipSuccess || g->dread.ensure(read_bytes) != hipSuccess ||
        g->dsegs.ensure((size_t)g->seg_cap * sizeof(GenomeSeg)) != hipSuccess ||
        g->dwg.ensure((size_t)genome_parse_workgroups(GenomeFormat::kText, (long long)text_cap) * 4 * sizeof(long long)) != hipSuccess ||
        g->hread.ensure(read_bytes) != hipSuccess || g->hsegs.ensure((size_t)g->seg_cap * sizeof(GenomeSeg)) != hipSuccess) {
      set_global_error("genome text: out of device or pinned memory for the staging buffers");
      return bad(RSI_ERR_HIP);
    }
    g->src.borrow(g->pin[0], g->pin[1], g->text_dev[0].p, g->text_dev[1].p, g->chunk);
    if (g->bed) {   // the run list: room for every piece a sorted chunk can give (bedgraph_run_cap)
      long long sum_len = 0;
      for (int64_t n : g->ref_len) if (n > 0 && n < (1ll << 31) - 4096) sum_len += n;
      const unsigned long long cap = bedgraph_run_cap((long long)text_cap, sum_len);
      if (cap > 0xffffffffull) { set_global_error(std::string(fn) + ": the run list would exceed 2^32 entries"); return bad(RSI_ERR_UNSUPPORTED); }
      g->run_cap = (unsigned)cap;
      if (g->druns.ensure(256 + (size_t)cap * sizeof(BedRun)) != hipSuccess) {
        set_global_error("genome bedGraph: out of device memory for the run list");
        return bad(RSI_ERR_HIP);
      }
    }
    g->slot_buf.reset(new DevBuf[(size_t)g->max_resident]);
    g->slot_state.assign((size_t)g->max_resident, 0);
    g->slot_n.assign((size_t)g->max_resident, 0);
    return g.release();
  } catch (const std::exception& e) {
    set_global_error(std::string(fn) + ": " + e.what());
    *st = RSI_ERR_INTERNAL;
    return nullptr;
  }
}

}  // namespace

extern "C" {

rsi_genome_text* rsi_genome_text_open(int device, const char* path, int nref, const char* const* names, const int64_t* lengths,
                                      int max_resident, size_t chunk_bytes, int* status) {
  return genome_text_open("rsi_genome_text_open", device, path, nref, names, lengths, nullptr, 0, max_resident, chunk_bytes, status);
}

rsi_genome_text* rsi_genome_text_open_samples(int device, const char* path, int nref, const char* const* names, const int64_t* lengths,
                                              const int32_t* cols, int ncols, int max_resident, size_t chunk_bytes, int* status) {
  if (!cols) {
    set_global_error("rsi_genome_text_open_samples: no columns");
    if (status) *status = RSI_ERR_BAD_ARG;
    return nullptr;
  }
  return genome_text_open("rsi_genome_text_open_samples", device, path, nref, names, lengths, cols, ncols, max_resident, chunk_bytes, status);
}

rsi_genome_text* rsi_genome_bedgraph_open(int device, const char* path, int nref, const char* const* names, const int64_t* lengths,
                                          int max_resident, size_t chunk_bytes, int* status) {
  return genome_text_open("rsi_genome_bedgraph_open", device, path, nref, names, lengths, nullptr, 0, max_resident, chunk_bytes, status, true);
}

rsi_genome_text* rsi_genome_bedgraph_open_indexed(int device, const char* path, const char* index_path, int nref, const char* const* names,
                                                  const int64_t* lengths, int max_resident, size_t chunk_bytes, int* status) {
  if (!index_path || !index_path[0]) {
    set_global_error("rsi_genome_bedgraph_open_indexed: no index");
    if (status) *status = RSI_ERR_BAD_ARG;
    return nullptr;
  }
  return genome_text_open("rsi_genome_bedgraph_open_indexed", device, path, nref, names, lengths, nullptr, 0, max_resident, chunk_bytes, status, true, index_path);
}

int rsi_genome_text_index_range(const rsi_genome_text* g, int64_t* begin, int64_t* stop) {
  if (!g || !g->src.ranged) return RSI_ERR_BAD_ARG;
  if (begin) *begin = g->src.range_begin;
  if (stop) *stop = g->src.range_stop;
  return RSI_OK;
}

int rsi_genome_text_samples(const rsi_genome_text* g) { return g ? g->ncols() : RSI_ERR_BAD_ARG; }

int rsi_genome_text_max_resident(const rsi_genome_text* g) { return g ? g->max_resident : RSI_ERR_BAD_ARG; }

const void* rsi_genome_text_sample_depth(const rsi_genome_text* g, int slot, int j) {
  if (!g || slot < 0 || slot >= g->max_resident || g->slot_state[(size_t)slot] != 2 || j < 0 || j >= g->ncols()) return nullptr;
  return static_cast<const int32_t*>(g->slot_buf[(size_t)slot].p) + (size_t)j * (size_t)g->sample_stride(slot);
}

int64_t rsi_genome_text_copy_sample_depth(rsi_genome_text* g, int slot, int j, int32_t* out, int64_t cap) {
  if (!g || slot < 0 || slot >= g->max_resident || g->slot_state[(size_t)slot] != 2 || j < 0 || j >= g->ncols()) return RSI_ERR_BAD_ARG;
  if (g->failed) return RSI_ERR_BAD_ARG;
  const int64_t n = g->slot_n[(size_t)slot];
  if (!out) return n;
  const int64_t k = std::min(n, cap);
  if (hipSetDevice(g->device) != hipSuccess) return g->fail_(RSI_ERR_HIP, "hipSetDevice failed");
  const int32_t* src = static_cast<const int32_t*>(g->slot_buf[(size_t)slot].p) + (size_t)j * (size_t)g->sample_stride(slot);
  if (int rc = g->hip_(hipMemcpyAsync(out, src, (size_t)k * 4, hipMemcpyDeviceToHost, g->stream), "hipMemcpyAsync")) return rc;
  if (int rc = g->wait()) return rc;
  return k;
}

int rsi_genome_text_next(rsi_genome_text* g, rsi_genome_chrom* out) {
  if (!g || !out) return RSI_ERR_BAD_ARG;
  if (g->failed) return RSI_ERR_BAD_ARG;
  try {
    if (hipSetDevice(g->device) != hipSuccess) return g->fail_(RSI_ERR_HIP, "hipSetDevice failed");
    while (g->ready_head == g->ready.size() && !g->done) {
      g->ready.erase(g->ready.begin(), g->ready.begin() + (ptrdiff_t)g->ready_head);
      g->ready_head = 0;
      if (int rc = g->advance()) return rc;
    }
    if (g->ready_head == g->ready.size()) return 0;
    *out = g->ready[g->ready_head++];
    if (out->slot >= 0) g->slot_state[(size_t)out->slot] = 2;
    return 1;
  } catch (const std::exception& e) {
    return g->fail_(RSI_ERR_INTERNAL, std::string("rsi_genome_text_next: ") + e.what());
  }
}

void rsi_genome_text_release(rsi_genome_text* g, int slot) {
  if (g && slot >= 0 && slot < g->max_resident && g->slot_state[(size_t)slot] == 2) g->slot_state[(size_t)slot] = 0;
}

int64_t rsi_genome_text_copy_depth(rsi_genome_text* g, int slot, int32_t* out, int64_t cap) {
  return rsi_genome_text_copy_sample_depth(g, slot, 0, out, cap);
}

int rsi_genome_text_kernel_ms(const rsi_genome_text* g, double* bound_ms, double* parse_ms) {
  if (!g) return RSI_ERR_BAD_ARG;
  if (bound_ms) *bound_ms = g->ms_bound;
  if (parse_ms) *parse_ms = g->ms_parse;
  return RSI_OK;
}

const char* rsi_genome_text_last_error(const rsi_genome_text* g) { return g ? g->err.c_str() : "null reader"; }

int rsi_genome_text_inflate_stats(const rsi_genome_text* g, rsi_inflate_stats* out) {
  if (!g || !out) return RSI_ERR_BAD_ARG;
  *out = g->src.st;
  return RSI_OK;
}

void rsi_genome_text_close(rsi_genome_text* g) {
  if (!g) return;
  (void)hipSetDevice(g->device);
  delete g;
}

}  // extern "C"
