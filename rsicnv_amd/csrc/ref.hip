// ref.hip -- the reference read on the device (rsi_ref): an indexed FASTA, text or BGZF, one sequence at a time
// into HBM.  The host decisions are ref_host.h's pure functions; the bytes of a sequence's lines reach HBM as the file holds
// them -- text: pread() through two pinned buffers; BGZF: the compressed bytes of the covering members through the depth
// readers' chunk source (chunk_source.h), which inflates them there -- and k_ref_unfold (kernels_ref.hip) picks the bases out.
#include "chunk_source.h"
#include "ref_host.h"
#include <fstream>
#include <memory>

using namespace rsik;
using namespace rsip;
using namespace rsing;

struct rsi_ref {
  std::string path, gzi_path, err;   // gzi_path "": the members are walked
  bool gzi_named = false;            // the caller named the .gzi: it must be readable
  std::vector<rsiref::Seq> seqs;
  int format = 0;
  int64_t file_size = 0;
  rsiref::MemberTable table;         // BGZF: built at the first load
  bool table_ready = false, index_used = false;
  int64_t text_size = -1;            // BGZF, members walked: the whole text's length
  std::mutex mu;                     // one load at a time
  int fd = -1;
  // device side, made at the first load
  int device = -1;
  hipStream_t own_stream = nullptr;
  hipEvent_t wait_ev = nullptr, ev[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}}, done[2] = {nullptr, nullptr};
  PinBuf pin[2], hflags;
  DevBuf dev[2], dflags, dseq;
  // BGZF: the chunk source's staging (compressed bytes, member tables, status words), lent to each load's ChunkSource and taken
  // back behind it, so that a chromosome costs no pinned or device allocation of its own
  ChunkSource::Staging stage;
  int64_t chunk_bases = 0;           // text: bases per transfer and launch (0: kRefChunkBases); rsi_ref_debug_set_chunks
  size_t span_bytes = 0;             // BGZF: text per inflate launch (0: kRefSpanBytes)
  ~rsi_ref() {
    if (fd >= 0) close(fd);
    if (device >= 0) (void)hipSetDevice(device);
    for (int b = 0; b < 2; ++b) { for (int k = 0; k < 2; ++k) if (ev[b][k]) (void)hipEventDestroy(ev[b][k]); if (done[b]) (void)hipEventDestroy(done[b]); }
    if (wait_ev) (void)hipEventDestroy(wait_ev);
    if (own_stream) (void)hipStreamDestroy(own_stream);
  }
};

namespace {

constexpr int64_t kRefChunkBases = int64_t(32) << 20;   // text: bases unfolded per transfer (a multiple of 16: whole 16-byte stores)
constexpr size_t kRefSpanBytes = size_t(32) << 20;      // BGZF: text inflated per launch
constexpr size_t kRefMinSpanBytes = 1024;               // ... and the least a test may set: the carried tail (a terminator) must fit half of it
// The handle's staging lent to a load's ChunkSource; back in the handle when the load ends, however it ends
struct LendStaging {
  rsi_ref* r; ChunkSource& s;
  LendStaging(rsi_ref* ref, ChunkSource& src) : r(ref), s(src) { r->stage.swap(s.stage); }
  ~LendStaging() { r->stage.swap(s.stage); }
};
std::string g_ref_open_error;                           // why the last rsi_ref_open failed (guarded by g_err_mu)

int ref_fail(rsi_ref* r, int code, const std::string& m) {
  if (r) r->err = m;
  std::lock_guard<std::mutex> lk(g_err_mu);
  g_ref_open_error = m;
  return code;
}
#define REFHIP(expr)                                                                                          \
  do {                                                                                                        \
    const hipError_t e__ = (expr);                                                                            \
    if (e__ != hipSuccess) return ref_fail(r, RSI_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e__)); \
  } while (0)

// The member table of a BGZF reference: the .gzi's, or -- without one -- the members' BSIZE and ISIZE fields walked on the host
// (two small reads per member, nothing inflated)
int ref_member_table(rsi_ref* r) {
  if (r->table_ready) return RSI_OK;
  if (!r->gzi_path.empty()) {
    FILE* f = fopen(r->gzi_path.c_str(), "rb");
    if (!f) return ref_fail(r, RSI_ERR_BAD_ARG, "cannot open the index " + r->gzi_path);
    std::vector<uint8_t> image;
    uint8_t buf[1 << 16];
    for (size_t got; (got = fread(buf, 1, sizeof(buf), f)) > 0;) image.insert(image.end(), buf, buf + got);
    fclose(f);
    const std::string bad = rsiref::parse_gzi(image.data(), image.size(), r->table);
    if (!bad.empty()) return ref_fail(r, RSI_ERR_BAD_ARG, "index " + r->gzi_path + " does not fit " + r->path + ": it " + bad);
    if (r->table.back().first >= r->file_size) return ref_fail(r, RSI_ERR_BAD_ARG, "index " + r->gzi_path + " does not fit " + r->path + ": an offset lies behind the file's end");
    r->index_used = true;
  } else {
    int64_t text = 0;
    for (int64_t at = 0; at < r->file_size;) {
      uint8_t head[512], foot[4];
      const ssize_t got = pread(r->fd, head, sizeof(head), (off_t)at);
      rsinf::Member m;
      if (got <= 0 || rsinf::bgzf_member(head, (size_t)got, m) != 1 || at + (int64_t)m.bsize > r->file_size ||
          pread(r->fd, foot, 4, (off_t)(at + m.bsize - 4)) != 4)
        return ref_fail(r, RSI_ERR_BAD_ARG, "BGZF: no whole member at compressed offset " + std::to_string((long long)at) + " of " + r->path);
      r->table.emplace_back(at, text);
      text += (int64_t)((uint32_t)foot[0] | ((uint32_t)foot[1] << 8) | ((uint32_t)foot[2] << 16) | ((uint32_t)foot[3] << 24));
      at += m.bsize;
    }
    if (r->table.empty()) return ref_fail(r, RSI_ERR_BAD_ARG, "BGZF: " + r->path + " holds no member");
    r->text_size = text;
  }
  r->table_ready = true;
  return RSI_OK;
}

int ref_device(rsi_ref* r, int device) {
  if (r->device >= 0 && r->device != device)
    return ref_fail(r, RSI_ERR_BAD_ARG, "this rsi_ref loads on device " + std::to_string(r->device) + ": open one handle per device");
  REFHIP(hipSetDevice(device));
  if (r->device < 0) {
    REFHIP(hipStreamCreateWithFlags(&r->own_stream, hipStreamNonBlocking));
    REFHIP(hipEventCreateWithFlags(&r->wait_ev, hipEventDisableTiming));
    for (int b = 0; b < 2; ++b) {
      REFHIP(hipEventCreateWithFlags(&r->done[b], hipEventDisableTiming));
      for (int k = 0; k < 2; ++k) REFHIP(hipEventCreate(&r->ev[b][k]));
    }
    r->device = device;
  }
  REFHIP(r->dflags.ensure(16));
  REFHIP(r->hflags.ensure(16));
  return RSI_OK;
}

// `missing` bytes of the sequence's text lie behind the end of the file (or of the BGZF text): accepted only as the last line's
// terminator of a sequence whose LENGTH is a multiple of LINEBASES
bool short_end_ok(const rsiref::Seq& s, int64_t missing) { return missing > 0 && missing <= s.terminator() && s.length % s.linebases == 0; }

int ref_load_text(rsi_ref* r, const rsiref::Seq& s, const RefLayout& L, uint8_t* d_out, unsigned int* d_flags, hipStream_t stream, rsi_ref_stats* st) {
  bool used[2] = {false, false};
  auto retire = [&](int b) {
    if (!used[b]) return hipSuccess;
    used[b] = false;
    const hipError_t e = event_wait(r->done[b]);
    if (e == hipSuccess) st->t_kernel_ms += elapsed_ms(r->ev[b][0], r->ev[b][1]);
    return e;
  };
  int b = 0;
  const int64_t chunk = r->chunk_bases > 0 ? r->chunk_bases : kRefChunkBases;
  for (int64_t k0 = 0; k0 < s.length; k0 += chunk, b ^= 1) {
    const int64_t k1 = std::min(s.length, k0 + chunk);
    int64_t ta = 0, tb = 0;
    rsiref::text_range(s, k0, k1, ta, tb);
    if (tb > r->file_size) {
      if (k1 != s.length || !short_end_ok(s, tb - r->file_size))
        return ref_fail(r, RSI_ERR_BAD_ARG, "reference " + s.name + ": its lines end at byte " + std::to_string((long long)tb) + ", behind the end of " + r->path + " (" + std::to_string((long long)r->file_size) + " bytes): the .fai does not fit the file");
      tb = r->file_size;
    }
    const size_t len = (size_t)(tb - ta);
    REFHIP(retire(b));
    REFHIP(r->pin[b].ensure(len + 64));
    REFHIP(r->dev[b].ensure(len + 64));
    for (size_t have = 0; have < len;) {
      const ssize_t got = pread(r->fd, r->pin[b].as<char>() + have, len - have, (off_t)(ta + (int64_t)have));
      if (got <= 0) return ref_fail(r, RSI_ERR_INTERNAL, "reference " + s.name + ": short read on " + r->path);
      have += (size_t)got;
    }
    REFHIP(hipMemcpyAsync(r->dev[b].p, r->pin[b].p, len, hipMemcpyHostToDevice, stream));
    REFHIP(hipEventRecord(r->ev[b][0], stream));
    launch_ref_unfold(r->dev[b].p, ta, (long long)len, L, k0, k1, d_out, d_flags, stream);
    REFHIP(hipEventRecord(r->ev[b][1], stream));
    REFHIP(hipEventRecord(r->done[b], stream));
    used[b] = true;
    st->bytes_read += (int64_t)len; st->text_bytes += (int64_t)len;
  }
  for (int k = 0; k < 2; ++k) REFHIP(retire(k));
  return RSI_OK;
}

int ref_load_bgzf(rsi_ref* r, const rsiref::Seq& s, const RefLayout& L, uint8_t* d_out, unsigned int* d_flags, hipStream_t stream, rsi_ref_stats* st) {
  if (int rc = ref_member_table(r)) return rc;
  const std::string index_name = r->index_used ? "index " + r->gzi_path : "the member walk";
  auto misfit = [&](const std::string& what) { return ref_fail(r, RSI_ERR_BAD_ARG, "reference " + s.name + ": " + index_name + " does not fit " + r->path + ": " + what); };
  int64_t ta = 0, tb = 0;
  rsiref::text_range(s, 0, s.length, ta, tb);
  if (r->text_size >= 0 && tb > r->text_size) {
    if (!short_end_ok(s, tb - r->text_size))
      return ref_fail(r, RSI_ERR_BAD_ARG, "reference " + s.name + ": its lines end at byte " + std::to_string((long long)tb) + ", behind the end of the text of " + r->path + " (" + std::to_string((long long)r->text_size) + " bytes): the .fai does not fit the file");
    tb = r->text_size;
  }
  if (tb <= ta) return misfit("no text for the sequence");
  size_t first = 0, stop = 0;
  int64_t skew = 0;
  rsiref::member_cover(r->table, ta, tb, first, stop, skew);
  const int64_t cbegin = r->table[first].first, cstop = stop < r->table.size() ? r->table[stop].first : r->file_size;
  ChunkSource src;
  if (int rc = src.open_(r->path)) return ref_fail(r, rc, src.err);
  if (src.format != 1) return ref_fail(r, RSI_ERR_BAD_ARG, r->path + " is no longer BGZF");
  // text per launch: the whole sequence's when that is little (the source's staging is sized by it), whole members in any case
  const size_t span = r->span_bytes ? r->span_bytes
      : (size_t)std::min<int64_t>((int64_t)kRefSpanBytes, std::max<int64_t>(tb - ta + skew + 2 * (int64_t)kMemberMax, (int64_t)kBgzfMinChunk));
  LendStaging lend(r, src);
  REFHIP(r->dev[0].ensure(span + 4 * kMemberMax));
  REFHIP(r->dev[1].ensure(span + 4 * kMemberMax));
  src.borrow(nullptr, nullptr, r->dev[0].p, r->dev[1].p, span);
  src.carry_max = span / 2;
  if (int rc = src.open_members(cbegin, cstop, r->table[first].second)) return ref_fail(r, rc, src.err);   // the depth readers' indexed seek
  size_t seen = 0;                         // members checked against the table
  int64_t kdone = 0;
  for (int cur = 0; kdone < s.length; cur ^= 1) {
    const size_t tail = src.total[cur ^ 1] - src.len[cur ^ 1];
    if (int rc = src.fill(cur, stream)) {   // a bad member: with a .gzi the index may be what is wrong, without one it is the file
      if (rc == RSI_ERR_BAD_ARG && r->index_used) return misfit(src.err + " (or " + r->path + " itself is damaged)");
      return ref_fail(r, rc, "reference " + s.name + ": " + src.err);
    }
    const bool grew = src.total[cur] > tail;
    REFHIP(stream_wait(stream, r->wait_ev));
    int nl = -1;
    if (int rc = src.check(cur, &nl)) return ref_fail(r, rc, "reference " + s.name + ": " + src.err);
    for (; seen < src.index.size(); ++seen) {   // every member read is the table's next one, at the table's text offset
      if (first + seen >= r->table.size() || src.index[seen].second != r->table[first + seen].first)
        return misfit("the file has a member at compressed offset " + std::to_string((long long)src.index[seen].second) + " that it does not list");
      if (src.index[seen].first != r->table[first + seen].second)
        return misfit("the member at compressed offset " + std::to_string((long long)src.index[seen].second) + " begins at text offset " +
                      std::to_string((long long)src.index[seen].first) + " by the ISIZE of the members before it, not at " + std::to_string((long long)r->table[first + seen].second));
    }
    const int64_t sa = src.foff[cur], sb = sa + (int64_t)src.total[cur];
    int64_t k0 = 0, k1 = 0;
    // the span ends the whole text: the file's last member was read, or (members walked) the text's length is known
    const bool text_end = src.exhausted && (cstop == r->file_size || sb == r->text_size);
    rsiref::contained_bases(s, sa, sb, text_end, k0, k1);
    if (k0 > kdone) return misfit("the text at offset " + std::to_string((long long)sa) + " begins behind base " + std::to_string((long long)kdone));
    if (k1 > kdone) {
      REFHIP(hipEventRecord(r->ev[0][0], stream));
      launch_ref_unfold(src.dev[cur], sa, (long long)src.total[cur], L, kdone, k1, d_out, d_flags, stream);
      REFHIP(hipEventRecord(r->ev[0][1], stream));
      REFHIP(stream_wait(stream, r->wait_ev));
      st->t_kernel_ms += elapsed_ms(r->ev[0][0], r->ev[0][1]);
      kdone = k1;
    }
    if (kdone >= s.length) break;
    if (!grew && src.exhausted) break;
    const int64_t keep = std::min<int64_t>(std::max<int64_t>(rsiref::base_pos(s, kdone) - sa, 0), (int64_t)src.total[cur]);
    if (int rc = src.give_back(cur, (size_t)keep)) return ref_fail(r, rc, "reference " + s.name + ": a line terminator longer than the reader carries");
  }
  st->bytes_read += src.st.compressed_bytes; st->text_bytes += src.st.text_bytes; st->members += src.st.blocks;
  st->t_kernel_ms += src.st.t_inflate_kernel_ms;
  // every member of the cover begins in front of the text's end, so a load that got all its bases has read them all: members
  // that do not end where the table's next one begins are not the table's
  const int64_t read_to = src.read_to();
  if (kdone >= s.length && stop < r->table.size() && read_to != cstop)
    return misfit("the members from compressed offset " + std::to_string((long long)cbegin) + " end at " + std::to_string((long long)read_to) + ", not at " + std::to_string((long long)cstop));
  if (kdone < s.length)
    return ref_fail(r, RSI_ERR_BAD_ARG, "reference " + s.name + ": the text of " + r->path + " ends at base " + std::to_string((long long)kdone) + " of " + std::to_string((long long)s.length) + ": the .fai or " + index_name + " does not fit the file");
  return RSI_OK;
}

}  // namespace

extern "C" {

int rsi_ref_open(const char* fasta_path, const char* fai_path, const char* gzi_path, rsi_ref** out) {
  if (!fasta_path || !out) return ref_fail(nullptr, RSI_ERR_BAD_ARG, "null argument");
  *out = nullptr;
  std::unique_ptr<rsi_ref> r(new rsi_ref);
  r->path = fasta_path;
  r->fd = open(fasta_path, O_RDONLY);
  struct stat sb;
  if (r->fd < 0 || fstat(r->fd, &sb) != 0) return ref_fail(nullptr, RSI_ERR_BAD_ARG, "Cannot open file " + r->path);
  r->file_size = (int64_t)sb.st_size;
  uint8_t head[512];
  const ssize_t got = pread(r->fd, head, sizeof(head), 0);
  r->format = rsinf::detect_format(head, got > 0 ? (size_t)got : 0);
  if (r->format == 2)
    return ref_fail(nullptr, RSI_ERR_UNSUPPORTED, r->path + " is gzip, not BGZF: a compressed reference must be seekable -- recompress it with bgzip (bgzip -i also writes the .gzi) and index it with samtools faidx");
  const std::string fai = fai_path ? fai_path : r->path + ".fai";
  std::ifstream in(fai.c_str());
  if (!in) return ref_fail(nullptr, RSI_ERR_BAD_ARG, "[read_fasta] Index file " + fai + " not found");
  std::string line;
  for (int64_t no = 1; std::getline(in, line); ++no) {
    if (line.find_first_not_of(" \t\r") == std::string::npos) continue;
    rsiref::Seq s;
    const std::string bad = rsiref::parse_fai_line(line, s);
    if (!bad.empty()) return ref_fail(nullptr, RSI_ERR_BAD_ARG, fai + " line " + std::to_string((long long)no) + ": " + bad);
    if (s.name.size() > 255) return ref_fail(nullptr, RSI_ERR_BAD_ARG, fai + " line " + std::to_string((long long)no) + ": a name longer than 255 bytes");
    // a text file's size bounds every sequence now (its last terminator may be missing); a BGZF file's text is measured at the first load
    if (r->format == 0 && s.length > 0 && s.offset + rsiref::flen(s) - (s.length % s.linebases == 0 ? s.terminator() : 0) > r->file_size)
      return ref_fail(nullptr, RSI_ERR_BAD_ARG, fai + " line " + std::to_string((long long)no) + ": " + s.name + " ends behind the end of " + r->path + " (" + std::to_string((long long)r->file_size) + " bytes)");
    r->seqs.push_back(s);
  }
  if (r->format == 1) {
    if (gzi_path && strcmp(gzi_path, "none") != 0) { r->gzi_path = gzi_path; r->gzi_named = true; }
    else if (!gzi_path && access((r->path + ".gzi").c_str(), R_OK) == 0) r->gzi_path = r->path + ".gzi";
    if (r->gzi_named && access(r->gzi_path.c_str(), R_OK) != 0) return ref_fail(nullptr, RSI_ERR_BAD_ARG, "cannot open the index " + r->gzi_path);
  }
  *out = r.release();
  return RSI_OK;
}

void rsi_ref_close(rsi_ref* ref) { delete ref; }

const char* rsi_ref_last_error(const rsi_ref* ref) {
  if (ref) return ref->err.c_str();
  std::lock_guard<std::mutex> lk(g_err_mu);
  static thread_local std::string copy;
  copy = g_ref_open_error;
  return copy.c_str();
}

int rsi_ref_count(const rsi_ref* ref) { return ref ? (int)ref->seqs.size() : RSI_ERR_BAD_ARG; }

int rsi_ref_sequence(const rsi_ref* ref, int i, rsi_ref_seq* out) {
  if (!ref || !out || i < 0 || i >= (int)ref->seqs.size()) return RSI_ERR_BAD_ARG;
  const rsiref::Seq& s = ref->seqs[(size_t)i];
  memset(out, 0, sizeof(*out));
  out->length = s.length; out->offset = s.offset; out->linebases = s.linebases; out->linewidth = s.linewidth;
  memcpy(out->name, s.name.data(), std::min<size_t>(s.name.size(), 255));
  return RSI_OK;
}

int rsi_ref_find(const rsi_ref* ref, const char* rname) { return ref && rname ? rsiref::find(ref->seqs, rname) : -1; }
int rsi_ref_format(const rsi_ref* ref) { return ref ? ref->format : RSI_ERR_BAD_ARG; }
const char* rsi_ref_index_path(const rsi_ref* ref) { return ref ? ref->gzi_path.c_str() : ""; }

}  // extern "C"

namespace {
// rsi_ref_load_device with the handle's lock held by the caller
int ref_load_locked(rsi_ref* r, int device, int i, void* d_out, int64_t cap, void* stream, rsi_ref_stats* st) {
  if (i < 0 || i >= (int)r->seqs.size()) return ref_fail(r, RSI_ERR_BAD_ARG, "no such sequence");
  const rsiref::Seq& s = r->seqs[(size_t)i];
  if (cap < s.length + 64 || (reinterpret_cast<uintptr_t>(d_out) & 15)) return ref_fail(r, RSI_ERR_BAD_ARG, "reference " + s.name + ": the device buffer must be 16-byte aligned and hold LENGTH + 64 bytes");
  const double t0 = now_ms();
  st->format = r->format;
  if (int rc = ref_device(r, device)) return rc;
  drain_stale_errors();
  hipStream_t q = stream ? static_cast<hipStream_t>(stream) : r->own_stream;
  unsigned int* d_flags = r->dflags.as<unsigned int>();
  REFHIP(hipMemsetAsync(d_flags, 0, 16, q));
  int rc = RSI_OK;
  if (s.length > 0) {
    const RefLayout L{(long long)s.offset, (long long)s.length, s.linebases, s.linewidth};
    rc = r->format == 1 ? ref_load_bgzf(r, s, L, static_cast<uint8_t*>(d_out), d_flags, q, st) : ref_load_text(r, s, L, static_cast<uint8_t*>(d_out), d_flags, q, st);
  }
  st->index_used = r->index_used ? 1 : 0;
  if (rc != RSI_OK) { (void)hipStreamSynchronize(q); (void)take_launch_error(); return rc; }   // nothing of this load stays queued
  unsigned int* h_flags = r->hflags.as<unsigned int>();
  REFHIP(hipMemcpyAsync(h_flags, d_flags, 8, hipMemcpyDeviceToHost, q));
  REFHIP(stream_wait(q, r->wait_ev));
  REFHIP(take_launch_error());
  st->t_wall_ms = now_ms() - t0;
  if (h_flags[0] || h_flags[1])
    return ref_fail(r, RSI_ERR_BAD_ARG, "reference " + s.name + ": the .fai does not fit " + r->path + ": " + std::to_string(h_flags[0]) +
                                            " line terminator positions hold something other than a line end, " + std::to_string(h_flags[1]) +
                                            " base positions hold a line end or '>'");
  return RSI_OK;
}
}  // namespace

extern "C" {

int rsi_ref_load_device(rsi_ref* r, int device, int i, void* d_out, int64_t cap, void* stream, rsi_ref_stats* stats) {
  rsi_ref_stats local;
  rsi_ref_stats* st = stats ? stats : &local;
  memset(st, 0, sizeof(*st));
  if (!r || !d_out) return ref_fail(r, RSI_ERR_BAD_ARG, "null argument");
  std::lock_guard<std::mutex> lk(r->mu);
  return ref_load_locked(r, device, i, d_out, cap, stream, st);
}

int rsi_ref_load_host(rsi_ref* r, int device, int i, uint8_t* out, int64_t cap) {
  if (!r || !out) return ref_fail(r, RSI_ERR_BAD_ARG, "null argument");
  if (i < 0 || i >= (int)r->seqs.size()) return ref_fail(r, RSI_ERR_BAD_ARG, "no such sequence");
  const int64_t n = r->seqs[(size_t)i].length;
  if (cap < n) return ref_fail(r, RSI_ERR_BAD_ARG, "rsi_ref_load_host: cap is smaller than the sequence (" + std::to_string((long long)n) + " bases)");
  std::lock_guard<std::mutex> lk(r->mu);   // the handle's own device buffer is part of the load: one lock over both
  REFHIP(hipSetDevice(device));
  REFHIP(r->dseq.ensure((size_t)n + 64));
  rsi_ref_stats st;
  memset(&st, 0, sizeof(st));
  if (int rc = ref_load_locked(r, device, i, r->dseq.p, (int64_t)r->dseq.cap, nullptr, &st)) return rc;
  if (n > 0) REFHIP(hipMemcpy(out, r->dseq.p, (size_t)n, hipMemcpyDeviceToHost));
  return RSI_OK;
}

int rsi_ref_debug_set_chunks(rsi_ref* r, int64_t text_chunk_bases, int64_t bgzf_span_bytes) {
  if (!r || text_chunk_bases < 0 || bgzf_span_bytes < 0 || (bgzf_span_bytes > 0 && bgzf_span_bytes < (int64_t)kRefMinSpanBytes) ||
      text_chunk_bases > kRefChunkBases || bgzf_span_bytes > (int64_t)kRefSpanBytes)
    return ref_fail(r, RSI_ERR_BAD_ARG, "rsi_ref_debug_set_chunks: sizes must be 0 (the default) or within [1, 32 Mi] bases and [1024, 32 Mi] bytes");
  std::lock_guard<std::mutex> lk(r->mu);
  r->chunk_bases = text_chunk_bases; r->span_bytes = (size_t)bgzf_span_bytes;
  return RSI_OK;
}

void* rsi_ref_device_alloc(int device, int64_t bytes) {
  void* p = nullptr;
  if (bytes < 0 || hipSetDevice(device) != hipSuccess || hipMalloc(&p, (size_t)bytes) != hipSuccess) return nullptr;
  return p;
}
void rsi_ref_device_free(int device, void* p) {
  if (p && hipSetDevice(device) == hipSuccess) (void)hipFree(p);
}

int rsi_ref_debug_fai_line(const char* line, rsi_ref_seq* out) {
  if (!line || !out) return ref_fail(nullptr, RSI_ERR_BAD_ARG, "null argument");
  rsiref::Seq s;
  const std::string bad = rsiref::parse_fai_line(line, s);
  if (!bad.empty()) return ref_fail(nullptr, RSI_ERR_BAD_ARG, bad);
  memset(out, 0, sizeof(*out));
  out->length = s.length; out->offset = s.offset; out->linebases = s.linebases; out->linewidth = s.linewidth;
  memcpy(out->name, s.name.data(), std::min<size_t>(s.name.size(), 255));
  return RSI_OK;
}

int rsi_ref_debug_ranges(const rsi_ref_seq* q, int64_t k0, int64_t k1, int64_t a_in, int64_t b_in, int at_eof, int64_t* out) {
  if (!q || !out || q->linebases <= 0 || q->linewidth < q->linebases || k0 < 0 || k1 <= k0 || k1 > q->length) return ref_fail(nullptr, RSI_ERR_BAD_ARG, "bad argument");
  rsiref::Seq s;
  s.length = q->length; s.offset = q->offset; s.linebases = q->linebases; s.linewidth = q->linewidth;
  out[0] = rsiref::flen(s);
  rsiref::text_range(s, k0, k1, out[1], out[2]);
  rsiref::contained_bases(s, a_in, b_in, at_eof != 0, out[3], out[4]);
  return RSI_OK;
}

int64_t rsi_ref_debug_gzi(const uint8_t* image, int64_t len, int64_t* table, int64_t cap) {
  if (!image || len < 0) return ref_fail(nullptr, RSI_ERR_BAD_ARG, "null argument");
  rsiref::MemberTable t;
  const std::string bad = rsiref::parse_gzi(image, (size_t)len, t);
  if (!bad.empty()) return ref_fail(nullptr, RSI_ERR_BAD_ARG, "the .gzi " + bad);
  if (table && (int64_t)t.size() <= cap) for (size_t i = 0; i < t.size(); ++i) { table[2 * i] = t[i].first; table[2 * i + 1] = t[i].second; }
  return (int64_t)t.size();
}

int rsi_ref_debug_cover(const int64_t* table, int64_t n, int64_t a, int64_t b, int64_t* out) {
  if (!table || !out || n <= 0 || a < 0 || b <= a || table[1] > a) return ref_fail(nullptr, RSI_ERR_BAD_ARG, "bad argument");
  rsiref::MemberTable t;
  for (int64_t i = 0; i < n; ++i) t.emplace_back(table[2 * i], table[2 * i + 1]);
  size_t first = 0, stop = 0;
  rsiref::member_cover(t, a, b, first, stop, out[2]);
  out[0] = (int64_t)first; out[1] = (int64_t)stop;
  return RSI_OK;
}

}  // extern "C"
