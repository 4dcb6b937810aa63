// ingest.hip -- the two data formats in front of the path: the depth of one chromosome from a
// text file (load_data_from_text, loaddata.cpp:496-517) or from a BAM (the pileup loop, samfunctions.cpp), built in HBM.
// The file bytes go through pinned double buffers; parsing, per-read work and the difference-array scan are kernels
// (kernels_io.hip); a BAM's BGZF inflation and record walk run on host threads (bam_host.cpp) or, with rsi_hot_set_bam_read's
// device mode, on the device too (kernels_inflate.hip, kernels_bam.hip).  An armed load (rsi_hot_set_bam_pairs) also keeps the
// pair table, from which the RP / Q0 annotation is computed with no second pass over the file (kernels_pairs.hip).  At the end of the file: the reference
// reader (rsi_ref), which brings an indexed FASTA, text or BGZF, into HBM through the same chunk source.
#include "pipeline_internal.h"
#include "inflate_core.h"
#include "bam_pairs_core.h"
#include "bam_pin_core.h"
#include "pin_host.h"
#include "text_rules.h"
#include "track_index_host.h"
#include "ref_host.h"
#include <fstream>
#include <memory>
#include <unordered_set>
#include <zlib.h>

using namespace rsik;
using namespace rsip;
using rsih::Candidate;
using rsih::Region;

namespace {

// The sequential parse loop (the reference's rules in the reference's order), used when the device
// cannot prove that positions are strictly increasing.  named: "RNAME pos depth" lines of one chromosome (the genome
// reader's fallback): the name token and the blanks around it go first, lines without one are skipped.  cols (named cohort
// lines, "RNAME pos d1 ... dK"): the 1-based depth columns to keep; sample j's array is rd[j * stride, ...), and a column is
// what `iss >> pos >> d1 >> ... >> dc` leaves in dc (0 once an extraction has failed).  bed (named bedGraph lines, "RNAME start
// end d"): each line is read as the lines "RNAME p d", p = start + 1 .. end, in order; "track" and "browser"
// lines are skipped.  Every extraction is text_rules.h's, the device kernels' own.
void parse_depth_text_host(const char* p, size_t sz, int64_t size, std::vector<int32_t>& rd, rsi_text_stats* st, bool named = false,
                           const std::vector<int32_t>* cols = nullptr, int64_t stride = 0, bool bed = false) {
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

constexpr size_t kTextChunk = size_t(64) << 20;   // bytes of text per transfer + kernel
constexpr size_t kBgzfMinChunk = size_t(128) << 10; // BGZF input: a chunk holds whole members, at least this much text
constexpr size_t kMemberMax = 65536;               // BGZF: BSIZE and ISIZE

// The BGZF member at compressed offset `at`, with `avail` bytes of the input at p: "" and m filled when it is a whole,
// well-formed member, else the error to report
std::string bgzf_member_error(const uint8_t* p, size_t avail, int64_t at, rsinf::Member& m) {
  const int r = rsinf::bgzf_member(p, avail, m);
  const std::string where = " at compressed offset " + std::to_string((long long)at);
  if (r == 0) return "BGZF: not a BGZF member" + where;
  if (r < 0 || m.bsize > avail) return "BGZF: the member" + where + " runs past the end of the input";
  if (m.isize > kMemberMax) return "BGZF: ISIZE above 65536 in the member" + where;
  return std::string();
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

// The chunk source of both text readers.  It owns the file and turns its text -- plain, gzip or BGZF -- into
// line-aligned chunks in two buffers that the reader lends (pin[b] on the host, dev[b] in HBM) and fills in turn.  fill(b)
// puts the tail of the chunk before (its bytes behind the cut) in front of the new text.  Text and gzip: read() or zlib's
// gzread() into pin[b], cut at the last line end at once.  BGZF: the host walks the member headers, uploads the compressed
// payloads and a member table, and one launch inflates them into dev[b] behind the tail (moved there device to device), so
// the text exists only in HBM; cut(b) takes the last line end from the launch's status word once the caller has waited
// behind it.  A reader may keep less of a chunk (give_back).  foff[b] is chunk b's text offset; host_range() gives the
// sequential fallback any text range once more.
struct DepthSource {
  int fd = -1;
  std::string path, err;
  int64_t file_size = 0;
  int format = 0;                  // 0 text, 1 BGZF, 2 gzip
  gzFile gz = nullptr;
  rsi_inflate_stats st{};
  char* pin[2] = {nullptr, nullptr};   // the reader's buffers (borrow)
  void* dev[2] = {nullptr, nullptr};
  size_t cap = 0;                  // text bytes per chunk
  size_t carry_max = 0;            // a cut leaves fewer bytes than this behind it
  size_t total[2] = {0, 0};        // bytes in buffer b; the chunk is [0, len[b]) of them, the rest its tail
  size_t len[2] = {0, 0};
  int64_t foff[2] = {0, 0};        // text offset of buffer b's first byte
  int last_nl[2] = {-1, -1};       // BGZF: the last line end in buffer b (-1: none, or not read back yet)
  bool exhausted = false;          // no text left in the file
  // BGZF
  std::vector<uint8_t> cbuf;       // compressed bytes read from the file; cbuf[cpos..] not taken yet
  size_t cpos = 0;
  int64_t cbuf_off = 0;            // file offset of cbuf[0]
  bool file_eof = false;
  std::vector<std::pair<int64_t, int64_t>> index;   // (text offset, file offset) of every member: the fallback's entry points
  PinBuf cpin[2], tpin[2], wpin;
  DevBuf cdev[2], tdev[2], wdev;
  std::vector<int64_t> foffs[2];   // file offsets of the members of each launch (messages)
  bool launched[2] = {false, false};
  hipEvent_t ev[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};
  // BGZF read by index (open_range): the members [range_begin, range_stop) of the file alone.  The first one is inflated on the
  // host when the range is opened, for the index checks; its text from the begin's in-member offset on goes in front of the
  // first chunk like a tail.
  bool ranged = false, first_pending = false, file_has_eof = false;
  int64_t range_begin = 0, range_stop = 0;
  size_t range_drop = 0;           // text of the range's last member behind the range's end: foreign lines, the last one cut short
  std::vector<char> first_text;

  ~DepthSource() {
    if (gz) gzclose(gz);
    if (fd >= 0) close(fd);
    for (int b = 0; b < 2; ++b) for (int k = 0; k < 2; ++k) if (ev[b][k]) (void)hipEventDestroy(ev[b][k]);
  }
  int fail_(int code, const std::string& m) { err = m; return code; }
  int bad_data(const std::string& m) { st.input_error = 1; return fail_(RSI_ERR_BAD_ARG, m); }   // the compressed data is broken
  int too_long(size_t n) { return fail_(RSI_ERR_UNSUPPORTED, "a line of the depth file is longer than " + std::to_string(n) + " bytes"); }

  int open_(const std::string& p) {
    path = p;
    fd = open(path.c_str(), O_RDONLY);
    if (fd < 0) return fail_(RSI_ERR_BAD_ARG, "Cannot open file " + path);
    struct stat sb;
    if (fstat(fd, &sb) != 0) return fail_(RSI_ERR_BAD_ARG, "Cannot stat file " + path);
    file_size = (int64_t)sb.st_size;
    uint8_t head[512];
    const ssize_t n = pread(fd, head, sizeof(head), 0);
    format = rsinf::detect_format(head, n > 0 ? (size_t)n : 0);
    st.format = format;
    if (format == 0) { st.compressed_bytes = st.text_bytes = file_size; return RSI_OK; }
    if (format == 2) {
      st.compressed_bytes = file_size;
      const int d = dup(fd);
      gz = d >= 0 ? gzdopen(d, "rb") : nullptr;
      if (!gz) { if (d >= 0) close(d); return fail_(RSI_ERR_INTERNAL, "zlib: cannot read " + path); }
      gzbuffer(gz, 1 << 20);
    }
    return RSI_OK;
  }

  void borrow(char* pin0, char* pin1, void* dev0, void* dev1, size_t chunk) {
    pin[0] = pin0; pin[1] = pin1; dev[0] = dev0; dev[1] = dev1;
    cap = carry_max = chunk;
  }

  // The next chunk into buffer b, the other one holding the chunk before: that chunk's tail, then new text.  len[b] == 0:
  // the end of the file.  BGZF queues its copies and the inflate on s; len[b] is the whole buffer until cut(b).
  int fill(int b, hipStream_t s) {
    const int p = b ^ 1;
    const size_t tail = total[p] - len[p];
    foff[b] = foff[p] + (int64_t)len[p];
    last_nl[b] = -1;
    if (format == 1) {
      size_t lead = tail;
      int lead_nl = last_nl[p] >= (int)len[p] ? last_nl[p] - (int)len[p] : -1;
      if (tail) {
        const hipError_t e = hipMemcpyAsync(dev[b], static_cast<char*>(dev[p]) + len[p], tail, hipMemcpyDeviceToDevice, s);
        if (e != hipSuccess) return fail_(RSI_ERR_HIP, std::string("BGZF: ") + hipGetErrorString(e));
      } else if (first_pending) {   // the range's first member, inflated by open_range: through pin[b], which a BGZF chunk does not use
        first_pending = false;
        lead = first_text.size();
        memcpy(pin[b], first_text.data(), lead);
        for (lead_nl = (int)lead - 1; lead_nl >= 0 && pin[b][lead_nl] != '\n';) --lead_nl;
        const hipError_t e = hipMemcpyAsync(dev[b], pin[b], lead, hipMemcpyHostToDevice, s);
        if (e != hipSuccess) return fail_(RSI_ERR_HIP, std::string("BGZF: ") + hipGetErrorString(e));
      }
      size_t added = 0;
      const int rc = launch(b, lead, lead_nl, s, added);
      total[b] = len[b] = lead + added;
      if (ranged && exhausted && added >= range_drop) { total[b] = len[b] = lead + added - range_drop; range_drop = 0; }   // (the launch that took the last member)
      return rc;
    }
    if (tail) memcpy(pin[b], pin[p] + len[p], tail);
    size_t have = tail;
    while (have < cap && !exhausted) {
      const ssize_t got = read_text(pin[b] + have, cap - have);
      if (got < 0) return format == 2 ? RSI_ERR_BAD_ARG : RSI_ERR_INTERNAL;
      exhausted = got == 0;
      have += (size_t)got;
    }
    total[b] = len[b] = have;
    if (exhausted) return RSI_OK;
    len[b] = line_cut(b, have);
    return len[b] ? RSI_OK : too_long(cap);
  }

  // After the caller's wait behind fill(b): BGZF's chunk is cut behind the last line end the inflate reported.  Text and
  // gzip were cut in fill().
  int cut(int b) {
    if (format != 1) return RSI_OK;
    if (int rc = check(b, &last_nl[b])) return rc;
    if (exhausted) return RSI_OK;
    if (last_nl[b] < 0) return too_long(cap);
    return give_back(b, (size_t)last_nl[b] + 1);
  }

  // the reader keeps [0, k) of chunk b; the rest goes in front of the next chunk
  int give_back(int b, size_t k) {
    len[b] = k;
    return total[b] - k >= carry_max ? too_long(carry_max) : RSI_OK;
  }

  // text and gzip: the end of the last whole line in the first n bytes of pin[b] (0: none)
  size_t line_cut(int b, size_t n) const {
    while (n > 0 && pin[b][n - 1] != '\n') --n;
    return n;
  }

  // chunk b's text to dev[b] on s (BGZF: there already)
  hipError_t upload(int b, hipStream_t s) {
    return format == 1 ? hipSuccess : hipMemcpyAsync(dev[b], pin[b], len[b], hipMemcpyHostToDevice, s);
  }

  // text / gzip: like read(); < 0 on an error (err)
  ssize_t read_text(char* buf, size_t n) {
    if (format == 0) {
      const ssize_t got = read(fd, buf, n);
      if (got < 0) err = "read error on " + path;
      return got;
    }
    const double t = now_ms();
    const int got = gzread(gz, buf, (unsigned)std::min<size_t>(n, size_t(1) << 30));
    st.t_host_inflate_ms += now_ms() - t;
    int e = Z_OK;
    const char* m = got <= 0 ? gzerror(gz, &e) : nullptr;
    if (got < 0 || (got == 0 && e != Z_OK)) {   // a file cut inside a member ends with 0 and Z_BUF_ERROR, not with -1
      bad_data(std::string("gzip: ") + m + " near compressed offset " + std::to_string((long long)gzoffset(gz)) + " of " + path);
      return -1;
    }
    st.text_bytes += got;
    return got;
  }

  // at least `need` untaken compressed bytes in cbuf, unless the file ends first
  bool have_bytes(size_t need) {
    if (cbuf.size() - cpos >= need) return true;
    if (cpos) { cbuf.erase(cbuf.begin(), cbuf.begin() + (ptrdiff_t)cpos); cbuf_off += (int64_t)cpos; cpos = 0; }
    while (cbuf.size() < need && !file_eof) {
      const size_t old = cbuf.size(), want = std::max(need - old, size_t(4) << 20);
      cbuf.resize(old + want);
      const ssize_t got = read(fd, cbuf.data() + old, want);
      cbuf.resize(old + (got > 0 ? (size_t)got : 0));
      if (got < 0) { err = "read error on " + path; return false; }
      if (got == 0) file_eof = true;
    }
    return cbuf.size() - cpos >= need;
  }

  // BGZF: the next members into dev[b] behind its `tail` bytes -- at most cap bytes of text in the buffer in all, one member
  // at least.  tail_nl: offset of the last line end in the tail (-1: none).  Queues the uploads, the inflate launch and its
  // status read-back on s.  added: text bytes added (0 with exhausted: the end).
  void st_range_end() { st.eof_block = file_has_eof; }   // (the file's end-of-file block is not read: it is there or not all the same)
  int launch(int b, size_t tail, int tail_nl, hipStream_t s, size_t& added) {
    added = 0;
    launched[b] = false;
    foffs[b].clear();
    std::vector<InflateBlock> tab;
    const size_t ccap = cap + 4 * kMemberMax;
    if (cpin[b].ensure(ccap) != hipSuccess || cdev[b].ensure(ccap) != hipSuccess || wpin.ensure(32) != hipSuccess || wdev.ensure(32) != hipSuccess)
      return fail_(RSI_ERR_HIP, "BGZF: out of pinned or device memory for the compressed staging");
    uint8_t* cp = cpin[b].as<uint8_t>();
    size_t comp = 0;
    while (!exhausted) {
      if (ranged && cbuf_off + (int64_t)cpos >= range_stop) { exhausted = true; st_range_end(); break; }   // the range's end is the text's
      // the member's fixed header, its extra field (BSIZE), then all of it, as far as the file has them
      have_bytes(18);
      if (cbuf.size() - cpos >= 12) have_bytes(12 + ((size_t)cbuf[cpos + 10] | ((size_t)cbuf[cpos + 11] << 8)));
      rsinf::Member m;
      if (rsinf::bgzf_member(cbuf.data() + cpos, cbuf.size() - cpos, m) > 0) have_bytes(m.bsize);
      if (!err.empty()) return RSI_ERR_INTERNAL;
      if (cbuf.size() == cpos) { exhausted = true; break; }
      const int64_t at = cbuf_off + (int64_t)cpos;
      const std::string bad = bgzf_member_error(cbuf.data() + cpos, cbuf.size() - cpos, at, m);
      if (!bad.empty()) return bad_data(bad);
      if (!tab.empty() && (tail + added + m.isize > cap || comp + m.clen > ccap)) break;
      memcpy(cp + comp, cbuf.data() + cpos + m.hdr, m.clen);
      tab.push_back(InflateBlock{(long long)comp, (long long)(tail + added), m.clen, m.isize, m.crc, 0});
      index.emplace_back(foff[b] + (int64_t)(tail + added), at);
      foffs[b].push_back(at);
      comp += m.clen; added += m.isize; cpos += m.bsize;
      st.compressed_bytes += m.bsize; st.text_bytes += m.isize; ++st.blocks;
      st.eof_block = m.isize == 0;
      if (ranged && cbuf_off + (int64_t)cpos >= range_stop) { exhausted = true; st_range_end(); break; }   // the range's last member: the text ends with this chunk
    }
    if (tab.empty()) return RSI_OK;
    const size_t tb = tab.size() * sizeof(InflateBlock);
    if (tpin[b].ensure(tb) != hipSuccess || tdev[b].ensure(tb) != hipSuccess) return fail_(RSI_ERR_HIP, "BGZF: out of memory for the member table");
    memcpy(tpin[b].p, tab.data(), tb);
    char* w = wdev.as<char>() + 16 * b;
    hipError_t e = hipMemcpyAsync(cdev[b].p, cp, comp, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(tdev[b].p, tpin[b].p, tb, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemsetAsync(w, 0xff, 8, s);
    if (e == hipSuccess) e = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(w + 8), tail_nl, 1, s);
    if (e != hipSuccess) return fail_(RSI_ERR_HIP, std::string("BGZF: ") + hipGetErrorString(e));
    for (int k = 0; k < 2; ++k) if (!ev[b][k]) (void)hipEventCreate(&ev[b][k]);
    if (ev[b][0]) (void)hipEventRecord(ev[b][0], s);
    launch_inflate_bgzf(cdev[b].p, tdev[b].as<InflateBlock>(), (int)tab.size(), dev[b], reinterpret_cast<int*>(w + 8),
                        reinterpret_cast<unsigned long long*>(w), s);
    if (ev[b][1]) (void)hipEventRecord(ev[b][1], s);
    e = hipMemcpyAsync(wpin.as<char>() + 16 * b, w, 16, hipMemcpyDeviceToHost, s);
    if (e != hipSuccess) return fail_(RSI_ERR_HIP, std::string("BGZF: ") + hipGetErrorString(e));
    launched[b] = true;
    return RSI_OK;
  }

  // after a wait behind launch(b): the first bad member's error, else *last_nl (unchanged when nothing was launched)
  int check(int b, int* last_nl) {
    if (!launched[b]) return RSI_OK;
    launched[b] = false;
    float ms = 0;
    if (ev[b][0] && ev[b][1] && hipEventElapsedTime(&ms, ev[b][0], ev[b][1]) == hipSuccess) st.t_inflate_kernel_ms += ms;
    const char* w = wpin.as<char>() + 16 * b;
    unsigned long long status;
    memcpy(&status, w, 8);
    if (status != ~0ull) {
      const size_t k = (size_t)(status >> 8);
      const int64_t at = k < foffs[b].size() ? foffs[b][k] : -1;
      return bad_data("BGZF: the member at compressed offset " + std::to_string(at) + " of " + path + " is bad: " +
                                        rsinf::err_name((int)(status & 0xff)));
    }
    memcpy(last_nl, w + 8, 4);
    return RSI_OK;
  }

  // The member at compressed offset `at`, inflated on the host (zlib) with its CRC32 and ISIZE checked: "" or what is wrong with it
  std::string host_member(int64_t at, rsinf::Member& m, std::vector<char>& text) {
    std::vector<uint8_t> raw(kMemberMax);
    const ssize_t got = at >= 0 && at < file_size ? pread(fd, raw.data(), raw.size(), (off_t)at) : 0;
    const std::string bad = bgzf_member_error(raw.data(), got > 0 ? (size_t)got : 0, at, m);
    if (!bad.empty()) return bad;
    text.assign(m.isize, 0);
    z_stream z;
    memset(&z, 0, sizeof(z));
    if (inflateInit2(&z, -15) != Z_OK) return "zlib: inflateInit2 failed";
    z.next_in = raw.data() + m.hdr; z.avail_in = m.clen;
    Bytef spare = 0;
    z.next_out = m.isize ? reinterpret_cast<Bytef*>(text.data()) : &spare; z.avail_out = m.isize;
    const int zr = inflate(&z, Z_FINISH);
    const bool whole = zr == Z_STREAM_END && z.avail_out == 0 && z.avail_in == 0;
    inflateEnd(&z);
    if (!whole || (uint32_t)crc32(crc32(0L, Z_NULL, 0), reinterpret_cast<const Bytef*>(text.data()), m.isize) != m.crc)
      return "BGZF: the member at compressed offset " + std::to_string((long long)at) + " is bad";
    return std::string();
  }

  // The sequence name that begins text[at ...], as far as the member holds it (whole: a delimiter ends it inside the member)
  static std::string name_at(const std::vector<char>& text, size_t at, bool& whole) {
    size_t k = at;
    while (k < text.size() && text[k] != '\t' && text[k] != ' ' && text[k] != '\n') ++k;
    whole = k < text.size();
    return std::string(text.data() + at, k - at);
  }
  static bool names_it(const std::vector<std::string>& names, const std::string& got, bool whole) {
    for (const std::string& n : names)
      for (const std::string& form : {n, "chr" + n, n.compare(0, 3, "chr") == 0 ? n.substr(3) : n})
        if (whole ? form == got : form.compare(0, got.size(), got) == 0) return true;
    return false;
  }

  // After open_(): the file is read from the smallest chunk begin to the largest chunk end that the index (.tbi or .csi) holds
  // for `names`, and nothing else of it.  An index that does not fit the file -- a begin that is no member header or lies
  // behind a byte other than a line end, a first line of another sequence, a line of the sequences directly behind the end --
  // is RSI_ERR_BAD_ARG naming the index: never quiet wrong depth.  No line for any name: the range is empty.
  int open_range(const std::string& index_path, const std::vector<std::string>& names) {
    if (format != 1) return fail_(RSI_ERR_BAD_ARG, "index " + index_path + ": " + path + " is not BGZF, an index cannot be used with it");
    rsitbx::FileIndex ix;
    std::string why;
    if (!rsitbx::read_index(index_path, ix, why)) return fail_(RSI_ERR_BAD_ARG, why);
    uint64_t beg = rsitbx::kNoOffset, end = 0;
    for (const std::string& n : names) {
      uint64_t b = 0, e = 0;
      if (rsitbx::locate(ix, n, b, e)) { beg = std::min(beg, b); end = std::max(end, e); }
    }
    uint8_t tail28[rsitrack::kBgzfEofBytes];
    file_has_eof = file_size >= (int64_t)sizeof(tail28) && pread(fd, tail28, sizeof(tail28), (off_t)(file_size - (int64_t)sizeof(tail28))) == (ssize_t)sizeof(tail28) &&
                   memcmp(tail28, rsitrack::bgzf_eof(), sizeof(tail28)) == 0;
    ranged = true;
    if (end <= beg) { range_begin = range_stop = 0; return RSI_OK; }   // nothing to read: the reader finds no sequence
    auto misfit = [&](const std::string& what) { return fail_(RSI_ERR_BAD_ARG, "index " + index_path + " does not fit " + path + ": " + what); };
    const int64_t cb = (int64_t)(beg >> 16), ce = (int64_t)(end >> 16);
    const size_t ub = (size_t)(beg & 0xffff), ue = (size_t)(end & 0xffff);
    rsinf::Member mb, me;
    std::vector<char> tb, te;
    std::string bad = host_member(cb, mb, tb);
    if (!bad.empty()) return misfit("its range begins where no sound member does (" + bad + ")");
    if (ub >= tb.size()) return misfit("its range begins behind the text of the member at compressed offset " + std::to_string((long long)cb));
    if (ub > 0 && tb[ub - 1] != '\n') return misfit("its range begins inside a line (compressed offset " + std::to_string((long long)cb) + ", text offset " + std::to_string(ub) + ")");
    bool whole = false;
    const std::string first = name_at(tb, ub, whole);
    if (!names_it(names, first, whole)) return misfit("the first line of its range names " + first);
    range_begin = cb;
    range_stop = ce;
    if (ue > 0) {   // the range ends inside the member at ce: read to that member's end, and look at what follows the range in it
      if (ce == cb) { me = mb; te = tb; }
      else if (!(bad = host_member(ce, me, te)).empty()) return misfit("its range ends where no sound member is (" + bad + ")");
      if (ue > te.size()) return misfit("its range ends behind the text of the member at compressed offset " + std::to_string((long long)ce));
      if (ue < te.size()) {
        const std::string next = name_at(te, ue, whole);
        if (names_it(names, next, whole)) return misfit("a line of " + next + " follows the end of its range");
      }
      range_stop = ce + (int64_t)me.bsize;
      range_drop = te.size() - ue;   // what follows the range in its last member is foreign by construction: not handed on
    }
    if (range_stop <= cb || range_stop > file_size) return misfit("its range ends in front of its begin, or behind the file");
    // the first member is taken: its text from ub on leads the first chunk; the chunks go on with the member behind it
    first_text.assign(tb.begin() + (ptrdiff_t)ub, ce == cb && ue > 0 ? tb.begin() + (ptrdiff_t)ue : tb.end());
    if (ce == cb) range_drop = 0;
    first_pending = true;
    index.emplace_back(-(int64_t)ub, cb);
    st.compressed_bytes += mb.bsize; st.text_bytes += mb.isize; ++st.blocks;
    cbuf_off = cb + (int64_t)mb.bsize;
    if (lseek(fd, (off_t)cbuf_off, SEEK_SET) != (off_t)cbuf_off) return fail_(RSI_ERR_INTERNAL, "cannot seek in " + path);
    return RSI_OK;
  }

  // The fallback parser's text: [start, end) of the whole text once more, on the host.  Text: pread().  BGZF and gzip:
  // inflated from the member that holds `start` (BGZF) or from the start of the file (gzip), through a descriptor of its
  // own (fd's offset belongs to the chunks).  A short read is an error.
  int host_range(int64_t start, int64_t end, std::vector<char>& out) {
    out.assign((size_t)(end - start), 0);
    if (format == 0) {
      for (size_t have = 0; have < out.size();) {
        const ssize_t got = pread(fd, out.data() + have, out.size() - have, (off_t)(start + (int64_t)have));
        if (got <= 0) return fail_(RSI_ERR_INTERNAL, "read error on " + path);
        have += (size_t)got;
      }
      return RSI_OK;
    }
    int64_t coff = 0, skip = start;
    if (format == 1) {
      auto it = std::upper_bound(index.begin(), index.end(), std::make_pair(start, INT64_MAX));
      if (it != index.begin()) { --it; skip = start - it->first; coff = it->second; }
    }
    const double t = now_ms();
    const int hfd = open(path.c_str(), O_RDONLY);
    if (hfd < 0 || lseek(hfd, (off_t)coff, SEEK_SET) != (off_t)coff) { if (hfd >= 0) close(hfd); return bad_data("Cannot open file " + path); }
    gzFile g = gzdopen(hfd, "rb");
    if (!g) { close(hfd); return fail_(RSI_ERR_INTERNAL, "zlib: cannot read " + path); }
    gzbuffer(g, 1 << 20);
    bool ok = skip == 0 || gzseek(g, (z_off_t)skip, SEEK_SET) == (z_off_t)skip;
    for (size_t have = 0; ok && have < out.size();) {
      const int got = gzread(g, out.data() + have, (unsigned)std::min<size_t>(out.size() - have, size_t(1) << 30));
      ok = got > 0;
      if (ok) have += (size_t)got;
    }
    int e = 0;
    const char* m = ok ? nullptr : gzerror(g, &e);
    const std::string msg = ok ? std::string() : std::string("gzip: ") + (e ? m : "unexpected end of the text") + " in " + path;
    gzclose(g);
    st.t_host_inflate_ms += now_ms() - t;
    return ok ? RSI_OK : bad_data(msg);
  }
};

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
  DepthSource src;
  struct StatsOut { rsi_ctx* c; const DepthSource& s; ~StatsOut() { c->last_inflate = s.st; } } stats_out{ctx, src};   // every return
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
  if (ctx->timing) { double tot = 0; for (const KernelTime& k : ctx->ktimes) { float ms = 0; (void)hipEventElapsedTime(&ms, k.a, k.b); tot += ms; } st->t_parse_kernel_ms = tot; }
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
  DevBuf dcomp, dtext, dtab, dword;
  HIPCHK(dword.ensure(16));
  unsigned long long status = 0;
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
    HIPCHK(dtab.ensure(part.size() * sizeof(InflateBlock)));
    HIPCHK(hipMemcpyAsync(dcomp.p, comp + cbase, (size_t)(c1 - cbase), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(dtab.p, part.data(), part.size() * sizeof(InflateBlock), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemsetAsync(dword.p, 0xff, 8, ctx->stream));
    HIPCHK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(dword.as<char>() + 8), -1, 1, ctx->stream));
    HIPCHK(hipEventRecord(ea, ctx->stream));
    launch_inflate_bgzf(dcomp.p, dtab.as<InflateBlock>(), (int)part.size(), dtext.p, reinterpret_cast<int*>(dword.as<char>() + 8),
                        dword.as<unsigned long long>(), ctx->stream);
    HIPCHK(hipEventRecord(eb, ctx->stream));
    HIPCHK(hipMemcpyAsync(&status, dword.p, 8, hipMemcpyDeviceToHost, ctx->stream));
    if (t1 > t0) HIPCHK(hipMemcpyAsync(out + t0, dtext.p, (size_t)(t1 - t0), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(CTX_SYNC());
    float ms = 0;
    if (hipEventElapsedTime(&ms, ea, eb) == hipSuccess) st.t_inflate_kernel_ms += ms;
    if (status != ~0ull) {
      const size_t k = i + (size_t)(status >> 8);
      const int64_t at = k < starts.size() ? starts[k] : -1;
      ctx->last_inflate = st;
      return fail(ctx, RSI_ERR_BAD_ARG, "BGZF: the member at compressed offset " + std::to_string(at) + " is bad: " + rsinf::err_name((int)(status & 0xff)));
    }
    i = j;
  }
  ctx->last_inflate = st;
  if (stats) *stats = st;
  return text;
}

}  // extern "C"

namespace {
// The sequence of a run that loaded its depth itself: the host's bytes go to the context's buffer; a device pointer (the
// _dfasta entry points) is used where it is
int upload_fasta(rsi_ctx* ctx, const uint8_t* fasta, int64_t n) {
  HIPCHK(ctx->in_fasta.ensure((size_t)n + 64));
  HIPCHK(hipMemcpyAsync(ctx->in_fasta.p, fasta, (size_t)n, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return RSI_OK;
}
// ---- the pair table of an armed BAM load and what is computed from it ----
constexpr size_t kPairsFirstCap = size_t(1) << 20;           // entries of the first allocation (20 MB); doubled when it fills up

PairTable pair_table(const rsi_ctx* ctx) {
  int32_t* b = ctx->pairs.tab.as<int32_t>();
  const size_t c = ctx->pairs.cap;
  return PairTable{b, b + c, b + 2 * c, b + 3 * c, reinterpret_cast<uint32_t*>(b + 4 * c)};
}
// Room for `need` entries: a larger table takes over the entries written so far, copied on the stream.
int pairs_reserve(rsi_ctx* ctx, size_t need) {
  rsi_ctx::Pairs& P = ctx->pairs;
  if (need <= P.cap) return RSI_OK;
  const size_t cap = std::max(need, P.cap ? 2 * P.cap : kPairsFirstCap);
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
  for (size_t k = first; k + 1 < last && k + 1 < ctx->pairs.events.size(); k += 2) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, ctx->pairs.events[k], ctx->pairs.events[k + 1]) == hipSuccess) sum += ms;
  }
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
    const size_t cap = std::max(need, Q.cap ? 2 * Q.cap : kPairsFirstCap);
    DevBuf grown;
    HIPCHK(grown.ensure(cap * 8));
    for (int k = 0; k < 2 && Q.n > 0; ++k)
      HIPCHK(hipMemcpyAsync(grown.as<int32_t>() + (size_t)k * cap, Q.tab.as<int32_t>() + (size_t)k * Q.cap, (size_t)Q.n * 4, hipMemcpyDeviceToDevice, ctx->stream));
    if (Q.tab.p) HIPCHK(hipStreamSynchronize(ctx->stream));
    std::swap(Q.tab.p, grown.p); std::swap(Q.tab.cap, grown.cap);
    Q.cap = cap;
  }
  if (pool_need > Q.pool_cap) {
    const size_t cap = std::max(pool_need, Q.pool_cap ? 2 * Q.pool_cap : kPairsFirstCap);
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
  float ms = 0;
  if (hipEventElapsedTime(&ms, Q.ev[0], Q.ev[1]) == hipSuccess) Q.t_table_ms += ms;
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
double pin_elapsed(rsi_ctx* ctx) {
  float ms = 0;
  return hipEventElapsedTime(&ms, ctx->pin.ev[0], ctx->pin.ev[1]) == hipSuccess ? ms : 0.0;
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
  Q.stats.t_sample_ms = pin_elapsed(ctx);
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
  Q.stats.t_sample_ms += pin_elapsed(ctx);
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
  Q.stats.t_windows_ms = pin_elapsed(ctx);
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
// the deflate payloads into a pinned buffer and builds the member table; upload and launch_inflate_bgzf run on a stream of
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
    const size_t tb = tab.size() * sizeof(InflateBlock);
    if (D.tpin[b].ensure(tb) != hipSuccess || D.tdev[b].ensure(tb) != hipSuccess) { perr = "out of memory for the BGZF member table"; return RSI_ERR_HIP; }
    memcpy(D.tpin[b].p, tab.data(), tb);
    char* w = D.wdev.as<char>() + 64 * b;
    hipStream_t s = D.istream;
    hipError_t e = used[b] ? hipStreamWaitEvent(s, D.ev[b][3], 0) : hipSuccess;   // text_dev[b]'s chunk before is piled up
    if (e == hipSuccess) e = hipEventRecord(D.ev[b][0], s);
    if (e == hipSuccess) e = hipMemcpyAsync(D.cdev[b].p, cp, comp, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(D.tdev[b].p, D.tpin[b].p, tb, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemsetAsync(w, 0xff, 16, s);     // the status word; last_nl (unused here) starts at -1
    if (e == hipSuccess) e = hipEventRecord(D.ev[b][1], s);
    if (e != hipSuccess) { perr = std::string("BAM device read: ") + hipGetErrorString(e); return RSI_ERR_HIP; }
    launch_inflate_bgzf(D.cdev[b].p, D.tdev[b].as<InflateBlock>(), (int)tab.size(), ctx->text_dev[b].p, reinterpret_cast<int*>(w + 8),
                        reinterpret_cast<unsigned long long*>(w), s);
    e = hipMemcpyAsync(D.wpin.as<char>() + 64 * b, w, 16, hipMemcpyDeviceToHost, s);
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
      float ms = 0;
      if (hipEventElapsedTime(&ms, D.ev[cur][0], D.ev[cur][1]) == hipSuccess) rs.t_upload_ms += ms;
      if (hipEventElapsedTime(&ms, D.ev[cur][1], D.ev[cur][2]) == hipSuccess) { rs.t_inflate_ms += ms; st->t_inflate_ms += ms; }
      unsigned long long status;
      memcpy(&status, D.wpin.as<char>() + 64 * cur, 8);
      if (status != ~0ull) {
        const size_t k = (size_t)(status >> 8);
        return fail(ctx, RSI_ERR_BAD_ARG, "BGZF: the block at file offset " + std::to_string(k < c.at.size() ? (unsigned long long)c.at[k] : 0ull) + " of " + bam_path +
                                              " is bad: " + rsinf::err_name((int)(status & 0xff)));
      }
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
      BamFindReport* d_rep = reinterpret_cast<BamFindReport*>(w + 16);
      HIPCHK(hipEventRecord(D.find[0], ctx->stream));
      { Timer t(ctx, "bam_guess"); launch_bam_guess(data, (long long)total, (int)reflen.size(), D.reflen.as<int32_t>(), D.guess.as<uint32_t>(), ctx->stream); }
      { Timer t(ctx, "bam_walk"); launch_bam_walk(data, (long long)total, tid, D.guess.as<uint32_t>(), D.segout.as<BamSegOut>(), D.lists.as<uint32_t>(), ctx->stream); }
      { Timer t(ctx, "bam_stitch"); launch_bam_stitch(data, (long long)total, tid, D.guess.as<uint32_t>(), D.segout.as<BamSegOut>(), D.lists.as<uint32_t>(), D.rec.as<uint32_t>(), d_rep, ctx->stream); }
      HIPCHK(hipEventRecord(D.find[1], ctx->stream));
      HIPCHK(hipMemcpyAsync(D.wpin.as<char>() + 64 * cur + 16, d_rep, sizeof(BamFindReport), hipMemcpyDeviceToHost, ctx->stream));
      { const double tq = now_ms(); HIPCHK(CTX_SYNC()); st->t_wait_ms += now_ms() - tq; }
      memcpy(&rep, D.wpin.as<char>() + 64 * cur + 16, sizeof(rep));
      float ms = 0;
      if (hipEventElapsedTime(&ms, D.find[0], D.find[1]) == hipSuccess) { rs.t_find_ms += ms; st->t_walk_ms += ms; }
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

int rsi_hot_run_bam(rsi_ctx* ctx, const rsi_params* p, const char* bam_path, const char* chrom, int minq, int min_baseq,
                    const uint8_t* fasta, int64_t n, rsi_result** out, rsi_bam_stats* stats) {
  return run_bam(ctx, p, bam_path, chrom, minq, min_baseq, fasta, nullptr, n, out, stats);
}
int rsi_hot_run_bam_dfasta(rsi_ctx* ctx, const rsi_params* p, const char* bam_path, const char* chrom, int minq, int min_baseq,
                           const void* d_fasta, int64_t n, rsi_result** out, rsi_bam_stats* stats) {
  return run_bam(ctx, p, bam_path, chrom, minq, min_baseq, nullptr, d_fasta, n, out, stats);
}

}  // extern "C"

// ------------------------------------------------------------------------------------------
// Whole-genome depth text ("RNAME pos depth", every chromosome in one file): a streaming reader that hands over each
// chromosome's depth, resident in HBM, once its last line has been parsed, so that the caller can run it while the next one
// is being parsed.  Per chunk of the file: one transfer, the boundary pass (kernels_io.hip, k_text_name_bounds), ONE small
// read-back (the chunk's name changes and the counts of the chromosomes closed in the chunk before), then parse launches
// over the chunk's segments -- each new name resolved to a depth buffer by the host in between.  Every chromosome's lines
// give what its slice (its lines without the name) gives through rsi_hot_load_depth_text: same rules, same order proof
// (per chromosome), same fallback to the sequential loop (over that chromosome's bytes only).
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
  DepthSource src;                       // the file, its chunks in pin[b] / text_dev[b], their cuts and offsets
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
      float ms = 0;
      if (hipEventElapsedTime(&ms, t.a, t.b) == hipSuccess) (t.parse ? ms_parse : ms_bound) += ms;
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

// ------------------------------------------------------------------------------------------
// The reference read on the device: an indexed FASTA, text or BGZF, one sequence at a time into HBM.  The host
// decisions are ref_host.h's pure functions; the bytes of a sequence's lines reach HBM as the file holds them -- text: pread()
// through two pinned buffers; BGZF: the compressed bytes of the covering members through the depth readers' DepthSource, which
// inflates them there -- and k_ref_unfold (kernels_ref.hip) picks the bases out, span by span.
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
  // BGZF: the chunk source's staging (compressed bytes, member tables, status words), lent to each load's DepthSource and taken
  // back behind it, so that a chromosome costs no pinned or device allocation of its own
  PinBuf cpin[2], tpin[2], wpin;
  DevBuf cdev[2], tdev[2], wdev;
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
template <class B> void swap_buf(B& a, B& b) { std::swap(a.p, b.p); std::swap(a.cap, b.cap); }
// The handle's staging lent to a load's DepthSource; back in the handle when the load ends, however it ends
struct LendStaging {
  rsi_ref* r; DepthSource& s;
  void swap_all() {
    for (int b = 0; b < 2; ++b) { swap_buf(r->cpin[b], s.cpin[b]); swap_buf(r->tpin[b], s.tpin[b]); swap_buf(r->cdev[b], s.cdev[b]); swap_buf(r->tdev[b], s.tdev[b]); }
    swap_buf(r->wpin, s.wpin); swap_buf(r->wdev, s.wdev);
  }
  LendStaging(rsi_ref* ref, DepthSource& src) : r(ref), s(src) { swap_all(); }
  ~LendStaging() { swap_all(); }
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
    float ms = 0;
    if (e == hipSuccess && hipEventElapsedTime(&ms, r->ev[b][0], r->ev[b][1]) == hipSuccess) st->t_kernel_ms += ms;
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
  DepthSource src;
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
  src.ranged = true; src.range_begin = cbegin; src.range_stop = cstop; src.cbuf_off = cbegin;   // the depth readers' indexed seek
  if (lseek(src.fd, (off_t)cbegin, SEEK_SET) != (off_t)cbegin) return ref_fail(r, RSI_ERR_INTERNAL, "cannot seek in " + r->path);
  src.foff[1] = r->table[first].second;   // "the chunk before" of the first fill: empty, ending where the first member's text begins
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
    if (src.launched[cur]) {
      float ms = 0;
      if (hipEventElapsedTime(&ms, src.ev[cur][0], src.ev[cur][1]) == hipSuccess) st->t_kernel_ms += ms;
    }
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
      float ms = 0;
      if (hipEventElapsedTime(&ms, r->ev[0][0], r->ev[0][1]) == hipSuccess) st->t_kernel_ms += ms;
      kdone = k1;
    }
    if (kdone >= s.length) break;
    if (!grew && src.exhausted) break;
    const int64_t keep = std::min<int64_t>(std::max<int64_t>(rsiref::base_pos(s, kdone) - sa, 0), (int64_t)src.total[cur]);
    if (int rc = src.give_back(cur, (size_t)keep)) return ref_fail(r, rc, "reference " + s.name + ": a line terminator longer than the reader carries");
  }
  st->bytes_read += src.st.compressed_bytes; st->text_bytes += src.st.text_bytes; st->members += src.st.blocks;
  // every member of the cover begins in front of the text's end, so a load that got all its bases has read them all: members
  // that do not end where the table's next one begins are not the table's
  const int64_t read_to = src.cbuf_off + (int64_t)src.cpos;
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
