// chunk_source.h -- the chunk source: a file of text -- plain, gzip or BGZF, whole or the members an index
// names -- as line-aligned chunks in the reader's two buffers, BGZF inflated on the device (bgzf_launch.h).  The depth-text
// readers (ingest.hip, ingest_genome.hip) and the reference reader (ref.hip) take their bytes from it.
#pragma once
#include "pipeline_internal.h"
#include "inflate_core.h"
#include "track_index_host.h"
#include <zlib.h>

namespace rsing __attribute__((visibility("hidden"))) {

using rsip::now_ms;
constexpr size_t kBgzfMinChunk = size_t(128) << 10; // BGZF input: a chunk holds whole members, at least this much text

// The BGZF member at compressed offset `at`, with `avail` bytes of the input at p: "" and m filled when it is a whole,
// well-formed member, else the error to report
inline std::string bgzf_member_error(const uint8_t* p, size_t avail, int64_t at, rsinf::Member& m) {
  const int r = rsinf::bgzf_member(p, avail, m);
  const std::string where = " at compressed offset " + std::to_string((long long)at);
  if (r == 0) return "BGZF: not a BGZF member" + where;
  if (r < 0 || m.bsize > avail) return "BGZF: the member" + where + " runs past the end of the input";
  if (m.isize > kMemberMax) return "BGZF: ISIZE above 65536 in the member" + where;
  return std::string();
}

// The chunk source of both text readers.  It owns the file and turns its text -- plain, gzip or BGZF -- into
// line-aligned chunks in two buffers that the reader lends (pin[b] on the host, dev[b] in HBM) and fills in turn.  fill(b)
// puts the tail of the chunk before (its bytes behind the cut) in front of the new text.  Text and gzip: read() or zlib's
// gzread() into pin[b], cut at the last line end at once.  BGZF: the host walks the member headers, uploads the compressed
// payloads and a member table, and one launch inflates them into dev[b] behind the tail (moved there device to device), so
// the text exists only in HBM; cut(b) takes the last line end from the launch's status word once the caller has waited
// behind it.  A reader may keep less of a chunk (give_back).  foff[b] is chunk b's text offset; host_range() gives the
// sequential fallback any text range once more.
struct ChunkSource {
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
  struct Staging {                 // per buffer: the compressed payloads, pinned and in HBM, and their inflate
    PinBuf cpin[2];
    DevBuf cdev[2];
    BgzfLaunch inflate[2];
    void swap(Staging& o) { for (int b = 0; b < 2; ++b) { swap_buf(cpin[b], o.cpin[b]); swap_buf(cdev[b], o.cdev[b]); inflate[b].swap(o.inflate[b]); } }
  } stage;
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

  ~ChunkSource() {
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
    if (stage.cpin[b].ensure(ccap) != hipSuccess || stage.cdev[b].ensure(ccap) != hipSuccess)
      return fail_(RSI_ERR_HIP, "BGZF: out of pinned or device memory for the compressed staging");
    uint8_t* cp = stage.cpin[b].as<uint8_t>();
    size_t comp = 0;
    while (!exhausted) {
      if (ranged && read_to() >= range_stop) { exhausted = true; st_range_end(); break; }   // the range's end is the text's
      // the member's fixed header, its extra field (BSIZE), then all of it, as far as the file has them
      have_bytes(18);
      if (cbuf.size() - cpos >= 12) have_bytes(12 + ((size_t)cbuf[cpos + 10] | ((size_t)cbuf[cpos + 11] << 8)));
      rsinf::Member m;
      if (rsinf::bgzf_member(cbuf.data() + cpos, cbuf.size() - cpos, m) > 0) have_bytes(m.bsize);
      if (!err.empty()) return RSI_ERR_INTERNAL;
      if (cbuf.size() == cpos) { exhausted = true; break; }
      const int64_t at = read_to();
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
      if (ranged && read_to() >= range_stop) { exhausted = true; st_range_end(); break; }   // the range's last member: the text ends with this chunk
    }
    if (tab.empty()) return RSI_OK;
    BgzfLaunch& inflate = stage.inflate[b];
    if (inflate.reserve(tab.size()) != hipSuccess) return fail_(RSI_ERR_HIP, "BGZF: out of memory for the member table");
    for (int k = 0; k < 2; ++k) if (!ev[b][k]) (void)hipEventCreate(&ev[b][k]);
    const hipError_t e = inflate.queue(tab, cp, comp, stage.cdev[b].p, dev[b], tail_nl, s, ev[b][0], ev[b][1]);
    if (e != hipSuccess) return fail_(RSI_ERR_HIP, std::string("BGZF: ") + hipGetErrorString(e));
    launched[b] = true;
    return RSI_OK;
  }

  // after a wait behind launch(b): the first bad member's error, else *last_nl (unchanged when nothing was launched)
  int check(int b, int* last_nl) {
    if (!launched[b]) return RSI_OK;
    launched[b] = false;
    const BgzfLaunch::Result r = stage.inflate[b].result();
    st.t_inflate_kernel_ms += r.kernel_ms;
    if (!r.ok) {
      const int64_t at = r.member < foffs[b].size() ? foffs[b][r.member] : -1;
      return bad_data("BGZF: the member at compressed offset " + std::to_string(at) + " of " + path + " is bad: " + rsinf::err_name(r.error));
    }
    *last_nl = r.last_nl;
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

  // After open_(), BGZF: the members [cbegin, cstop) of the file are read, and nothing else of it.  text_off: the text offset at
  // which the first chunk begins (foff[b] counts from it).  taken: compressed bytes at cbegin whose text the caller has
  // already (open_range inflates the first member itself); the chunks begin behind them.
  int open_members(int64_t cbegin, int64_t cstop, int64_t text_off, size_t taken = 0) {
    ranged = true; range_begin = cbegin; range_stop = cstop;
    cbuf_off = cbegin + (int64_t)taken;
    foff[1] = text_off;   // "the chunk before" of the first fill: empty, ending where the first chunk's text begins
    if (lseek(fd, (off_t)cbuf_off, SEEK_SET) != (off_t)cbuf_off) return fail_(RSI_ERR_INTERNAL, "cannot seek in " + path);
    return RSI_OK;
  }
  int64_t read_to() const { return cbuf_off + (int64_t)cpos; }   // the file offset behind the last member taken

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
    if (end <= beg) { ranged = true; return RSI_OK; }   // the empty range [0, 0): nothing to read, the reader finds no sequence   // nothing to read: the reader finds no sequence
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
    int64_t stop = ce;
    if (ue > 0) {   // the range ends inside the member at ce: read to that member's end, and look at what follows the range in it
      if (ce == cb) { me = mb; te = tb; }
      else if (!(bad = host_member(ce, me, te)).empty()) return misfit("its range ends where no sound member is (" + bad + ")");
      if (ue > te.size()) return misfit("its range ends behind the text of the member at compressed offset " + std::to_string((long long)ce));
      if (ue < te.size()) {
        const std::string next = name_at(te, ue, whole);
        if (names_it(names, next, whole)) return misfit("a line of " + next + " follows the end of its range");
      }
      stop = ce + (int64_t)me.bsize;
      range_drop = te.size() - ue;   // what follows the range in its last member is foreign by construction: not handed on
    }
    if (stop <= cb || stop > file_size) return misfit("its range ends in front of its begin, or behind the file");
    // the first member is taken: its text from ub on leads the first chunk; the chunks go on with the member behind it
    first_text.assign(tb.begin() + (ptrdiff_t)ub, ce == cb && ue > 0 ? tb.begin() + (ptrdiff_t)ue : tb.end());
    if (ce == cb) range_drop = 0;
    first_pending = true;
    index.emplace_back(-(int64_t)ub, cb);
    st.compressed_bytes += mb.bsize; st.text_bytes += mb.isize; ++st.blocks;
    return open_members(cb, stop, 0, mb.bsize);
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

}  // namespace rsing
