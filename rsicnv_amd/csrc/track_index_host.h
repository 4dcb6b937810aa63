// track_index_host.h -- the tabix index of BGZF tracks, host side: the builder that turns the device's per-slice records (kernels.h:
// chunk starts and window starts, virtual offsets relative to the slice) into per-chromosome chunk lists and linear indexes, and
// the .tbi writer.  Plain C++ with zlib (librsi_hot.so and cli.cpp include it; tests/sanitize_index builds it alone under
// ASan + UBSan).  The format and the rules: DESIGN.md 6i.
#pragma once
#include <errno.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <zlib.h>
#include <algorithm>
#include <map>
#include <string>
#include <vector>
#include "track_host.h"

struct rsi_track_index;   // include/rsi_hot.h's opaque type: defined below

namespace rsitbx {

constexpr int64_t kMaxEnd = int64_t(1) << 29;            // tabix's coordinate limit: five levels above 16 384-base leaves
constexpr uint32_t kWindows = uint32_t(kMaxEnd >> 14);   // 32 768 windows of the linear index
constexpr uint32_t kBins = 37449;                        // bins 0 .. 37448
constexpr uint64_t kNoOffset = ~uint64_t(0);             // a window no line has touched yet

// a record as the device leaves it (rsik::TrackIndexRec): chunk start {voff, a = bin}, window start {voff, a = w_first, b = w_last}
struct Rec { uint64_t voff; uint32_t a, b; };
struct Chunk { uint64_t beg, end; uint32_t bin; };
struct Chrom {
  std::string name;
  std::vector<Chunk> chunks;      // in file order
  std::vector<uint64_t> linear;   // kNoOffset: untouched so far
  int64_t reached = -1;           // the last window a line of this chromosome reaches
};

enum { kOk = 0, kUnsupported = 1, kBadRecords = 2 };

inline uint32_t reg2bin(int64_t s, int64_t e) {   // [s, e) half-open, e > s
  const int64_t e1 = e - 1;
  if (s >> 14 == e1 >> 14) return uint32_t(4681 + (s >> 14));
  if (s >> 17 == e1 >> 17) return uint32_t(585 + (s >> 17));
  if (s >> 20 == e1 >> 20) return uint32_t(73 + (s >> 20));
  if (s >> 23 == e1 >> 23) return uint32_t(9 + (s >> 23));
  if (s >> 26 == e1 >> 26) return uint32_t(1 + (s >> 26));
  return 0;
}

// Records a slice that spans `windows` 16 384-base windows can have (lines sorted and disjoint: a bin changes only at a line
// that touches a window boundary its predecessor did not)
inline uint32_t chunk_capacity(int64_t windows) { return uint32_t(2 * windows + 1); }
inline uint32_t window_capacity(int64_t windows) { return uint32_t(windows + 1); }
inline int64_t windows_spanned(int64_t lo, int64_t hi) { return hi > lo ? ((hi - 1) >> 14) - (lo >> 14) + 1 : 0; }   // of [lo, hi)

// ---- reading an index: where a chromosome's lines lie in the file (.tbi as written below, .csi as bcftools / mosdepth write it) ----
struct RefRange { std::string name; uint64_t beg = kNoOffset, end = 0; bool any = false; };   // smallest chunk begin, largest chunk end
struct FileIndex { bool csi = false; int min_shift = 14, depth = 5; std::vector<RefRange> refs; };

// Both kinds are gzip data: inflated with gzread.  false: err says why (unreadable, neither kind, truncated, counts that cannot be).
inline bool read_index(const std::string& path, FileIndex& out, std::string& err) {
  out = FileIndex();
  auto bad = [&](const std::string& why) { err = "index " + path + ": " + why; return false; };
  gzFile g = gzopen(path.c_str(), "rb");
  if (!g) return bad("cannot open");
  std::string raw;
  std::vector<char> buf(size_t(1) << 20);
  for (;;) {
    const int got = gzread(g, buf.data(), (unsigned)buf.size());
    if (got < 0) { gzclose(g); return bad("not readable as gzip data"); }
    if (got == 0) break;
    raw.append(buf.data(), (size_t)got);
    if (raw.size() > (size_t(1) << 31)) { gzclose(g); return bad("larger than 2 GiB"); }
  }
  int zerr = Z_OK;
  (void)gzerror(g, &zerr);
  gzclose(g);
  if (zerr != Z_OK && zerr != Z_STREAM_END) return bad("not readable as gzip data");
  size_t p = 0;
  bool short_ = false;
  auto take = [&](size_t n) -> const unsigned char* {
    if (short_ || n > raw.size() - p) { short_ = true; return nullptr; }
    p += n;
    return reinterpret_cast<const unsigned char*>(raw.data()) + p - n;
  };
  auto u32 = [&]() -> uint32_t { const unsigned char* b = take(4); return b ? uint32_t(b[0]) | uint32_t(b[1]) << 8 | uint32_t(b[2]) << 16 | uint32_t(b[3]) << 24 : 0; };
  auto u64 = [&]() -> uint64_t { const uint64_t lo = u32(); return lo | uint64_t(u32()) << 32; };
  const unsigned char* magic = take(4);
  if (!magic) return bad("truncated");
  int32_t n_ref = 0;
  std::string names;
  constexpr size_t kWholeFile = ~size_t(0);
  bool bed_like = true;
  auto header = [&](size_t limit) {   // format .. l_nm and the names; limit: the bytes of a .csi's aux block, which they must fit
    const size_t at = p;
    const uint32_t format = u32();   // 0 generic, 1 SAM, 2 VCF; 0x10000: 0-based half-open coordinates, as BED
    if ((format & 0xffffu) != 0) bed_like = false;
    for (int k = 0; k < 5; ++k) (void)u32();
    const uint32_t l_nm = u32();
    if (short_ || l_nm > raw.size() - p || 28 + (size_t)l_nm > limit) { short_ = true; return; }
    names.assign(raw.data() + p, l_nm);
    p = limit == kWholeFile ? p + l_nm : at + limit;   // a .csi's aux block may hold more behind the names
  };
  if (memcmp(magic, "TBI\1", 4) == 0) {
    n_ref = (int32_t)u32();
    header(kWholeFile);
  } else if (memcmp(magic, "CSI\1", 4) == 0) {
    out.csi = true;
    out.min_shift = (int32_t)u32(); out.depth = (int32_t)u32();
    const uint32_t l_aux = u32();
    if (short_ || l_aux > raw.size() - p) return bad("truncated");
    if (out.min_shift < 1 || out.min_shift > 30 || out.depth < 1 || out.depth > 9) return bad("min_shift or depth out of range");
    header(l_aux);
    n_ref = (int32_t)u32();
  } else return bad("neither a .tbi nor a .csi");
  if (short_) return bad("truncated");
  if (!bed_like) return bad("made for a SAM or VCF file, not for a BED-like one");
  if (n_ref < 0 || (size_t)n_ref > names.size()) return bad("more references than names");
  std::vector<std::string> nm;
  for (size_t a = 0; a < names.size();) {
    const size_t z = names.find('\0', a);
    if (z == std::string::npos) return bad("a name is not terminated");
    nm.emplace_back(names, a, z - a);
    a = z + 1;
  }
  if (nm.size() != (size_t)n_ref) return bad("names and references differ in number");
  const uint32_t pseudo = out.csi ? uint32_t(((uint64_t(1) << 3 * (out.depth + 1)) - 1) / 7 + 1) : 37450u;
  for (int32_t r = 0; r < n_ref; ++r) {
    RefRange ref;
    ref.name = nm[(size_t)r];
    const int32_t n_bin = (int32_t)u32();
    if (short_ || n_bin < 0) return bad("truncated");
    for (int32_t b = 0; b < n_bin; ++b) {
      const uint32_t bin = u32();
      if (out.csi) (void)u64();
      const int32_t n_chunk = (int32_t)u32();
      if (short_ || n_chunk < 0 || (size_t)n_chunk > (raw.size() - p) / 16) return bad("truncated");
      for (int32_t c = 0; c < n_chunk; ++c) {
        const uint64_t beg = u64(), end = u64();
        if (bin == pseudo) continue;   // the reference's summary, not lines
        if (end < beg) return bad("a chunk ends in front of its begin");
        ref.beg = std::min(ref.beg, beg); ref.end = std::max(ref.end, end); ref.any = true;
      }
    }
    if (!out.csi) {
      const int32_t n_intv = (int32_t)u32();
      if (short_ || n_intv < 0 || (size_t)n_intv > (raw.size() - p) / 8) return bad("truncated");
      (void)take((size_t)n_intv * 8);
    }
    if (short_) return bad("truncated");
    out.refs.push_back(ref);
  }
  if (raw.size() - p != 0 && raw.size() - p != 8) return bad("bytes behind the last reference");
  return true;
}

// The range of `name`, matched with or without "chr" (as the FASTA's and the BED mask's names are); false: no lines of it
inline bool locate(const FileIndex& ix, const std::string& name, uint64_t& beg, uint64_t& end) {
  for (const RefRange& r : ix.refs)
    if (r.any && (r.name == name || r.name == "chr" + name || "chr" + r.name == name)) { beg = r.beg; end = r.end; return true; }
  return false;
}

}  // namespace rsitbx

struct rsi_track_index {
  std::vector<rsitbx::Chrom> chroms;
  std::string err;

  // One slice of `name`: its packed members are bytes [file_off, file_off + bytes) of the file; the records in any order.  A
  // name equal to the last chromosome's goes on with it (the slices of one call, and a later call that continues it).
  int add_slice(const std::string& name, int64_t file_off, int64_t bytes, const rsitbx::Rec* chunks, size_t nchunk, const rsitbx::Rec* wins,
                size_t nwin) {
    using namespace rsitbx;
    if (nchunk == 0 && nwin == 0) return kOk;   // a slice without a line
    if (nchunk == 0 || file_off < 0 || bytes <= 0 || file_off + bytes >= (int64_t(1) << 47))
      return refuse(kBadRecords, "track index: a slice's records do not fit its lines");
    std::vector<Rec> c(chunks, chunks + nchunk), w(wins, wins + nwin);
    auto by_offset = [](const Rec& x, const Rec& y) { return x.voff < y.voff; };
    std::sort(c.begin(), c.end(), by_offset);
    std::sort(w.begin(), w.end(), by_offset);
    const uint64_t base = uint64_t(file_off) << 16, end = uint64_t(file_off + bytes) << 16;
    for (size_t k = 0; k < nchunk; ++k) {
      if (c[k].a >= kBins || (c[k].voff >> 16) >= uint64_t(bytes) || (k > 0 && c[k].voff == c[k - 1].voff) || (k == 0 && c[k].voff != 0))
        return refuse(kBadRecords, "track index: a chunk record is out of range");
    }
    for (size_t k = 0; k < nwin; ++k) {
      if (w[k].b >= kWindows) return refuse(kUnsupported, "track index: a line ends beyond 2^29 = 536870912, the limit of a tabix index");
      if (w[k].a > w[k].b || (w[k].voff >> 16) >= uint64_t(bytes) || (k > 0 && (w[k].voff == w[k - 1].voff || w[k].b <= w[k - 1].b)))
        return refuse(kBadRecords, "track index: a window record is out of range");
    }
    if (chroms.empty() || chroms.back().name != name) { chroms.emplace_back(); chroms.back().name = name; }
    Chrom& ch = chroms.back();
    for (size_t k = 0; k < nchunk; ++k) {
      const Chunk piece{base + c[k].voff, k + 1 < nchunk ? base + c[k + 1].voff : end, c[k].a};
      if (!ch.chunks.empty() && ch.chunks.back().bin == piece.bin && ch.chunks.back().end == piece.beg) ch.chunks.back().end = piece.end;
      else ch.chunks.push_back(piece);
    }
    for (size_t k = 0; k < nwin; ++k) {
      const int64_t first = std::max<int64_t>(w[k].a, ch.reached + 1), last = w[k].b;   // (a slice's first line may only go on in a window)
      if (first > last) continue;
      ch.linear.resize(size_t(last) + 1, kNoOffset);
      for (int64_t x = first; x <= last; ++x) ch.linear[size_t(x)] = base + w[k].voff;
      ch.reached = last;
    }
    return kOk;
  }

  // src's chromosomes behind this one's, their compressed offsets moved by `shift` bytes; a first chromosome of src that has
  // the name this index ends with goes on with that chromosome
  int append(const rsi_track_index& src, int64_t shift) {
    using namespace rsitbx;
    if (shift < 0 || shift >= (int64_t(1) << 47)) return refuse(kBadRecords, "track index: bad shift");
    const uint64_t d = uint64_t(shift) << 16;
    for (const Chrom& s : src.chroms) {
      Chrom ch = s;
      for (Chunk& k : ch.chunks) { k.beg += d; k.end += d; }
      for (uint64_t& x : ch.linear) if (x != kNoOffset) x += d;
      if (chroms.empty() || chroms.back().name != ch.name) { chroms.push_back(std::move(ch)); continue; }
      // the chromosome this index ends with goes on in src (two parts of one chromosome), as a later slice of it would
      Chrom& last = chroms.back();
      for (const Chunk& k : ch.chunks) {
        if (!last.chunks.empty() && last.chunks.back().bin == k.bin && last.chunks.back().end == k.beg) last.chunks.back().end = k.end;
        else last.chunks.push_back(k);
      }
      if (ch.linear.size() > last.linear.size()) last.linear.resize(ch.linear.size(), kNoOffset);
      for (size_t w = 0; w < ch.linear.size(); ++w)   // a window the part before reached keeps that part's line
        if ((int64_t)w > last.reached && ch.linear[w] != kNoOffset) last.linear[w] = ch.linear[w];
      last.reached = std::max(last.reached, ch.reached);
    }
    return kOk;
  }

  void counts(int64_t& nref, int64_t& nchunks, int64_t& nwindows) const {
    nref = (int64_t)chroms.size(); nchunks = nwindows = 0;
    for (const rsitbx::Chrom& ch : chroms) { nchunks += (int64_t)ch.chunks.size(); nwindows += (int64_t)ch.linear.size(); }
  }

  // The .tbi stream, before compression.  A window no line touched takes the next touched window's offset.
  std::string tbi() const {
    using namespace rsitbx;
    std::string o("TBI\1", 4);
    auto i32 = [&](int32_t v) { const uint32_t u = (uint32_t)v; for (int k = 0; k < 4; ++k) o.push_back(char(u >> (8 * k) & 0xff)); };
    auto u64 = [&](uint64_t v) { for (int k = 0; k < 8; ++k) o.push_back(char(v >> (8 * k) & 0xff)); };
    size_t l_nm = 0;
    for (const Chrom& ch : chroms) l_nm += ch.name.size() + 1;
    i32((int32_t)chroms.size()); i32(0x10000); i32(1); i32(2); i32(3); i32('#'); i32(0); i32((int32_t)l_nm);
    for (const Chrom& ch : chroms) o.append(ch.name.c_str(), ch.name.size() + 1);
    for (const Chrom& ch : chroms) {
      std::map<uint32_t, std::vector<const Chunk*>> bins;
      for (const Chunk& k : ch.chunks) bins[k.bin].push_back(&k);
      i32((int32_t)bins.size());
      for (const auto& b : bins) {
        i32((int32_t)b.first); i32((int32_t)b.second.size());
        for (const Chunk* k : b.second) { u64(k->beg); u64(k->end); }
      }
      std::vector<uint64_t> lin(ch.linear);
      for (size_t x = lin.size(); x-- > 1;) if (lin[x - 1] == kNoOffset) lin[x - 1] = lin[x];   // (the last entry is a touched one)
      i32((int32_t)lin.size());
      for (uint64_t x : lin) u64(x);
    }
    return o;
  }

  // tbi() as BGZF members (zlib) and the end-of-file block into `path`.  false: err says why.
  bool write_tbi(const char* path) {
    const std::string raw = tbi();
    std::string file;
    for (size_t p = 0; p < raw.size(); p += (size_t)rsitrack::kMemberText) {
      const size_t len = std::min(raw.size() - p, (size_t)rsitrack::kMemberText);
      unsigned char body[rsitrack::kMemberSlot];
      z_stream z;
      memset(&z, 0, sizeof(z));
      if (deflateInit2(&z, 6, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) != Z_OK) { err = "track index: zlib failed"; return false; }
      z.next_in = reinterpret_cast<Bytef*>(const_cast<char*>(raw.data() + p)); z.avail_in = (uInt)len;
      z.next_out = body; z.avail_out = (uInt)(sizeof(body) - 26);
      const int zr = deflate(&z, Z_FINISH);
      const size_t clen = sizeof(body) - 26 - z.avail_out;
      deflateEnd(&z);
      if (zr != Z_STREAM_END) { err = "track index: a member did not fit 64 KiB"; return false; }   // (level 6 never expands 65280 bytes by 230)
      const size_t bsize = clen + 26;
      const unsigned char head[18] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, (unsigned char)((bsize - 1) & 0xff), (unsigned char)((bsize - 1) >> 8)};
      file.append(reinterpret_cast<const char*>(head), 18);
      file.append(reinterpret_cast<const char*>(body), clen);
      const uint32_t crc = (uint32_t)crc32(crc32(0L, Z_NULL, 0), reinterpret_cast<const Bytef*>(raw.data() + p), (uInt)len);
      for (int k = 0; k < 4; ++k) file.push_back(char(crc >> (8 * k) & 0xff));
      for (int k = 0; k < 4; ++k) file.push_back(char((uint32_t)len >> (8 * k) & 0xff));
    }
    file.append(rsitrack::bgzf_eof(), rsitrack::kBgzfEofBytes);
    const int fd = ::open(path, O_WRONLY | O_CREAT | O_TRUNC, 0644);
    if (fd < 0) { err = std::string("track index: cannot write ") + path + ": " + strerror(errno); return false; }
    bool ok = rsitrack::write_all(fd, file.data(), file.size());
    const int e = errno;
    if (::close(fd) != 0 && ok) { err = std::string("track index: cannot write ") + path + ": " + strerror(errno); return false; }
    if (!ok) { err = std::string("track index: cannot write ") + path + ": " + strerror(e); (void)::unlink(path); }
    return ok;
  }

 private:
  int refuse(int code, const char* msg) { err = msg; return code; }
};
