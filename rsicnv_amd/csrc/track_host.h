// track_host.h -- the host side of the depth-track and bin-track writers that needs no device: name validation, the slice plans, write()
// until everything is out, and the command line's part files.  Plain C++ (librsi_hot.so and cli.cpp include it; tests/sanitize_track
// builds it alone under ASan + UBSan).
#pragma once
#include <errno.h>
#include <fcntl.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <unistd.h>
#include <algorithm>
#include <string>
#include <vector>

namespace rsitrack {

// Bounds of one slice, whatever the chromosome's length: at most kSliceBases bases, and few enough of them
// that even one line per base, each as long as a line of this call can be, fits kTextBytes.  Per context the writer holds
// kTextBytes + 8 (kSliceBases + 2) + 8 (kSliceBases / 256 + 2) + 32 bytes of HBM (text, run starts, two tile arrays, state) and
// 2 kTextBytes + 64 of pinned host memory -- at most; a short array takes what its one slice needs.  A BGZF track
// adds, for its kMaxMembers = 515 members of kMemberText text bytes a slice: a slot of kMemberSlot bytes and a 4-byte size each,
// and the packed members, at most kTextBytes + 31 kMaxMembers bytes -- 64.3 MiB of HBM more, and 31 kMaxMembers bytes more in
// each pinned buffer.  The plain-text track allocates none of it.
constexpr int64_t kSliceBases = int64_t(512) << 10;
constexpr int64_t kTextBytes = int64_t(32) << 20;
constexpr int kMaxName = 255;
constexpr int64_t kMemberText = 65280;     // text bytes of one BGZF member (bgzip's)
constexpr int64_t kMemberSlot = 65536;     // where the device leaves one: 18 + (kMemberText + 5) + 8 at most
constexpr int64_t kMemberOverhead = 31;    // header, a stored block's 5 bytes, footer
constexpr int64_t kMaxMembers = (kTextBytes + kMemberText - 1) / kMemberText;
static_assert(kMaxMembers == 515, "a slice's members: what k_bgzf_pack scans");
inline int64_t members_of(int64_t text_bytes) { return (text_bytes + kMemberText - 1) / kMemberText; }

// The name's length, or -1: empty, longer than kMaxName, or with a tab or a newline in it (either would break the line)
inline int name_length(const char* name) {
  if (!name) return -1;
  const size_t k = strnlen(name, (size_t)kMaxName + 1);
  if (k == 0 || k > (size_t)kMaxName) return -1;
  for (size_t i = 0; i < k; ++i) if (name[i] == '\t' || name[i] == '\n') return -1;
  return (int)k;
}

inline int dec_len(int64_t x) {   // characters of %lld
  uint64_t u = x < 0 ? uint64_t(0) - (uint64_t)x : (uint64_t)x;
  int d = x < 0 ? 2 : 1;
  while (u >= 10) { u /= 10; ++d; }
  return d;
}

struct Plan {
  int64_t slice;      // bases per slice
  int64_t max_line;   // bytes of the longest line this call can write
  int64_t text_cap;   // bytes a slice's text can take: (slice + 1) * max_line <= kTextBytes
};
// false: pos0 + n leaves int64, or n < 0.  slice_bases > 0 asks for that slice length (tests); the bounds above hold all the same.
inline bool plan(int name_len, int64_t pos0, int64_t n, int64_t slice_bases, Plan& p) {
  if (n < 0 || (pos0 > 0 && n > INT64_MAX - pos0)) return false;
  // coordinates run from pos0 to pos0 + n: the longest is at one of the two ends
  const int coord = std::max(dec_len(pos0), dec_len(pos0 + n));
  p.max_line = (int64_t)name_len + 4 + 2 * coord + 11;   // three tabs, the newline, a value as long as INT32_MIN
  int64_t s = slice_bases > 0 ? std::min(slice_bases, kSliceBases) : kSliceBases;
  s = std::min(s, kTextBytes / p.max_line - 1);           // one line more than bases: the run carried in from the slice before
  s = std::max<int64_t>(1, std::min(s, n));
  p.slice = s;
  p.text_cap = (s + 1) * p.max_line;
  return true;
}

// ---- the per-bin track: slices are ranges of bins ----
constexpr int kMaxBinRegions = 4096;   // removed regions of a chromosome (the pipeline's kMaxRegions)
constexpr int kMedianBytes = 11;       // a value as long as INT32_MIN
constexpr int kRatioBytes = 18;        // the largest q / 1000 with its point and three places
static_assert(kTextBytes / (kMaxName + 4 + 2 * 20 + kRatioBytes) > kMaxBinRegions + 1, "one bin and every region's cut fit the text buffer");
static_assert(kSliceBases > kMaxBinRegions, "one bin and every region's cut fit the pieces");

struct BinPlan {
  int64_t slice;       // bins per slice
  int64_t max_line;    // bytes of the longest line this call can write
  int64_t max_pieces;  // lines a slice can have: slice + nreg (every break cuts at most one bin)
  int64_t text_cap;    // max_pieces * max_line <= kTextBytes
};
// Bins of a chromosome of n bases with nreg removed regions; which: 0 = median, 1 = ratio.  false: n < 0, nb < 0, nreg outside
// [0, kMaxBinRegions] or which outside 0 and 1.  slice_bins > 0 asks for that slice length (tests); the bounds hold all the same:
// max_pieces <= kSliceBases + 1 (the depth track's starts workspace) and text_cap <= kTextBytes, with at least one bin a slice.
inline bool bin_plan(int name_len, int64_t n, int64_t nb, int nreg, int which, int64_t slice_bins, BinPlan& p) {
  if (n < 0 || nb < 0 || nreg < 0 || nreg > kMaxBinRegions || (which != 0 && which != 1)) return false;
  p.max_line = (int64_t)name_len + 4 + 2 * dec_len(n) + (which == 1 ? kRatioBytes : kMedianBytes);   // coordinates run from 0 to n
  int64_t s = slice_bins > 0 ? std::min(slice_bins, kSliceBases) : kSliceBases;
  s = std::min(s, kSliceBases + 1 - nreg);
  s = std::min(s, kTextBytes / p.max_line - nreg);
  s = std::max<int64_t>(1, std::min(s, nb));
  p.slice = s;
  p.max_pieces = s + nreg;
  p.text_cap = p.max_pieces * p.max_line;
  return true;
}

// npairs inclusive [start, end] pairs -> cbreak[k]: compacted index at which region k is cut out; cum[k]: bases removed in front
// of region k (cum[npairs]: in all) -- rsih::compact_table's table.  false: a region outside [0, n), empty, out of order, or
// touching the one before (at least one kept base lies between two regions).
inline bool bin_table(const int32_t* pairs, int npairs, int64_t n, std::vector<int64_t>& cbreak, std::vector<int64_t>& cum, int64_t& ncompact) {
  if (npairs < 0 || n < 0 || (npairs > 0 && !pairs)) return false;
  cbreak.assign((size_t)npairs, 0);
  cum.assign((size_t)npairs + 1, 0);
  for (int k = 0; k < npairs; ++k) {
    const int64_t a = pairs[2 * k], b = pairs[2 * k + 1];
    if (a < 0 || b < a || b >= n) return false;
    if (k > 0 && a <= (int64_t)pairs[2 * k - 1] + 1) return false;
    cbreak[(size_t)k] = a - cum[(size_t)k];
    cum[(size_t)k + 1] = cum[(size_t)k] + (b - a + 1);
  }
  ncompact = n - cum.back();
  return true;
}

// Twice a chromosome's median as an integer (the median of integers is a multiple of 0.5); false: it is not one, or out of range
inline bool twice_median(double median, int64_t& m2) {
  const double d = 2.0 * median;
  if (!(d >= 0.0) || d > 8589934592.0 || d != (double)(int64_t)d) return false;
  m2 = (int64_t)d;
  return true;
}

// Every byte of buf[0, len) to fd, going on after short writes and EINTR.  false: errno says why (a write() of 0 bytes: EIO).
inline bool write_all(int fd, const char* buf, size_t len) {
  while (len > 0) {
    const ssize_t k = ::write(fd, buf, len);
    if (k < 0) { if (errno == EINTR) continue; return false; }
    if (k == 0) { errno = EIO; return false; }
    buf += k; len -= (size_t)k;
  }
  return true;
}

// ---- the command line's part files: chromosomes finish in any order, each into PATH.part.<index>; the parts are appended to
// PATH in the caller's order and deleted.  Nothing but a copy buffer is held in memory. ----
inline std::string part_path(const std::string& path, size_t index) { return path + ".part." + std::to_string(index); }

inline void remove_parts(const std::string& path, size_t count) {
  for (size_t i = 0; i < count; ++i) (void)::unlink(part_path(path, i).c_str());
}

// The BGZF end-of-file block: the empty member that bgzip ends every file with, byte for byte
constexpr size_t kBgzfEofBytes = 28;
inline const char* bgzf_eof() {
  static const unsigned char e[kBgzfEofBytes] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  return reinterpret_cast<const char*>(e);
}
// Appends the end-of-file block to PATH (created if missing).  false: errno says why.
inline bool append_bgzf_eof(const char* path) {
  const int fd = ::open(path, O_WRONLY | O_CREAT | O_APPEND, 0644);
  if (fd < 0) return false;
  const bool ok = write_all(fd, bgzf_eof(), kBgzfEofBytes);
  const int err = errno;
  if (::close(fd) != 0 && ok) return false;
  errno = err;
  return ok;
}

// PATH = the parts `order` names, one after the other (a part that does not exist is a chromosome that wrote none: skipped).
// Every part 0 .. count - 1 is gone afterwards, whatever happened; on a failure PATH is removed too and err says why.
// bgzf: the parts are whole BGZF members (concatenation keeps the file valid) and one end-of-file block follows the last.
// offsets (optional): per entry of `order`, where its part begins in PATH, or -1 for a part that does not exist.
inline bool join_parts(const std::string& path, const std::vector<size_t>& order, size_t count, std::string& err, bool bgzf = false,
                       std::vector<int64_t>* offsets = nullptr) {
  bool ok = true;
  int64_t written = 0;
  if (offsets) offsets->assign(order.size(), -1);
  const int out = ::open(path.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
  if (out < 0) { err = "cannot write " + path + ": " + strerror(errno); ok = false; }
  std::vector<char> buf(size_t(1) << 20);
  for (size_t k = 0; ok && k < order.size(); ++k) {
    const std::string part = part_path(path, order[k]);
    const int in = ::open(part.c_str(), O_RDONLY);
    if (in < 0) {
      if (errno == ENOENT) continue;
      err = "cannot read " + part + ": " + strerror(errno); ok = false;
      break;
    }
    if (offsets) (*offsets)[k] = written;
    for (;;) {
      const ssize_t got = ::read(in, buf.data(), buf.size());
      if (got < 0 && errno == EINTR) continue;
      if (got < 0) { err = "cannot read " + part + ": " + strerror(errno); ok = false; break; }
      if (got == 0) break;
      if (!write_all(out, buf.data(), (size_t)got)) { err = "cannot write " + path + ": " + strerror(errno); ok = false; break; }
      written += (int64_t)got;
    }
    ::close(in);
  }
  if (ok && bgzf && !write_all(out, bgzf_eof(), kBgzfEofBytes)) { err = "cannot write " + path + ": " + strerror(errno); ok = false; }
  if (out >= 0 && ::close(out) != 0 && ok) { err = "cannot write " + path + ": " + strerror(errno); ok = false; }
  remove_parts(path, count);
  if (!ok) (void)::unlink(path.c_str());
  return ok;
}

}  // namespace rsitrack
