// track_host.h -- the host side of the depth-track writer that needs no device: name validation, the slice plan, write()
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
// 2 kTextBytes + 64 of pinned host memory -- at most; a short array takes what its one slice needs.
constexpr int64_t kSliceBases = int64_t(512) << 10;
constexpr int64_t kTextBytes = int64_t(32) << 20;
constexpr int kMaxName = 255;

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

// PATH = the parts `order` names, one after the other (a part that does not exist is a chromosome that wrote none: skipped).
// Every part 0 .. count - 1 is gone afterwards, whatever happened; on a failure PATH is removed too and err says why.
inline bool join_parts(const std::string& path, const std::vector<size_t>& order, size_t count, std::string& err) {
  bool ok = true;
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
    for (;;) {
      const ssize_t got = ::read(in, buf.data(), buf.size());
      if (got < 0 && errno == EINTR) continue;
      if (got < 0) { err = "cannot read " + part + ": " + strerror(errno); ok = false; break; }
      if (got == 0) break;
      if (!write_all(out, buf.data(), (size_t)got)) { err = "cannot write " + path + ": " + strerror(errno); ok = false; break; }
    }
    ::close(in);
  }
  if (out >= 0 && ::close(out) != 0 && ok) { err = "cannot write " + path + ": " + strerror(errno); ok = false; }
  remove_parts(path, count);
  if (!ok) (void)::unlink(path.c_str());
  return ok;
}

}  // namespace rsitrack
