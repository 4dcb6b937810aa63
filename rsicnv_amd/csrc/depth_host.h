// depth_host.h -- the host side of `rsicnv depth`, plain C++ with no HIP in it, for track.hip, cli.cpp and
// tests/depth_harness.cpp: the rounding rule of every mean and fraction, the window table, how a region is clipped and written,
// the slice plan of the region lines, the BED reader of `-by FILE`, and the writers of PREFIX.mosdepth.summary.txt and
// PREFIX.mosdepth.global.dist.txt.
#pragma once
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <istream>
#include <ostream>
#include <string>
#include <vector>

#include "track_host.h"

namespace rsidepth {

constexpr int kDistBins = 65536;   // depths 0 .. 65535; deeper bases are counted at 65535

// ---- the rounding rule: S / L with two decimals, rounded half up, in integers ----
// a = S / L, r = S mod L, hundredths (200 r + L) / (2 L), a hundred of them carrying into a.  200 S may leave 64 bits, 200 r does
// not (r < L < 2^55).  L <= 0 or S <= 0 gives 0.00.  The kernels' MeanValue is the same expression, with a and the hundredths in
// one word (a mean of int32 depths leaves room for that).
inline std::string fixed2(int64_t S, int64_t L) {
  uint64_t a = 0, h = 0;
  if (L > 0 && S > 0) {
    const uint64_t l = (uint64_t)L, r = (uint64_t)S % l;
    a = (uint64_t)S / l;
    h = (200 * r + l) / (2 * l);
    if (h == 100) { ++a; h = 0; }
  }
  char b[40];
  snprintf(b, sizeof b, "%llu.%02u", (unsigned long long)a, (unsigned)h);
  return b;
}

// ---- windows of W bases on a chromosome of n: [k W, min((k + 1) W, n)), the last one short ----
inline int64_t window_count(int64_t n, int64_t W) { return n <= 0 || W <= 0 ? 0 : (n + W - 1) / W; }
inline void window(int64_t k, int64_t W, int64_t n, int64_t& start, int64_t& end) { start = k * W; end = std::min(n, (k + 1) * W); }

// ---- a region [start, end) on a chromosome of n bases ----
// Clipped to [0, n): what is summed.  false: nothing of it is left (a == b == 0 then).
inline bool clip(int64_t start, int64_t end, int64_t n, int64_t& a, int64_t& b) {
  a = std::max<int64_t>(start, 0); b = std::min(end, n);
  if (b <= a) { a = b = 0; return false; }
  return true;
}
// What its line shows: the clipped coordinates, or -- empty after clipping -- the given ones, whose mean is then 0.00
inline void written(int64_t start, int64_t end, int64_t n, int64_t& s, int64_t& e) {
  int64_t a, b;
  if (clip(start, end, n, a, b)) { s = a; e = b; } else { s = start; e = end; }
}

// ---- the slice plan of the region lines (track.hip): lines per slice, bounded as the depth track's bases are ----
constexpr int kMeanBytes = 23;   // the largest 64-bit quotient, the point and two places
struct Plan { int64_t slice, max_line, text_cap; };
// false: count < 0.  slice_lines > 0 asks for that slice length (tests); the bounds hold all the same.
inline bool plan(int name_len, int64_t count, int64_t slice_lines, Plan& p) {
  if (count < 0) return false;
  p.max_line = (int64_t)name_len + 4 + 2 * 20 + kMeanBytes;   // three tabs, the newline, two coordinates as long as INT64_MIN
  int64_t s = slice_lines > 0 ? std::min(slice_lines, rsitrack::kSliceBases) : rsitrack::kSliceBases;
  s = std::min(s, rsitrack::kTextBytes / p.max_line);
  s = std::max<int64_t>(1, std::min(s, count));
  p.slice = s;
  p.text_cap = s * p.max_line;
  return true;
}

// ---- `-by FILE`: BED lines, kept in the file's order, overlaps and duplicates too ----
// A name matches a chromosome when they are equal or differ by a leading "chr", as -x matches
inline bool same_chrom(const std::string& a, const std::string& b) { return a == b || "chr" + a == b || a == "chr" + b; }
struct BedLine { std::string chrom; int64_t start = 0, end = 0; };
// Fields are separated by tabs or blanks and the first three count; empty lines, '#' lines and "track" / "browser" lines are
// skipped.  Every other line must be well formed: err names it as -x does ("PATH: line N: ...") and the result is false.
inline bool read_bed(std::istream& in, const std::string& path, std::vector<BedLine>& out, std::string& err) {
  auto coord = [](const std::string& t, int64_t* v) {   // a whole token of digits that fits 64 bits
    if (t.empty() || t.size() > 18) return false;
    int64_t x = 0;
    for (char c : t) { if (c < '0' || c > '9') return false; x = 10 * x + (c - '0'); }
    *v = x;
    return true;
  };
  std::string line;
  long long lineno = 0;
  while (std::getline(in, line)) {
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
    const std::string where = path + ": line " + std::to_string(lineno) + ": ";
    BedLine l;
    if (nt < 3) { err = where + "fewer than three fields"; return false; }
    if (!coord(tok[1], &l.start) || !coord(tok[2], &l.end)) { err = where + "start and end must be non-negative integers"; return false; }
    if (l.end < l.start) { err = where + "end < start"; return false; }
    l.chrom = tok[0];
    out.push_back(l);
  }
  return true;
}

// ---- PREFIX.mosdepth.summary.txt and PREFIX.mosdepth.global.dist.txt ----
struct ChromSummary {
  std::string name;
  int64_t length = 0, bases = 0;   // bases: the exact sum of depth
  int32_t min = 0, max = 0;
};
inline std::string summary_line(const ChromSummary& c) {
  return c.name + "\t" + std::to_string(c.length) + "\t" + std::to_string(c.bases) + "\t" + fixed2(c.bases, c.length) + "\t" + std::to_string(c.min) +
         "\t" + std::to_string(c.max) + "\n";
}
// the header, a line per chromosome, then "total": the lengths and bases added, the smallest minimum, the largest maximum
inline void write_summary(std::ostream& out, const std::vector<ChromSummary>& chroms) {
  out << "chrom\tlength\tbases\tmean\tmin\tmax\n";
  ChromSummary t;
  t.name = "total";
  bool first = true;
  for (const ChromSummary& c : chroms) {
    out << summary_line(c);
    if (c.length <= 0) continue;
    t.length += c.length; t.bases += c.bases;
    t.min = first ? c.min : std::min(t.min, c.min);
    t.max = first ? c.max : std::max(t.max, c.max);
    first = false;
  }
  out << summary_line(t);
}
// One line "name \t d \t fraction" for every d from min(max_depth, 65535) down to 0: the share of the n bases with depth at least d
// (dist[d]: bases of depth d, bin 65535 holding the deeper ones too).  Nothing for n <= 0.
inline void write_dist(std::ostream& out, const std::string& name, const int64_t* dist, int64_t n, int32_t max_depth) {
  if (n <= 0) return;
  int64_t at_least = 0;
  for (int d = (int)std::min<int64_t>(std::max<int32_t>(max_depth, 0), kDistBins - 1); d >= 0; --d) {
    at_least += dist[d];
    out << name << "\t" << d << "\t" << fixed2(at_least, n) << "\n";
  }
}

}  // namespace rsidepth
