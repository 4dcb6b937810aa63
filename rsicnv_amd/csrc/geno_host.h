// geno_host.h -- the host side of `rsicnv geno`, plain C++ with no HIP in it, for pipeline.hip, cli.cpp and
// tests/geno_harness.cpp: a list line's reference interval mapped through the run's removed regions into the compacted array,
// its flanks, the job and tile tables the kernels of kernels_geno.hip read, the ranks of the statistic, the formatted field.
#pragma once
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <string>
#include <vector>

namespace rsigeno {

// ---- the statistic: the reference's _lowerquartile / _median / _upperquartile on ints (partition_stat_tp with dy = 1,
// wufunctions.cpp:364-424) in closed form: of n >= 1 sorted values s[], s[max(n/4,1)-1], s[max(n/2,1)-1], s[max(3n/4,1)-1].
// rank1(n, q): that index plus one, the number of values that must lie at or below the answer (q = 0, 1, 2).
inline int64_t rank1(int64_t n, int q) {
  const int64_t r = q == 0 ? n / 4 : q == 1 ? n / 2 : n * 3 / 4;
  return r < 1 ? 1 : r;
}

// ---- regions ----
// Kept bases in front of reference position x (0-based, 0 <= x <= n): x minus the removed bases below x.  pairs: npairs inclusive
// (start, end) pairs, sorted and disjoint, as rsi_result_noncode reports them.
inline int64_t kept_before(int64_t x, const int32_t* pairs, int npairs) {
  int64_t removed = 0;
  for (int k = 0; k < npairs; ++k) {
    const int64_t s = pairs[2 * k], e = pairs[2 * k + 1];
    if (s >= x) break;
    removed += std::min<int64_t>(e + 1, x) - s;
  }
  return x - removed;
}
struct Span { int64_t a = 0, b = 0; };   // half-open, in the compacted array
// A list line's START / END (1-based, inclusive, in either order) on a chromosome of n bases: clipped to [1, n] and mapped -- the
// inverse of expand_coordinate.  A line wholly outside [1, n], or wholly inside removed regions, gives a == b.
inline Span map_line(int64_t start, int64_t end, int64_t n, const int32_t* pairs, int npairs) {
  if (start > end) std::swap(start, end);
  Span s;
  if (end < 1 || start > n) return s;
  start = std::max<int64_t>(start, 1);
  end = std::min<int64_t>(end, n);
  s.a = kept_before(start - 1, pairs, npairs);
  s.b = kept_before(end, pairs, npairs);
  return s;
}
// One line's ranges: the body and the two pieces of its flank, F = max(N, m) compacted bases on each side.
struct Ranges { Span body, left, right; };
inline Ranges line_ranges(Span body, int64_t m, int64_t ncompact) {
  Ranges r;
  r.body = body;
  const int64_t F = std::max<int64_t>(body.b - body.a, m);
  r.left.a = std::max<int64_t>(0, body.a - F); r.left.b = body.a;
  r.right.a = body.b; r.right.b = std::min(ncompact, body.b + F);
  if (r.right.b < r.right.a) r.right.b = r.right.a;
  return r;
}

// ---- the tables the kernels read ----
// Two jobs per line: 2 i the body, 2 i + 1 the flank (both pieces feed one statistic).  A tile is at most `tile` consecutive
// values of one piece; a job without values has no tile.
struct Tile { int32_t job, off, len, pad; };
constexpr int kDefaultTile = 16384;
inline bool build_tiles(const std::vector<Ranges>& lines, int64_t ncompact, int tile, std::vector<Tile>& tiles) {
  tiles.clear();
  if (tile < 1) return false;
  auto cut = [&](int64_t job, Span s) {
    for (int64_t p = s.a; p < s.b; p += tile) tiles.push_back(Tile{(int32_t)job, (int32_t)p, (int32_t)std::min<int64_t>(tile, s.b - p), 0});
  };
  for (size_t i = 0; i < lines.size(); ++i) {
    const Ranges& r = lines[i];
    for (const Span* s : {&r.body, &r.left, &r.right})
      if (s->a < 0 || s->b < s->a || s->b > ncompact) return false;
    cut(2 * (int64_t)i, r.body);
    cut(2 * (int64_t)i + 1, r.left);
    cut(2 * (int64_t)i + 1, r.right);
  }
  return true;
}

// ---- the field a line gets ----
// CN=%.2f;RATIO=%.3f;MED=%g;FLANK=%g;CHR=%g;N=%d -- RATIO the body's median over the chromosome's, CN = RATIO x ploidy; FLANK=NA
// for an empty flank; CN, RATIO and MED are NA for a line without kept bases (and CN, RATIO for a chromosome median of 0).
inline std::string cn_text(int64_t n_body, double body_med, double chrom_median, double ploidy) {
  if (n_body <= 0 || !(chrom_median > 0)) return "NA";
  char b[64];
  snprintf(b, sizeof b, "%.2f", body_med / chrom_median * ploidy);
  return b;
}
inline std::string format_field(int64_t n_body, int64_t n_flank, double body_med, double flank_med, double chrom_median, double ploidy) {
  char b[64];
  std::string s = "CN=" + cn_text(n_body, body_med, chrom_median, ploidy) + ";RATIO=";
  if (n_body <= 0 || !(chrom_median > 0)) s += "NA";
  else { snprintf(b, sizeof b, "%.3f", body_med / chrom_median); s += b; }
  s += ";MED=";
  if (n_body <= 0) s += "NA";
  else { snprintf(b, sizeof b, "%g", body_med); s += b; }
  s += ";FLANK=";
  if (n_flank <= 0) s += "NA";
  else { snprintf(b, sizeof b, "%g", flank_med); s += b; }
  snprintf(b, sizeof b, ";CHR=%g;N=%lld", chrom_median, (long long)n_body);
  return s + b;
}

}  // namespace rsigeno
