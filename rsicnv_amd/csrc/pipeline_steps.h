// pipeline_steps.h -- the small host decisions between the pipeline's kernels (pipeline.hip), as pure functions: what the host
// derives from one kernel's result before it launches the next.  Plain C++: no HIP call, no context, no device or pinned
// memory -- so every one of them also runs on the CPU, under ASan + UBSan, against the oracle (tests/sanitize/host_harness.cpp).
// Compiled with -ffp-contract=off like everything that must round as the reference does; the operand types, the order of the
// operations and the casts are the reference's (cited per function) and are part of the result.
#pragma once
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>
#include "host_calls.h"
#include "hostmath.h"
#include "kernels.h"   // record layouts the kernels share with the host: ValueMedian, SegItem, BestSeg, the scan pass record

namespace rsih {

// ---- boundary entries -> pairs ----------------------------------------------------------------------------------------------
// (pos << 1 | is_end) entries, in any order (the device appends them unordered: k_n_transitions, k_resolve_runs), into sorted
// [start, end] pairs.  end_exclusive: the end entries name the first position behind a run.  false = unbalanced starts / ends.
inline bool boundary_pairs(const uint64_t* raw, size_t cnt, bool end_exclusive, std::vector<Region>& out) {
  out.clear();
  std::vector<int64_t> s, e;
  for (size_t i = 0; i < cnt; ++i) { const uint64_t v = raw[i]; ((v & 1) ? e : s).push_back((int64_t)(v >> 1)); }
  if (s.size() != e.size()) return false;
  std::sort(s.begin(), s.end());
  std::sort(e.begin(), e.end());
  for (size_t i = 0; i < s.size(); ++i) out.push_back({(int)s[i], (int)(e[i] - (end_exclusive ? 1 : 0))});
  return true;
}

// ---- order-preserving float key -> float (the encoder: kernels_bin.hip, f32_key) ------------------------------------------------
inline float unkey_f32(uint32_t k) {
  const uint32_t b = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
  float f;
  memcpy(&f, &b, 4);
  return f;
}

// ---- N runs -> padded, merged regions (get_noseq_regions, loaddata.cpp:243-273) -> compaction table -------------------------------
inline std::vector<Region> noncode_regions(const std::vector<Region>& nruns, int64_t n, int dx) {
  std::vector<Region> noncode;
  for (const Region& r : nruns) {
    Region g{std::max(0, r.start - dx), (int)std::min<int64_t>(n - 1, (int64_t)r.end + dx)};
    if (!noncode.empty() && g.start <= noncode.back().end + 1) noncode.back().end = std::max(noncode.back().end, g.end);
    else noncode.push_back(g);
  }
  return noncode;
}
// cbreak[k]: compacted index at which region k is cut out; cum[k]: bases removed in front of region k (cum[nreg]: in all)
struct CompactTable { std::vector<int64_t> cbreak, cum; int64_t ncompact = 0; };
inline CompactTable compact_table(const std::vector<Region>& noncode, int64_t n) {
  CompactTable t;
  t.cbreak.resize(noncode.size());
  t.cum.assign(noncode.size() + 1, 0);
  for (size_t k = 0; k < noncode.size(); ++k) {
    t.cbreak[k] = (int64_t)noncode[k].start - t.cum[k];
    t.cum[k + 1] = t.cum[k] + (noncode[k].end - noncode[k].start + 1);
  }
  t.ncompact = n - t.cum.back();
  return t;
}

// ---- cap from the median of the uncompacted array (loaddata.cpp:229-240, Q15) ---------------------------------------------------
// hist_quantiles_int's result for the median (hostmath.h), from the device's walk; beyond: the median lies above the
// histogram's 65 536 values (loaddata.cpp:233 takes it from the whole rescaled array) and comes from the array itself
struct CapMedian { double med; bool beyond; };
inline CapMedian cap_median(const rsik::ValueMedian& vm, int64_t n) {
  CapMedian c;
  c.med = (double)vm.lo;
  if (vm.lo <= vm.hi && (double)vm.hi - (double)vm.lo >= 1.0 && vm.med >= 0) c.med = (double)vm.med;
  c.beyond = (uint64_t)n / 2 > vm.inrange;
  return c;
}
inline int32_t cap_value(double med, double cap) { return (int32_t)(med * cap); }   // RD[i] = RDmedian*cap, truncated (loaddata.cpp:238)

// ---- chromosome statistics ---------------------------------------------------------------------------------------------------
struct ChromStats { double median = 0, sd = 0; };
// From the residue-class histogram hres[value][kResClasses] (kernels.h) of the compacted depth: chromosome median / SD
// (rsi.cpp:2202-2203).  false: the histogram is empty.
inline bool hist_chrom_stats(const uint32_t* hres, size_t res_vals, int64_t ncompact, ChromStats& out) {
  std::vector<uint64_t> hall(res_vals, 0);
  for (size_t v = 0; v < res_vals; ++v) for (int c = 0; c < rsik::kResClasses; ++c) hall[v] += hres[v * rsik::kResClasses + c];
  Quantiles qall;
  if (!hist_quantiles_int(hall.data(), hall.size(), (uint64_t)ncompact, qall)) return false;
  out.median = qall.med;
  {   // variance(RD,...,-1), wufunctions.cpp:766-809: exact integer sums, one rounding each
    unsigned __int128 s1 = 0, s2 = 0;
    for (size_t v = 0; v < res_vals; ++v) { s1 += (unsigned __int128)v * hall[v]; s2 += (unsigned __int128)v * v * hall[v]; }
    const double d1 = (double)s1, d2 = (double)s2;
    const double mean = d1 / double((int)ncompact);
    out.sd = sqrt(d2 / double((int)ncompact) - mean * mean);
  }
  return true;
}
// MAD of the 31 interleaved subsamples from their value histograms (rsi.cpp:1127-1143).  false: a subsample's histogram is empty.
inline bool hist_subsample_mads(const uint32_t* hres, size_t res_vals, double RDmedian, uint64_t sublen, double mads[31]) {
  for (int j = 0; j < 31; ++j) {
    std::vector<uint64_t> hd(res_vals + 1, 0);
    for (size_t v = 0; v < res_vals; ++v) {
      const uint32_t c = hres[v * rsik::kResClasses + j];
      if (!c) continue;
      const int a = (int)fabs((float)(int)v - RDmedian);    // RDtmp[k]=abs((float)RD[i]-RDmedian), rsi.cpp:1134
      hd[(size_t)a] += c;
    }
    Quantiles qd;
    if (!hist_quantiles_int(hd.data(), hd.size(), sublen, qd)) return false;
    mads[j] = qd.med;
  }
  return true;
}
// value at which the cumulated count first reaches `rank` (partition_stat_tp's walk with dy = 1, wufunctions.cpp:398-420, as
// hist_quantiles_int restates it): the rank-th smallest, the minimum for rank 0 or when all values are equal
inline double rank_value_i32(std::vector<int32_t>& v, uint64_t rank) {
  if (v.empty()) return 0.0;
  const auto mm = std::minmax_element(v.begin(), v.end());
  const int32_t lo = *mm.first, hi = *mm.second;
  if ((double)hi - (double)lo < 1.0 || rank == 0) return (double)lo;
  const size_t k = (size_t)std::min<uint64_t>(rank, v.size()) - 1;
  std::nth_element(v.begin(), v.begin() + k, v.end());
  return (double)v[k];
}
// The same three from the compacted array itself (depths of 65 536 and more are not in the histogram): a selection instead of
// a histogram walk.  mads stays as it is when the array has fewer than 31 values.
inline void array_chrom_stats(const std::vector<int32_t>& rd, ChromStats& out, double mads[31]) {
  const int64_t ncompact = (int64_t)rd.size();
  out.sd = sqrt(variance_pop(rd.data(), (size_t)ncompact));   // the reference's own loop: double sums in index order (wufunctions.cpp:766-809)
  const uint64_t sublen = (uint64_t)(ncompact / 31);
  std::vector<int32_t> sub((size_t)sublen);
  std::vector<int32_t> sorted = rd;
  const double RDmed = rank_value_i32(sorted, (uint64_t)ncompact / 2);
  for (int j = 0; j < 31 && sublen > 0; ++j) {
    for (uint64_t k = 0; k < sublen; ++k) sub[(size_t)k] = (int)fabs((float)rd[(size_t)(j + 31 * k)] - RDmed);   // rsi.cpp:1134
    mads[j] = rank_value_i32(sub, sublen / 2);
  }
  out.median = RDmed;
}

// ---- NB reference levels (negative_binomial_transfer, rsi.cpp:1120-1188; host libm, as the reference) ----------------------------
struct NbLevels { double med_raw, del_raw, dup_raw; };
inline NbLevels nb_reference_levels(double RDmedian, int m, double r) {
  auto nbf = [&](double sum) {
    const double mm = (double)m;
    return 2.0 * sqrt(r) * log(sqrt((sum + 0.25) / (mm * r - 0.5)) + sqrt(1.0 + (sum + 0.25) / (mm * r - 0.5)));
  };
  return NbLevels{nbf(RDmedian * m), nbf(RDmedian / 2.0 * (double)m), nbf(RDmedian * 1.5 * (double)m)};
}
// the scaled reference levels (bins 0 and 2), as k_nb_scale_mm derives them from the raw minimum
struct NbScaled { float t0, t2; };
inline NbScaled nb_scaled_levels(double tmin, double nb_med_raw, double nb_del_raw, double RDmedian) {
  const double med_nbt = nb_med_raw - tmin;
  return NbScaled{(float)((nb_del_raw - tmin) / med_nbt * RDmedian), (float)(med_nbt / med_nbt * RDmedian)};
}

// ---- the keyed form of the NB transform and its quantile chains (kernels.h: launch_nb_keys) ------------------------------------
// A capped depth makes a bin's sum an integer in [0, m * capval]: K = m * capval + 1 possible sums.  The keyed form keeps a counter
// and a table entry per possible sum and its last workgroup reads them all, 128 a thread at the limit of 2^15; the first 2^14 are
// counted in 32 KB of LDS.  -m 101 -cap 4 at 30x gives 12 100 - 12 600 sums and is inside both; 2^15 leaves the same chromosome
// room up to 80x, and beyond it (deep coverage, wide bins) a bin sum spreads over so many values that the array passes are no
// longer the smaller part of the work: the chain of launches stays.
constexpr int64_t kNbKeyLimit = 1 << 15;
inline int64_t nb_key_count(int m, int32_t capval) { return (int64_t)m * (int64_t)capval + 1; }
// nb_route: the NB scan alone (no -MED scan shares the bucket array); capped: a cap exists; long_scan: the scan's long form
inline bool nb_keyed_applies(bool nb_route, bool capped, int64_t K, int64_t nb, bool long_scan) {
  return nb_route && capped && K >= 1 && K <= kNbKeyLimit && nb >= 8 && !long_scan;
}

// ---- scan parameters (rsicnvnbn, rsi.cpp:1262-1360 / rsicnvmed, rsi.cpp:1402-1501) ------------------------------------------------
struct Lamda { double tsigma, tlamda; };
inline Lamda lamda_from_mad(double absmed, double factor, double target) {
  Lamda l;
  l.tsigma = absmed / 0.6745;
  l.tlamda = factor * l.tsigma;
  l.tlamda = std::max(l.tlamda, target);
  return l;
}
// Lmax_ref: the reference's Lmax, as its log prints it; Lmax: what the scan runs with.
// More lengths than bins: the reference's sweeps run L = 1, 2, ... and the PROGRAM exits at L = nb + 1 (runmean refuses a
// span beyond the array, wufunctions.cpp:589-596) -- unless the 20 % rule (rsi.cpp:1226, 1256) has ended the sweep before,
// which on a chromosome with so few bins per length it usually has.  So the scan runs up to nb lengths (clipped), and a sweep
// that gets there without having stopped is what the reference exits on.
struct ScanSetup { double tsigma, tlamda, target, dev; int cal_max, Lmax_ref, Lmax; bool clipped; };
inline ScanSetup scan_first_pass(bool use_med, double tmedian, double absmed, double factor, int LmaxBase, float t0, float t2,
                                 double threshold, int64_t nb) {
  ScanSetup s;
  if (!use_med) {
    s.target = (t2 - t0) * sqrt(2.5);                 // float difference, as RDtrans[2]-RDtrans[0]
    const Lamda l = lamda_from_mad(absmed, factor, s.target);
    s.tsigma = l.tsigma; s.tlamda = l.tlamda;
    const double dnb = fabsf(t2 - t0) + 0.0001;
    const double q = s.tlamda * 2 / dnb;
    s.cal_max = (int)(q * q);
    s.dev = s.tsigma * 3.0;
  } else {
    s.target = tmedian * sqrt(2.0);
    const Lamda l = lamda_from_mad(absmed, factor, s.target);
    s.tsigma = l.tsigma; s.tlamda = l.tlamda;
    if (threshold > 0) s.tlamda = tmedian * threshold;
    const double q = s.tlamda * 4 / (tmedian + 0.001);
    s.cal_max = (int)(q * q);
    s.dev = tmedian * 0.6;
  }
  s.Lmax = LmaxBase;
  if (s.Lmax < s.cal_max) s.Lmax = s.cal_max;
  s.Lmax_ref = s.Lmax;
  s.clipped = s.Lmax > nb;
  if (s.clipped) s.Lmax = (int)nb;
  return s;
}

// ---- what one scan pass leaves in its work block (written by k_level_stop and the scan kernels; layout: kernels.h) ---------------
struct ScanRecord {
  const uint32_t* w;
  int Lmax;
  uint32_t escapes() const { return w[rsik::kScanRecEscapes]; }
  uint32_t inexact() const { return w[rsik::kScanRecInexact]; }
  uint32_t stop_level(int sweep) const { return w[rsik::kScanRecStop + sweep]; }   // 0: DEL, 1: DUP
  uint32_t tiles_listed() const { return w[rsik::kScanRecTiles]; }
  // per-L counts of the bins a sweep newly marked, Lmax + 1 of them
  const uint32_t* level_counts(int sweep) const { return w + rsik::kScanRecLevels + (size_t)sweep * rsik::scan_level_stride(Lmax); }
  // both sweeps of the pass ended by the 20 % rule (rsi.cpp:1226, 1256)
  bool sweeps_stopped(int64_t nb) const {
    for (int k = 0; k < 2; ++k) {
      const uint32_t* cnt = level_counts(k);
      uint64_t cum = 0;
      for (uint32_t L = 0; L <= stop_level(k) && L <= (uint32_t)Lmax; ++L) cum += cnt[L];
      if (!((double)(int)cum / (double)(int)nb > 0.2)) return false;
    }
    return true;
  }
};

// ---- filterstatus (rsi.cpp:948-1047) ---------------------------------------------------------------------------------------------
// The per-level sums: float accumulations in index order (App. A Q13), status values in [-Lmax, Lmax] -> entry status + Lmax.
inline void level_sums_host(const float* tv, const int* st, int64_t nb, int Lmax, std::vector<float>& wsum, std::vector<int>& wcnt) {
  std::fill(wsum.begin(), wsum.end(), 0.0f);
  std::fill(wcnt.begin(), wcnt.end(), 0);
  float s0 = 0.0f;
  int n0 = 0;
  for (int64_t i = 0; i < nb; ++i) {
    const int sv = st[i];
    if (sv == 0) { s0 += tv[i]; ++n0; }
    else { wsum[(size_t)(sv + Lmax)] += tv[i]; ++wcnt[(size_t)(sv + Lmax)]; }
  }
  wsum[(size_t)Lmax] = s0; wcnt[(size_t)Lmax] = n0;
}
// The level range the reference works on is [min status, max status]: taken from the counts.  has_level0 false (no unmarked
// bin in that range: the reference would throw): nothing else is set.  lines: the table the reference writes to its log --
// level, bins, mean; then the two chosen levels (rsi.cpp:991-997).  trim: the levels are in order and the runs' edges are trimmed
// against m0 -+ dev.
struct LevelChoice {
  bool has_level0 = false, trim = false;
  int lo = 0, hi = 0, leveldel = 0, leveladd = 0;
  float m0 = 0.0f;
  std::vector<std::string> lines;
};
inline LevelChoice choose_levels(const std::vector<float>& wsum, const std::vector<int>& wcnt, int Lmax, double dev) {
  LevelChoice c;
  int lo = 0, hi = 0;
  { int a = 0, b = 2 * Lmax; while (a < b && wcnt[a] == 0) ++a; while (b > a && wcnt[b] == 0) --b; lo = a - Lmax; hi = b - Lmax; }
  const int nl = hi - lo + 1;
  std::vector<float> lsum(wsum.begin() + (lo + Lmax), wsum.begin() + (hi + Lmax + 1));
  std::vector<int> lcnt(wcnt.begin() + (lo + Lmax), wcnt.begin() + (hi + Lmax + 1));
  for (int l = 0; l < nl; ++l) if (lcnt[l] != 0) lsum[l] /= (double)lcnt[l];
  c.lo = lo; c.hi = hi;
  if (!(lo <= 0 && -lo < nl)) return c;
  c.has_level0 = true;
  const float m0 = lsum[-lo];
  int leveldel = lo, leveladd = hi;
  for (int l = 0; l < nl; ++l) if (lsum[l] < m0 - dev) { leveldel = l + lo; break; }
  for (int l = nl - 1; l >= 0; --l) if (lsum[l] > m0 + dev) { leveladd = l + lo; break; }
  char line[128];
  for (int l = 0; l < nl; ++l) if (lcnt[l] != 0) { snprintf(line, sizeof(line), "%d\t%d\t%g", l + lo, lcnt[l], (double)lsum[l]); c.lines.push_back(line); }
  snprintf(line, sizeof(line), "%d\t%g", leveldel, (double)lsum[leveldel - lo]); c.lines.push_back(line);
  snprintf(line, sizeof(line), "%d\t%g", leveladd, (double)lsum[leveladd - lo]); c.lines.push_back(line);
  c.trim = !(leveldel > 0 || leveladd < 0 || leveldel > leveladd);
  if (!c.trim) c.lines.push_back("warning level error, status not filtered");
  c.m0 = m0; c.leveldel = leveldel; c.leveladd = leveladd;
  return c;
}

// ---- get_rsi_segments (rsi.cpp:1060-1117) around the device's best-subsegment kernel -------------------------------------------
// The work items: each run's lengths in chunks with about pairs_per_item (L, offset) pairs; poff[r]: where run r's prefix
// (len + 1 entries) starts in the scratch.
// pairs_per_item as a run chooses it.  About 256 pairs per thread of a workgroup (65 536 an item) where a dozen chromosomes share
// the chip; a chromosome that has it to itself (lonely) waits for exactly this kernel and spreads its pairs over as many items as
// still ride in the kernel arguments (kItemsInline; every run's last item is a partial one), down to 32 pairs per thread.
inline int64_t segment_pairs_per_item(const std::vector<Region>& runs, bool lonely) {
  int64_t pairs_per_item = 1 << 16;
  if (lonely) {
    int64_t total = 0;
    for (const Region& r : runs) { const int64_t len = r.end - r.start + 1; total += len * (len + 1) / 2; }
    const int64_t room = std::max<int64_t>(8, (int64_t)rsik::kItemsInline - 2 * (int64_t)runs.size());
    pairs_per_item = std::min<int64_t>(pairs_per_item, std::max<int64_t>(1 << 13, total / room + 1));
  }
  return pairs_per_item;
}
inline void segment_items(const std::vector<Region>& runs, int64_t pairs_per_item, std::vector<int64_t>& poff, std::vector<rsik::SegItem>& items) {
  poff.assign(runs.size() + 1, 0);
  items.clear();
  for (size_t r = 0; r < runs.size(); ++r) {
    const int len = runs[r].end - runs[r].start + 1;
    poff[r + 1] = poff[r] + len + 1;
    int L = 1;
    while (L <= len) {
      int64_t pairs = 0; int Le = L;
      while (Le <= len && pairs < pairs_per_item) { pairs += len - Le + 1; ++Le; }
      items.push_back({(int32_t)r, (int32_t)len, (int32_t)L, (int32_t)Le});
      L = Le;
    }
  }
}
// best[i]: what the kernel found for item i.  One candidate per run: its best subsegment (the whole run when nothing scored),
// typed by the median of the status values it covers, kept when its score reaches half of tlamda.
inline void segments_from_best(const std::vector<Region>& runs, const std::vector<rsik::SegItem>& items, const rsik::BestSeg* best,
                               const IntSpan& status2, double tlamda, std::vector<Candidate>& segs) {
  std::vector<rsik::BestSeg> per_run(runs.size(), rsik::BestSeg{-1.0, 0, 0});
  for (size_t i = 0; i < items.size(); ++i) {   // items of a run are in increasing L: strict > keeps the earliest
    rsik::BestSeg& b = per_run[(size_t)items[i].run];
    if (best[i].score > b.score) b = best[i];
  }
  for (size_t r = 0; r < runs.size(); ++r) {
    Candidate c;
    const int len = runs[r].end - runs[r].start + 1;
    double sc = per_run[r].score;
    if (sc > 0) { c.start = runs[r].start + per_run[r].start; c.end = c.start + per_run[r].len - 1; }
    else { c.start = runs[r].start; c.end = runs[r].start + len - 1; sc = 0; }
    const Quantiles q = grid_quantiles(status2.at(c.start), (size_t)(c.end - c.start + 1));
    if (q.med > 0) { c.type = kDup; c.score = sc; } else { c.type = kDel; c.score = -sc; }
    if (fabs(c.score) < tlamda * 0.5) continue;   // rsi.cpp:1343-1346
    segs.push_back(c);
  }
}

}  // namespace rsih
