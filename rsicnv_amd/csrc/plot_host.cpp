// plot_host.cpp -- the data (.dat) and script (.gp) files of a call's gnuplot figure, as plot_icnv writes them
// (plotcnv.cpp:245-610), behind the command line's -p and behind `rsicnv view`.  The text rules live here once: a figure is planned
// (plot_plan.h: which rows, which values), filled -- from an array in host memory here (fill_host), or on the device from one in
// HBM (plot.hip) -- and written (write_planned).  rsi_plot_write_files is plan + fill_host + write_planned over the
// capped, GC-adjusted depth a run leaves (rsi_hot_fetch "rd_concat"), expanded by the removed N regions (expand_data,
// loaddata.cpp:140-183).  The reference runs gnuplot on the pair and deletes both files; this writer only produces them (the
// command line runs gnuplot when there is one, and keeps the files when not).
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/rsi_hot.h"
#include "hostmath.h"
#include "plot_plan.h"

namespace {

const char* kType[3] = {"DEL", "DUP", "UNKNOWN"};

// _lowerquartile / _median / _upperquartile on ints (partition_stat_tp with dy = 1, wufunctions.cpp:364-424) in closed form: of n >= 1
// sorted values s[], s[max(n/4,1)-1], s[max(n/2,1)-1], s[max(3n/4,1)-1] -- what rsih::grid_quantiles<int> walks a counter per unit
// of max - min for, all-equal values included (their mean is their value).  v is reordered.
void rank_quantiles(std::vector<int>& v, double q[3]) {
  const size_t n = v.size();
  const size_t r[3] = {n / 4, n / 2, n * 3 / 4};
  for (int k = 0; k < 3; ++k) {
    const size_t at = std::max<size_t>(r[k], 1) - 1;
    std::nth_element(v.begin(), v.begin() + (ptrdiff_t)at, v.end());
    q[k] = (double)v[at];
  }
}

}  // namespace

namespace rsiplot {

// The host's fill: the neighbourhood gathered, its prefix sums, a window sum per running-mean query -- runmeantp with end_rule = 1
// (wufunctions.cpp:573-647) is the mean of the window around the clamped centre, and a sum of ints is the same in any order.
void fill_host(const Plan& P, const int32_t* rd, Filled& F) {
  F = Filled{};
  if (P.refusal != kOk) return;
  std::vector<int> ref;
  ref.reserve((size_t)P.nref);
  for (int i = P.a0; i < P.a1; ++i) ref.push_back(rd[i]);
  for (int i = P.b0; i < P.b1; ++i) ref.push_back(rd[i]);
  std::vector<int64_t> pre((size_t)P.nref + 1, 0);
  for (int i = 0; i < P.nref; ++i) pre[(size_t)i + 1] = pre[(size_t)i] + ref[(size_t)i];
  F.ref_sum = pre[(size_t)P.nref];
  std::vector<int> body(rd + P.c1, rd + P.c2 + 1);
  rank_quantiles(body, F.body_q);
  rank_quantiles(ref, F.ref_q);   // (the prefix sums are taken: ref may be reordered)
  F.value.assign(P.q.size(), 0);
  F.wsum.assign(P.q.size(), 0);
  const int h = P.band / 2;
  for (size_t k = 0; k < P.q.size(); ++k) {
    const Query& q = P.q[k];
    if (q.depth >= 0) F.value[k] = rd[q.depth];
    if (q.ref >= 0) { const int c = window_centre(q.ref, P.band, P.nref); F.wsum[k] = pre[(size_t)(c + h + 1)] - pre[(size_t)(c - h)]; }
  }
}

int write_planned(const Plan& P, const Filled& F, int length, int type, double p1, const char* title_in, double chrom_median, const char* format,
                  double gnuplot_version, const char* datfile, const char* gpfile, const char* imgfile) {
  if (P.refusal != kOk || !title_in || !format || !datfile || !gpfile || !imgfile) return RSI_ERR_BAD_ARG;
  if (F.value.size() != P.q.size() || F.wsum.size() != P.q.size()) return RSI_ERR_BAD_ARG;
  const int cs = P.cs, ce = P.ce;
  int i1 = P.i1, i2 = P.i2;
  std::string term = "png xffffff x222222";
  const std::string fmt = format;
  if (fmt == "ps") term = "postscript color enhanced solid";
  if (fmt == "eps") term = "postscript eps enhanced solid";
  const double refmean = (double)F.ref_sum / double(P.nref);
  struct Q3 { double lqt, med, uqt; };
  const Q3 qc{F.body_q[0], F.body_q[1], F.body_q[2]}, qr{F.ref_q[0], F.ref_q[1], F.ref_q[2]};
  int ymax = (int)(qr.med * 2.25);
  const double y2max = (double)ymax / refmean / 2.0;
  if (qc.med < qr.med) ymax = (int)(qr.med * 2);
  else ymax = (int)(qc.uqt + 1.5 * (qr.uqt - qr.lqt));
  // the float overload of runmeantp rounds every mean to float (wufunctions.cpp:640-646)
  auto runmean = [&](size_t k) { return (float)((double)F.wsum[k] / double(P.band)); };

  std::ofstream D(datfile);
  if (!D) return RSI_ERR_BAD_ARG;
  D << "#" << cs << " ~ " << ce << "  " << length << "  " << kType[type < 0 || type > 2 ? 2 : type] << "  " << p1 << std::endl;
  int RDmax = 0;
  size_t k = 0;
  // blocks 0 - 2: in front of the call, the call, behind it: position, depth, running mean of the neighbourhood (none in the call)
  for (int b = 0; b < 3; ++b) {
    for (int r = 0; r < P.rows[b]; ++r, ++k) {
      const Query& q = P.q[k];
      if (q.depth < 0) { D << q.pos << "\t0\tNaN" << std::endl; continue; }
      D << q.pos << "\t" << F.value[k] << "\t";
      if (q.ref >= 0) D << runmean(k); else D << "NaN";
      D << std::endl;
      if (q.depth > 0 && F.value[k] > RDmax) RDmax = F.value[k];
    }
    D << std::endl << std::endl;
  }
  // block 3: the line that joins the two running means
  D << cs << "\t" << runmean(k) << std::endl << ce << "\t" << runmean(k + 1) << std::endl;
  D << std::endl << std::endl;
  // blocks 4-6: median and quartiles of the call; 7-9: of the neighbourhood; 10: nothing
  const double cq[3] = {qc.med, qc.lqt, qc.uqt}, rq[3] = {qr.med, qr.lqt, qr.uqt};
  for (int b = 0; b < 3; ++b) D << cs << "\t" << cq[b] << std::endl << ce << "\t" << cq[b] << std::endl << std::endl << std::endl;
  for (int b = 0; b < 3; ++b) D << i1 << "\t" << rq[b] << std::endl << i2 << "\t" << rq[b] << std::endl << std::endl << std::endl;
  D << "NaN\tNaN\n" << "NaN\tNaN\n" << std::endl << std::endl;
  D.close();

  std::string title = title_in;
  std::replace(title.begin(), title.end(), '~', '-');
  if (ymax > RDmax) ymax = RDmax + RDmax / 10;
  int d = (i2 - i1 + 1) / 6;
  i1 = i1 + d / 2;
  i2 = i2 - d / 2;
  std::ofstream G(gpfile);
  if (!G) return RSI_ERR_BAD_ARG;
  if (gnuplot_version > 4.19) {
    G << "f=\"" << datfile << "\"" << std::endl
      << "set datafile missing 'NaN'" << std::endl
      << "info=\"" << title << " \"" << std::endl
      << "set terminal " << term << std::endl
      << "set output \"" << imgfile << "\"" << std::endl
      << "#set nokey" << std::endl
      << "##set label 1 info at graph  0.25, graph  0.9" << std::endl
      << "set title info offset 0,-0.5" << std::endl
      << "set xrange [" << i1 << ":" << i2 << "]" << std::endl
      << "set xtics " << i1 << "," << d << "," << i2 << std::endl
      << "set yrange [0:" << ymax << "]" << std::endl;
    G << "set y2range[0:" << y2max << "]" << std::endl;
    G << "set ytics nomirror" << std::endl;
    G << "plot \\" << std::endl
      << "f in 0 u 1:2 w p pt 7 ps 0.5 lt rgb \"blue\" t \"Neighbor\", \\" << std::endl
      << "f in 1 u 1:2 w p pt 7 ps 0.5 lt rgb \"red\" t \"CNV\", \\" << std::endl
      << "f in 2 u 1:2 w p pt 7 ps 0.5 lt rgb \"blue\" not, \\" << std::endl
      << "f in 0 u 1:3 w l lt 1 lw 8 lc rgb \"green\" t \"Runmean\", \\" << std::endl
      << "f in 2 u 1:3 w l lt 1 lw 8 lc rgb \"green\" not, \\" << std::endl
      << "f in 3 u 1:2 w l lt 0 lw 8 lc rgb \"green\" not, \\" << std::endl
      << "f in 4 u 1:2 w l lt 1 lw 8 lc rgb \"cyan\" t \"CNV med\", \\" << std::endl
      << "f in 5 u 1:2 w l lt 0 lw 8 lc rgb \"cyan\" t \"CNV 1st,3rd quart\", \\" << std::endl
      << "f in 6 u 1:2 w l lt 0 lw 8 lc rgb \"cyan\" not, \\" << std::endl
      << qr.lqt << " w l lt 0 lw 8 lc rgb \"green\" t \"Neighbor 1st,3rd quar\", \\" << std::endl
      << qr.uqt << " w l lt 0 lw 8 lc rgb \"green\" not, \\" << std::endl;
    if (chrom_median > 0) G << chrom_median << " w l lt 4 lw 4 t \"CHROM med\", \\" << std::endl;
    G << "f in 10 u 1:2 not" << std::endl;
  } else {   // gnuplot up to 4.1: no string variables, no rgb colours
    G << "#f=\"" << datfile << "\"" << std::endl
      << "#info=\"" << title << " \"" << std::endl
      << "set terminal " << term << std::endl
      << "set output \"" << imgfile << "\"" << std::endl
      << "#set nokey" << std::endl
      << "set title \"" << title << "\"" << " 0,-0.5" << std::endl
      << "set xrange [" << i1 << ":" << i2 << "]" << std::endl
      << "set xtics " << i1 << "," << d << "," << i2 << std::endl
      << "set yrange [0:" << ymax << "]" << std::endl;
    G << "set ytics nomirror" << std::endl;
    G << "set y2range[0:" << y2max << "]" << std::endl;
    G << "plot \\" << std::endl
      << "\"" << datfile << "\" in 0 u 1:2 w p pt 7 ps 0.5 lt 3 not, \\" << std::endl
      << "\"" << datfile << "\" in 1 u 1:2 w p pt 7 ps 0.5 lt 1 not, \\" << std::endl
      << "\"" << datfile << "\" in 2 u 1:2 w p pt 7 ps 0.5 lt 3 not, \\" << std::endl
      << "\"" << datfile << "\" in 0 u 1:3 w l lt 2 lw 8 t \"runmean\", \\" << std::endl
      << "\"" << datfile << "\" in 2 u 1:3 w l lt 2 lw 8 not, \\" << std::endl
      << "\"" << datfile << "\" in 3 u 1:2 w l lt 2 lw 2 not, \\" << std::endl
      << "\"" << datfile << "\" in 4 u 1:2 w l lt 5 lw 8 t \"CNV med\", \\" << std::endl
      << "\"" << datfile << "\" in 5 u 1:2 w l lt 5 lw 4 t \"CNV 1st,3rd quart\", \\" << std::endl
      << "\"" << datfile << "\" in 6 u 1:2 w l lt 5 lw 4 not, \\" << std::endl
      << qr.lqt << " w l lt 2 lw 2 t \"Neighbor 1st,3rd quart\", \\" << std::endl
      << qr.uqt << " w l lt 2 lw 2 not , \\" << std::endl;
    if (chrom_median > 0) G << chrom_median << " w l lt 4 lw 4 t \"WG mean\", \\" << std::endl;
    G << "\"" << datfile << "\" in 10 u 1:2 not" << std::endl;
  }
  G << "set output" << std::endl << "quit" << std::endl;
  return RSI_OK;
}

}  // namespace rsiplot

extern "C" {

// Writes <base>.dat and <base>.gp for call `c` (coordinates in the expanded array, as printed in the output table).
// rd: the expanded per-base depth (n values); chrom_median: _median of that array (plot::RDmed, plotcnv.cpp:625);
// m / minmlen / chklen: the run's parameters (rsi.cpp:34-98); format: "ps", "eps" or "png" (plot::format);
// gnuplot_version: what `gnuplot -V` reports, -1 = none found (gnuplot_version(), plotcnv.cpp:51-65).  The script has two
// dialects and the reference picks the newer one only above 4.19 (plotcnv.cpp:512) -- "none found" gets the older one.
// Returns RSI_OK, or RSI_ERR_BAD_ARG when the call lies outside the array (the reference draws an empty frame there).
int rsi_plot_write_files(const rsi_call* c, const char* title_in, const int32_t* rd, int64_t n, double chrom_median, int m,
                         double minmlen, double chklen, const char* format, double gnuplot_version, const char* datfile,
                         const char* gpfile, const char* imgfile) {
  if (!c || !title_in || !rd || n <= 0 || !format || !datfile || !gpfile || !imgfile) return RSI_ERR_BAD_ARG;
  const rsiplot::Plan P = rsiplot::plan_call(c->start, c->end, n, m, minmlen, chklen);
  if (P.refusal != rsiplot::kOk) return RSI_ERR_BAD_ARG;
  rsiplot::Filled F;
  rsiplot::fill_host(P, rd, F);
  return rsiplot::write_planned(P, F, c->length, c->type, c->p1, title_in, chrom_median, format, gnuplot_version, datfile, gpfile, imgfile);
}

rsi_plot_batch* rsi_plot_batch_new(int64_t n, int m, double minmlen, double chklen) {
  if (n <= 0 || n >= (1ll << 31) - 4096 || m < 1) return nullptr;
  rsi_plot_batch* b = new rsi_plot_batch;
  b->n = n; b->m = m; b->minmlen = minmlen; b->chklen = chklen;
  return b;
}
void rsi_plot_batch_free(rsi_plot_batch* b) { delete b; }
int rsi_plot_batch_add(rsi_plot_batch* b, const rsi_call* c) {
  if (!b || !c) return RSI_ERR_BAD_ARG;
  b->calls.push_back(*c);
  b->plans.push_back(rsiplot::plan_call(c->start, c->end, b->n, b->m, b->minmlen, b->chklen));
  b->is_filled = false;
  return b->plans.back().refusal;
}
int rsi_plot_batch_add_span(rsi_plot_batch* b, int start, int end, int type) {
  rsi_call c;
  memset(&c, 0, sizeof(c));
  c.start = start; c.end = end; c.type = type; c.p1 = 1.0;   // cnv_st's defaults: length 0, p1 1
  return rsi_plot_batch_add(b, &c);
}
int rsi_plot_batch_size(const rsi_plot_batch* b) { return b ? (int)b->plans.size() : 0; }
int rsi_plot_batch_refusal(const rsi_plot_batch* b, int i) { return (!b || i < 0 || i >= (int)b->plans.size()) ? RSI_ERR_BAD_ARG : b->plans[(size_t)i].refusal; }
const char* rsi_plot_refusal_text(int refusal) { return rsiplot::refusal_text(refusal); }
int64_t rsi_plot_batch_queries(const rsi_plot_batch* b) {
  int64_t k = 0;
  if (b) for (const rsiplot::Plan& P : b->plans) k += (int64_t)P.q.size();
  return k;
}
int rsi_plot_batch_fill_host(rsi_plot_batch* b, const int32_t* rd, int64_t n) {
  if (!b || !rd || n != b->n) return RSI_ERR_BAD_ARG;
  b->filled.assign(b->plans.size(), rsiplot::Filled{});
  for (size_t i = 0; i < b->plans.size(); ++i) rsiplot::fill_host(b->plans[i], rd, b->filled[i]);
  bool any = false;
  for (const rsiplot::Plan& P : b->plans) any = any || P.refusal == rsiplot::kOk;
  b->chrom_median = 0;
  if (any) {   // plot::RDmed, plotcnv.cpp:625 (nothing to write: no median either, as on the device)
    std::vector<int> all(rd, rd + n);
    double q[3];
    rank_quantiles(all, q);
    b->chrom_median = q[1];
  }
  b->is_filled = true;
  return RSI_OK;
}
int rsi_plot_batch_compare(const rsi_plot_batch* a, const rsi_plot_batch* b) {
  if (!a || !b || !a->is_filled || !b->is_filled || a->plans.size() != b->plans.size()) return RSI_ERR_BAD_ARG;
  for (size_t i = 0; i < a->plans.size(); ++i) {
    const rsiplot::Filled& x = a->filled[i], & y = b->filled[i];
    if (a->plans[i].refusal != b->plans[i].refusal || x.value != y.value || x.wsum != y.wsum || x.ref_sum != y.ref_sum ||
        memcmp(x.body_q, y.body_q, sizeof x.body_q) != 0 || memcmp(x.ref_q, y.ref_q, sizeof x.ref_q) != 0)
      return (int)i + 1;
  }
  if (memcmp(&a->chrom_median, &b->chrom_median, sizeof(double)) != 0) return (int)a->plans.size() + 1;
  return 0;
}
double rsi_plot_batch_chrom_median(const rsi_plot_batch* b) { return b && b->is_filled ? b->chrom_median : 0.0; }
int rsi_plot_batch_write(const rsi_plot_batch* b, int i, const char* title, const char* format, double gnuplot_version, const char* datfile,
                         const char* gpfile, const char* imgfile) {
  if (!b || !b->is_filled || i < 0 || i >= (int)b->plans.size()) return RSI_ERR_BAD_ARG;
  const rsi_call& c = b->calls[(size_t)i];
  return rsiplot::write_planned(b->plans[(size_t)i], b->filled[(size_t)i], c.length, c.type, c.p1, title, b->chrom_median, format, gnuplot_version,
                                datfile, gpfile, imgfile);
}

// expand_data (loaddata.cpp:140-183): the compacted array with the removed regions back in, as zeros.  regions: npairs
// (start, end) pairs in reference coordinates, ascending; out: n values.
int rsi_plot_expand(const int32_t* rdc, int64_t ncompact, const int32_t* regions, int npairs, int32_t* out, int64_t n) {
  if (!rdc || !out || ncompact < 0 || n < ncompact || (npairs > 0 && !regions)) return RSI_ERR_BAD_ARG;
  int64_t removed = 0;
  for (int k = 0; k < npairs; ++k) {
    if (regions[2 * k] < 0 || regions[2 * k + 1] < regions[2 * k] || regions[2 * k + 1] >= n || (k > 0 && regions[2 * k] <= regions[2 * k - 1])) return RSI_ERR_BAD_ARG;
    removed += (int64_t)regions[2 * k + 1] - regions[2 * k] + 1;
  }
  if (ncompact + removed != n) return RSI_ERR_BAD_ARG;   // "cannot expand RD array", loaddata.cpp:149-153
  int64_t src = 0, dst = 0;
  for (int k = 0; k < npairs; ++k) {
    const int64_t s = regions[2 * k], e = regions[2 * k + 1];
    while (dst < s && src < ncompact && dst < n) out[dst++] = rdc[src++];
    while (dst <= e && dst < n) out[dst++] = 0;
  }
  while (src < ncompact && dst < n) out[dst++] = rdc[src++];
  return (src == ncompact && dst == n) ? RSI_OK : RSI_ERR_BAD_ARG;
}

}  // extern "C"
