// plot_plan.h -- a call's gnuplot figure in three steps, plain C++ with no HIP in it, for plot_host.cpp, plot.hip,
// cli.cpp and tests/plot_harness.cpp:
//   plan   what plot_icnv (plotcnv.cpp:245-610) looks at, from the call and the array's length alone: the body, the two pieces of
//          the neighbourhood, the running mean's band, and one query per printed row -- which position to print, which depth value
//          and which running-mean value belong beside it;
//   fill   a value per query and, per running-mean query, the exact integer sum of its window; the six quantiles and the
//          neighbourhood's sum.  fill_host does it from an array in host memory, plot.hip from one in HBM;
//   write  the .dat and .gp bytes from a plan and its fill (plot_host.cpp: write_planned), whoever filled it.
#pragma once
#include <stdint.h>
#include <stdlib.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/rsi_hot.h"

namespace rsiplot {

constexpr int kPlotPoints = 30000;   // plot::pts, plotcnv.cpp:29

// what the writer refuses (the reference draws an empty frame or returns without a figure)
enum Refusal { kOk = 0, kBeyond = 1, kSizeError = 2, kEmptyBody = 3, kNoBand = 4 };
inline const char* refusal_text(int r) {
  switch (r) {
    case kOk: return "ok";
    case kBeyond: return "the call lies beyond the array";
    case kSizeError: return "size error: the neighbourhood does not fit the array";
    case kEmptyBody: return "the call holds no value of the array";
    default: return "no running-mean band fits the neighbourhood";
  }
}

// One printed row of blocks 0, 1, 2, or one of the two rows of block 3.  depth: index of the array value printed beside pos, -1
// for a "0 NaN" row (and for block 3, which prints none); ref: index into the neighbourhood (front piece, then back piece) whose
// running mean is printed, -1 for none.
struct Query { int32_t pos, depth, ref; };

struct Plan {
  int refusal = kOk;
  int cs = 0, ce = 0, i1 = 0, i2 = 0, c1 = 0, c2 = 0;   // as in plot_icnv: the call, the neighbourhood's ends (1-based), the body (0-based, inclusive)
  int a0 = 0, a1 = 0, b0 = 0, b1 = 0;                   // the neighbourhood's pieces, half-open ranges of the array: positions i1 .. cs-1, ce+1 .. i2
  int nref = 0, band = 0;                               // values in the neighbourhood; the running mean's window (odd)
  int rows[3] = {0, 0, 0};                              // queries of blocks 0, 1, 2; block 3's two follow
  std::vector<Query> q;
};

// the window of query index r: centre clamped so that the window lies inside the neighbourhood (runmeantp's end_rule = 1)
inline int window_centre(int r, int band, int nref) { const int h = band / 2; return std::min(std::max(r, h), nref - 1 - h); }

inline Plan plan_call(int start, int end, int64_t n, int m, double minmlen, double chklen) {
  Plan P;
  int cs = start, ce = end;
  if (cs > ce) std::swap(cs, ce);
  const int size = (int)n;
  P.cs = cs; P.ce = ce;
  if (cs > size || ce > size) { P.refusal = kBeyond; return P; }
  int d = ce - cs + 1;
  if (d < m * minmlen) d = (int)(m * minmlen);
  int i1 = (int)(cs - chklen * d), i2 = (int)(ce + chklen * d);
  if (i1 < 1) i1 = 1;
  if (i1 > size - 1) i1 = size - 1;
  if (i2 > size - 1) i2 = size - 1;
  int c1 = cs - 1, c2 = ce - 1;
  if (c1 < 0) c1 = 0;
  if (c1 >= size) c1 = size - 1;
  if (c2 >= size) c2 = size - 1;
  P.i1 = i1; P.i2 = i2; P.c1 = c1; P.c2 = c2;
  // the neighbourhood: positions i1 .. cs-1 and ce+1 .. i2, the value of position p at index p - 1
  P.nref = abs(cs - i1 + i2 - ce);
  P.a0 = i1 - 1; P.a1 = std::max(cs - 1, P.a0);
  P.b0 = ce;     P.b1 = std::max(i2, P.b0);
  const int k = (P.a1 - P.a0) + (P.b1 - P.b0);
  if (i1 < 1 || k != P.nref || P.nref == 0 || P.a1 > size || P.b1 > size || P.b0 < 0) { P.refusal = kSizeError; return P; }
  if (c2 - c1 + 1 <= 0) { P.refusal = kEmptyBody; return P; }
  d = abs(ce - cs) + 1;
  int band = d + ((d + 1) % 2) * 1;
  if (band > P.nref) band = P.nref / 2 + ((P.nref / 2 + 1) % 2) * 1;   // plotcnv.cpp:344-347
  while (band > P.nref) band -= 2;
  if (band <= 0) { P.refusal = kNoBand; return P; }
  P.band = band;

  double step = (double)(i2 - i1 + 1) / (double)kPlotPoints;
  if (step < 1.0) step = 1.0;
  int i = 0;
  // block 0: in front of the call.  Its last row is position cs, whose running-mean index cs - i1 is the back piece's first value;
  // with an empty back piece that is one past the neighbourhood (the reference reads past its array there): the last value's mean
  for (double ir = (double)i1 + 0.00001; ir < (double)cs + 0.000011; ir += step) {
    i = (int)ir;
    const int ic = i - 1;
    if (ic < 0 || ic >= size) P.q.push_back(Query{i, -1, -1});
    else P.q.push_back(Query{i, ic, std::min(i - i1, P.nref - 1)});
  }
  P.rows[0] = (int)P.q.size();
  // block 1: the call
  for (double ir = (double)cs + 0.00001; ir <= (double)ce + 0.000011; ir += step) {
    const int ic = (int)(ir - 1);
    if (ic < 0 || ic >= size) P.q.push_back(Query{i, -1, -1});
    else P.q.push_back(Query{(int)ir, ic, -1});
  }
  P.rows[1] = (int)P.q.size() - P.rows[0];
  // block 2: behind the call
  for (double ir = (double)ce + 1.00001; ir <= (double)i2 + 0.000011; ir += step) {
    const int ic = (int)(ir - 1);
    if (ic < 0 || ic >= size) { P.q.push_back(Query{i, -1, -1}); continue; }
    const int ri = (int)(ir - i1 - d);
    P.q.push_back(Query{(int)ir, ic, std::min(std::max(ri, 0), P.nref - 1)});
  }
  P.rows[2] = (int)P.q.size() - P.rows[0] - P.rows[1];
  // block 3: the line that joins the two running means
  int imid1 = cs - 3 - i1, imid2 = ce + 1 - i1 - d;
  if (imid1 < 0) imid1 = 0;
  if (imid2 >= P.nref) imid2 = P.nref - 1;
  if (imid2 < 0) imid2 = 0;
  P.q.push_back(Query{cs, -1, imid1});
  P.q.push_back(Query{ce, -1, imid2});
  return P;
}

// What a fill leaves per call: value[k] / wsum[k] beside query k (0 where the query asks for none), the quantiles as (lower
// quartile, median, upper quartile) of partition_stat_tp, the neighbourhood's sum.
struct Filled {
  std::vector<int32_t> value;
  std::vector<int64_t> wsum;
  double body_q[3] = {0, 0, 0}, ref_q[3] = {0, 0, 0};
  int64_t ref_sum = 0;
};

void fill_host(const Plan& P, const int32_t* rd, Filled& F);

// The .dat and .gp files of a planned and filled call; length / type / p1 go into the data file's first line.  Returns RSI_OK, or
// RSI_ERR_BAD_ARG for a refused plan or a file that cannot be written.
int write_planned(const Plan& P, const Filled& F, int length, int type, double p1, const char* title, double chrom_median, const char* format,
                  double gnuplot_version, const char* datfile, const char* gpfile, const char* imgfile);

}  // namespace rsiplot

// A list of calls planned against one array length, and what a fill left for them (include/rsi_hot.h: rsi_plot_batch_*).
struct rsi_plot_batch {
  int64_t n = 0;
  int m = 0;
  double minmlen = 0, chklen = 0;
  std::vector<rsi_call> calls;
  std::vector<rsiplot::Plan> plans;
  std::vector<rsiplot::Filled> filled;
  double chrom_median = 0;
  bool is_filled = false;
};
