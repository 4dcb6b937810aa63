// tests/calls_harness.cpp -- the tester-less path of the three list stages (test_block_segments, merge_neighbours, call_from_segments of
// rsicnv_amd/csrc/host_calls.cpp) on the cases of tests/calls_cases.py, in a stand-alone program built with ASan + UBSan by
// tests/test_calls_host.py.  No GPU is touched: the depth is host memory behind DepthPager's host constructor.
//
//   calls_harness CASES OUT
//
// CASES (little endian): int32 count, then per case
//   int32 stage (0 block, 1 merge, 2 calls), n, ncand, nnoncode, span_all, sparse, m, maxchkbp, merge;
//   double minmlen, chklen, buffer, p, RDmedian, RDsd;
//   int32 depth[n]; int32 status[n] (stage 0 only); rsi_call cands[ncand]; int32 noncode[2 nnoncode] (start, end pairs).
// OUT: per case the lists the stage returns (one for stage 0 and 1; blocks, raw, kept for stage 2), each as int32 count + rsi_call records.
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "../rsicnv_amd/csrc/host_calls.h"

using rsih::Candidate;

static bool get(FILE* f, void* p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, f) == bytes; }

static Candidate from_call(const rsi_call& c) {
  Candidate k;
  k.type = c.type; k.geno = c.geno; k.status = c.status; k.start = c.start; k.end = c.end; k.length = c.length;
  k.score = c.score; k.p1 = c.p1; k.cnvmed = c.cnvmed; k.cnvsd = c.cnvsd; k.cnviqr = c.cnviqr; k.refmed = c.refmed; k.refsd = c.refsd;
  k.refiqr = c.refiqr;
  return k;
}

static void put_list(FILE* f, const std::vector<Candidate>& L) {
  const int32_t n = (int32_t)L.size();
  fwrite(&n, 4, 1, f);
  for (const Candidate& k : L) {
    rsi_call c;
    memset(&c, 0, sizeof(c));
    c.type = k.type; c.geno = k.geno; c.status = k.status; c.start = k.start; c.end = k.end; c.length = k.length;
    c.score = k.score; c.p1 = k.p1; c.cnvmed = k.cnvmed; c.cnvsd = k.cnvsd; c.cnviqr = k.cnviqr; c.refmed = k.refmed; c.refsd = k.refsd;
    c.refiqr = k.refiqr;
    fwrite(&c, sizeof(c), 1, f);
  }
}

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: calls_harness CASES OUT\n"); return 2; }
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) { fprintf(stderr, "error: cannot open the files\n"); return 2; }
  int32_t count = 0;
  if (!get(in, &count, 4)) { fprintf(stderr, "error: no case count\n"); return 2; }
  for (int32_t k = 0; k < count; ++k) {
    int32_t h[9];
    double d[6];
    if (!get(in, h, sizeof(h)) || !get(in, d, sizeof(d))) { fprintf(stderr, "error: case %d: short header\n", k); return 2; }
    const int stage = h[0], n = h[1], ncand = h[2], nnoncode = h[3], span_all = h[4], sparse = h[5];
    if (stage < 0 || stage > 2 || n < 1 || ncand < 0 || nnoncode < 0) { fprintf(stderr, "error: case %d: bad header\n", k); return 2; }
    std::vector<int32_t> depth((size_t)n), status(stage == 0 ? (size_t)n : 0), nc(2 * (size_t)nnoncode);
    std::vector<rsi_call> calls((size_t)ncand);
    if (!get(in, depth.data(), depth.size() * 4) || !get(in, status.data(), status.size() * 4) || !get(in, calls.data(), calls.size() * sizeof(rsi_call)) ||
        !get(in, nc.data(), nc.size() * 4)) {
      fprintf(stderr, "error: case %d: short body\n", k);
      return 2;
    }
    rsih::CallerInput ci{};   // (the stages read no other field of P than the seven set here)
    ci.P.m = h[6]; ci.P.maxchkbp = h[7]; ci.P.merge = h[8];
    ci.P.minmlen = d[0]; ci.P.chklen = d[1]; ci.P.buffer = d[2]; ci.P.p = d[3];
    ci.RDmedian = d[4]; ci.RDsd = d[5];
    ci.ncompact = span_all;
    std::vector<rsih::Region> regions;
    for (int i = 0; i < nnoncode; ++i) regions.push_back(rsih::Region{nc[2 * (size_t)i], nc[2 * (size_t)i + 1]});
    ci.noncode = &regions;
    int short_neighbourhoods = 0;
    ci.short_neighbourhoods = &short_neighbourhoods;
    std::vector<Candidate> L;
    for (const rsi_call& c : calls) L.push_back(from_call(c));
    if (stage == 0) {
      std::vector<int> bins(depth.begin(), depth.end()), st(status.begin(), status.end());
      ci.binmedint = rsih::IntSpan(bins);
      // the sparse form as the scan leaves it: the values inside the maximal runs of non-zero status, run after run
      std::vector<int> run_status;
      std::vector<rsih::IntSpan::Range> ranges;
      for (int64_t i = 0; i < n;) {
        if (st[(size_t)i] == 0) { ++i; continue; }
        int64_t j = i;
        while (j + 1 < n && st[(size_t)j + 1] != 0) ++j;
        ranges.push_back({i, j, (int64_t)run_status.size()});
        run_status.insert(run_status.end(), st.begin() + i, st.begin() + j + 1);
        i = j + 1;
      }
      if (sparse && ranges.empty()) { fprintf(stderr, "error: case %d: the sparse form needs a marked run\n", k); return 2; }
      // (run_status is exactly as long as the runs: a look-up outside them that did not return the shared zero would be caught here)
      rsih::test_block_segments(ci, sparse ? rsih::IntSpan(run_status.data(), n, &ranges) : rsih::IntSpan(st), L);
      put_list(out, L);
    } else if (stage == 1) {
      rsih::DepthPager pager(depth.data(), n);
      rsih::debug_merge_neighbours(ci, pager, L);
      put_list(out, L);
    } else {
      rsih::DepthPager pager(depth.data(), n);
      std::vector<Candidate> blocks, raw, kept;
      rsih::call_from_segments(ci, L, pager, blocks, raw, kept);
      put_list(out, blocks);
      put_list(out, raw);
      put_list(out, kept);
    }
    if (short_neighbourhoods) { fprintf(stderr, "error: case %d: a neighbourhood no longer than its candidate\n", k); return 2; }
  }
  fclose(in);
  if (fclose(out) != 0) { fprintf(stderr, "error: writing the results failed\n"); return 2; }
  printf("%d cases\n", count);
  return 0;
}
