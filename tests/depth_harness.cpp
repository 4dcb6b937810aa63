// depth_harness.cpp -- stand-alone driver of rsicnv_amd/csrc/depth_host.h for tests/test_depth_host.py, built with
// -fsanitize=address,undefined: the rounding rule, the window table, clipping, the slice plan, the BED reader and the two
// writers, one job per line of the job file, answers on stdout behind a "job K" line each.
//   H S L                                  -> the mean as text
//   W n W                                  -> the window count, then "start end" per window
//   C start end n                          -> "a b kept" (clipped), then "s e" (written)
//   P name_len count slice_lines           -> "slice max_line text_cap" or "bad"
//   B path                                 -> "ok" and "chrom start end" per line, or "bad <message>"
//   S k (name length bases min max) x k    -> PREFIX.mosdepth.summary.txt
//   D name n max k (depth count) x k       -> the chromosome's lines of PREFIX.mosdepth.global.dist.txt
#include <fstream>
#include <iostream>
#include <sstream>

#include "../rsicnv_amd/csrc/depth_host.h"

int main(int argc, char** argv) {
  if (argc < 2) { std::cerr << "usage: depth_harness JOBFILE\n"; return 2; }
  std::ifstream in(argv[1]);
  std::string text;
  int k = 0;
  while (std::getline(in, text)) {
    if (text.empty()) continue;
    std::istringstream iss(text);
    char what = 0;
    iss >> what;
    std::cout << "job " << k++ << "\n";
    if (what == 'H') {
      long long S = 0, L = 0;
      iss >> S >> L;
      std::cout << rsidepth::fixed2(S, L) << "\n";
    } else if (what == 'W') {
      long long n = 0, W = 0;
      iss >> n >> W;
      const int64_t count = rsidepth::window_count(n, W);
      std::cout << count << "\n";
      for (int64_t w = 0; w < count; ++w) { int64_t s, e; rsidepth::window(w, W, n, s, e); std::cout << s << " " << e << "\n"; }
    } else if (what == 'C') {
      long long start = 0, end = 0, n = 0;
      iss >> start >> end >> n;
      int64_t a, b, s, e;
      const bool kept = rsidepth::clip(start, end, n, a, b);
      rsidepth::written(start, end, n, s, e);
      std::cout << a << " " << b << " " << (kept ? 1 : 0) << "\n" << s << " " << e << "\n";
    } else if (what == 'P') {
      int name_len = 0;
      long long count = 0, slice = 0;
      iss >> name_len >> count >> slice;
      rsidepth::Plan p;
      if (!rsidepth::plan(name_len, count, slice, p)) std::cout << "bad\n";
      else std::cout << p.slice << " " << p.max_line << " " << p.text_cap << "\n";
    } else if (what == 'B') {
      std::string path, err;
      iss >> path;
      std::ifstream bed(path.c_str());
      std::vector<rsidepth::BedLine> lines;
      if (!rsidepth::read_bed(bed, path, lines, err)) { std::cout << "bad " << err << "\n"; continue; }
      std::cout << "ok\n";
      for (const rsidepth::BedLine& l : lines) std::cout << l.chrom << " " << l.start << " " << l.end << "\n";
    } else if (what == 'S') {
      size_t count = 0;
      iss >> count;
      std::vector<rsidepth::ChromSummary> rows(count);   // exactly as long as the list: a read past it is the sanitizer's
      for (rsidepth::ChromSummary& r : rows) iss >> r.name >> r.length >> r.bases >> r.min >> r.max;
      rsidepth::write_summary(std::cout, rows);
    } else if (what == 'D') {
      std::string name;
      long long n = 0, top = 0;
      size_t count = 0;
      iss >> name >> n >> top >> count;
      std::vector<int64_t> dist(rsidepth::kDistBins, 0);
      for (size_t i = 0; i < count; ++i) { long long d = 0, c = 0; iss >> d >> c; dist[(size_t)d] = c; }
      rsidepth::write_dist(std::cout, name, dist.data(), n, (int32_t)top);
    } else {
      std::cout << "error: unknown job " << what << "\n";
    }
  }
  return 0;
}
