// geno_harness.cpp -- stand-alone driver of rsicnv_amd/csrc/geno_host.h for tests/test_geno_host.py, built with
// -fsanitize=address,undefined: the region mapping, the flanks, the tile table, the ranks and the formatted field, one job per
// line of the job file, answers on stdout behind a "job K" line each.
//   M n npairs s0 e0 ... start end        -> "a b"
//   L a b m ncompact                      -> "lo hi flo0 fhi0 flo1 fhi1"
//   T tile ncompact nlines (6 ints each)  -> "ok|bad", then one "job off len" line per tile
//   R n                                   -> the three 1-based ranks
//   F n_body n_flank body_med flank_med chrom_median ploidy -> the field
#include <fstream>
#include <iostream>
#include <sstream>

#include "../rsicnv_amd/csrc/geno_host.h"

int main(int argc, char** argv) {
  if (argc < 2) { std::cerr << "usage: geno_harness JOBFILE\n"; return 2; }
  std::ifstream in(argv[1]);
  std::string text;
  int k = 0;
  while (std::getline(in, text)) {
    if (text.empty()) continue;
    std::istringstream iss(text);
    char what = 0;
    iss >> what;
    std::cout << "job " << k++ << "\n";
    if (what == 'M') {
      long long n = 0, start = 0, end = 0;
      int npairs = 0;
      iss >> n >> npairs;
      std::vector<int32_t> pairs((size_t)npairs * 2);   // exactly as long as the list: a read past it is the sanitizer's
      for (int32_t& p : pairs) iss >> p;
      iss >> start >> end;
      const rsigeno::Span s = rsigeno::map_line(start, end, n, pairs.data(), npairs);
      std::cout << s.a << " " << s.b << "\n";
    } else if (what == 'L') {
      rsigeno::Span b;
      long long m = 0, nc = 0;
      iss >> b.a >> b.b >> m >> nc;
      const rsigeno::Ranges r = rsigeno::line_ranges(b, m, nc);
      std::cout << r.body.a << " " << r.body.b << " " << r.left.a << " " << r.left.b << " " << r.right.a << " " << r.right.b << "\n";
    } else if (what == 'T') {
      int tile = 0;
      long long nc = 0;
      size_t nl = 0;
      iss >> tile >> nc >> nl;
      std::vector<rsigeno::Ranges> lines(nl);
      for (rsigeno::Ranges& r : lines) iss >> r.body.a >> r.body.b >> r.left.a >> r.left.b >> r.right.a >> r.right.b;
      std::vector<rsigeno::Tile> tiles;
      const bool ok = rsigeno::build_tiles(lines, nc, tile, tiles);
      std::cout << (ok ? "ok" : "bad") << "\n";
      if (ok) for (const rsigeno::Tile& t : tiles) std::cout << t.job << " " << t.off << " " << t.len << "\n";
    } else if (what == 'R') {
      long long n = 0;
      iss >> n;
      std::cout << rsigeno::rank1(n, 0) << " " << rsigeno::rank1(n, 1) << " " << rsigeno::rank1(n, 2) << "\n";
    } else if (what == 'F') {
      long long nb = 0, nf = 0;
      double bm = 0, fm = 0, cm = 0, pl = 2;
      iss >> nb >> nf >> bm >> fm >> cm >> pl;
      std::cout << rsigeno::format_field(nb, nf, bm, fm, cm, pl) << "\n";
    } else {
      std::cout << "error: unknown job " << what << "\n";
    }
  }
  return 0;
}
