// plot_harness.cpp -- stand-alone driver of rsicnv_amd/csrc/plot_host.cpp and plot_plan.h for tests/test_plot_host.py, built with
// -fsanitize=address,undefined: a call's two files on three roads, one job per line of the job file, "job K rc" on stdout each.
//   W ARRAY n start end type length p1 median version m minmlen chklen BASE TITLE...   rsi_plot_write_files
//   P (the same)                                                                       plan_call + fill_host + write_planned
//   B (the same)                                                                       rsi_plot_batch_new / _add / _fill_host / _write
//   R ARRAY n start end m minmlen chklen                                               "refusal nref band rows0 rows1 rows2" of the plan
// ARRAY: a file of n raw int32 values.  The files are BASE.dat and BASE.gp, the image name BASE.ps; rc is what the road returned
// (for B: the refusal's number when the call was refused, and then no file is written).
#include <fstream>
#include <iostream>
#include <sstream>

#include "../rsicnv_amd/csrc/plot_host.cpp"

int main(int argc, char** argv) {
  if (argc < 2) { std::cerr << "usage: plot_harness JOBFILE\n"; return 2; }
  std::ifstream in(argv[1]);
  std::string text;
  int k = 0;
  while (std::getline(in, text)) {
    if (text.empty()) continue;
    std::istringstream iss(text);
    char what = 0;
    std::string array;
    long long n = 0;
    iss >> what >> array >> n;
    std::vector<int32_t> rd((size_t)n);
    {
      std::ifstream a(array.c_str(), std::ios::binary);
      a.read(reinterpret_cast<char*>(rd.data()), (std::streamsize)(n * 4));
      if (a.gcount() != (std::streamsize)(n * 4)) { std::cout << "job " << k++ << " error: short array\n"; continue; }
    }
    if (what == 'R') {
      int start = 0, end = 0, m = 0;
      double minmlen = 0, chklen = 0;
      iss >> start >> end >> m >> minmlen >> chklen;
      const rsiplot::Plan P = rsiplot::plan_call(start, end, n, m, minmlen, chklen);
      std::cout << "job " << k++ << " " << P.refusal << " " << P.nref << " " << P.band << " " << P.rows[0] << " " << P.rows[1] << " " << P.rows[2] << "\n";
      continue;
    }
    rsi_call c;
    memset(&c, 0, sizeof(c));
    double median = 0, version = 0, minmlen = 0, chklen = 0;
    int m = 0;
    std::string base, title, word;
    iss >> c.start >> c.end >> c.type >> c.length >> c.p1 >> median >> version >> m >> minmlen >> chklen >> base;
    while (iss >> word) title += (title.empty() ? "" : " ") + word;
    const std::string dat = base + ".dat", gp = base + ".gp", img = base + ".ps";
    int rc = 0;
    if (what == 'W') {
      rc = rsi_plot_write_files(&c, title.c_str(), rd.data(), n, median, m, minmlen, chklen, "ps", version, dat.c_str(), gp.c_str(), img.c_str());
    } else if (what == 'P') {
      const rsiplot::Plan P = rsiplot::plan_call(c.start, c.end, n, m, minmlen, chklen);
      rsiplot::Filled F;
      rsiplot::fill_host(P, rd.data(), F);
      rc = rsiplot::write_planned(P, F, c.length, c.type, c.p1, title.c_str(), median, "ps", version, dat.c_str(), gp.c_str(), img.c_str());
    } else {
      rsi_plot_batch* b = rsi_plot_batch_new(n, m, minmlen, chklen);
      rc = rsi_plot_batch_add(b, &c);
      if (rc == 0) rc = rsi_plot_batch_fill_host(b, rd.data(), n);
      if (rc == 0) {
        b->chrom_median = median;   // the caller's, as on the other roads
        rc = rsi_plot_batch_write(b, 0, title.c_str(), "ps", version, dat.c_str(), gp.c_str(), img.c_str());
      }
      rsi_plot_batch_free(b);
    }
    std::cout << "job " << k++ << " " << rc << "\n";
  }
  return 0;
}
