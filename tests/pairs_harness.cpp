// pairs_harness.cpp -- the host annotation (bam_host.cpp: bam_pair_sample, bam_annotate_calls) and bam_pairs_core.h's serial forms
// side by side, as a stand-alone program built with -fsanitize=address,undefined (tests/test_pairs_host.py).  It reads a job file,
// one job per line, and prints one block per job:
//   X bam tid                      the pair table bam_pairs_core.h extracts from the file's records of tid: "x pos rend mpos isize info"
//   S bam tid tid_len table n      the insert-size sample: "s host isize sd" (bam = "-": skipped) and "s core count abs sq S isize sd"
//   A bam tid table n mean sd k start end type ...   per call "a host rp q0" (q0 as %a) and "a core rp q0_all q0_q0"
// table: a file of five int32 arrays of n entries each (pos, rend, mpos, isize, info).
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../rsicnv_amd/csrc/bam_host.h"
#include "../rsicnv_amd/csrc/bam_pairs_core.h"

namespace {

struct Bytes {
  const std::vector<uint8_t>& v;
  uint8_t at(uint64_t i) const { return v.at((size_t)i); }   // a read outside the stream throws
};

struct Table {
  std::vector<int32_t> a[5];
  bool read(const std::string& path, size_t n) {
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) return false;
    bool ok = true;
    for (auto& v : a) { v.resize(n); if (n && fread(v.data(), 4, n, f) != n) ok = false; }
    fclose(f);
    return ok;
  }
  const uint32_t* info() const { return reinterpret_cast<const uint32_t*>(a[4].data()); }
};

int fail(const std::string& m) { std::cout << "error " << m << "\n"; return 1; }

// the records of the file from the first one on, inflated into one stream
bool inflate_all(rsih::BamFile& bam, std::vector<uint8_t>& out, std::string& err) {
  std::vector<std::pair<std::string, int64_t>> refs;
  uint64_t first = 0;
  if (!bam.read_header(refs, first, err)) return false;
  uint64_t coff = first >> 16;
  size_t skip = (size_t)(first & 0xffff);
  for (;;) {
    rsih::BgzfBlock b;
    std::string e2;
    if (!bam.block_at(coff, b, e2)) { err = e2; return e2.empty(); }
    std::vector<uint8_t> buf(b.isize);
    if (!bam.inflate(b, buf.data(), err)) return false;
    out.insert(out.end(), buf.begin() + (long)std::min(skip, buf.size()), buf.end());
    skip = 0;
    coff += b.csize;
  }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) return fail("usage: pairs_harness JOBFILE");
  std::ifstream jobs(argv[1]);
  std::string line;
  while (std::getline(jobs, line)) {
    std::istringstream in(line);
    std::string kind, bam_path;
    int tid = 0;
    in >> kind >> bam_path >> tid;
    std::cout << "job " << kind << "\n";
    rsih::BamFile bam;
    std::string err;
    const bool have_bam = bam_path != "-";
    if (have_bam && !bam.open(bam_path, err)) return fail(err);
    const std::string bai = bam_path + ".bai";
    if (kind == "X") {
      std::vector<uint8_t> stream;
      if (!inflate_all(bam, stream, err)) return fail(err);
      const Bytes d{stream};
      uint64_t p = 0;
      while (p + 4 <= stream.size()) {
        const uint32_t bs = rsipairs::rd32(d, p);
        if (bs < 32 || p + 4 + bs > stream.size()) return fail("record chain");
        if ((int32_t)rsipairs::rd32(d, p + 4) == tid) {
          bool overrun = false;
          const rsipairs::Entry e = rsipairs::extract(d, p, tid, overrun);
          std::cout << "x " << e.pos << " " << e.rend << " " << e.mpos << " " << e.isize << " " << e.info << " " << (overrun ? 1 : 0) << "\n";
        }
        p += 4 + (uint64_t)bs;
      }
    } else if (kind == "S") {
      long long tid_len = 0;
      std::string table_path;
      size_t n = 0;
      in >> tid_len >> table_path >> n;
      Table t;
      if (!t.read(table_path, n)) return fail("table " + table_path);
      if (have_bam) {
        rsih::PairSample ps;
        if (!rsih::bam_pair_sample(bam, bai, tid, tid_len, 10000000, 349250621, ps, err)) return fail(err);
        std::cout << "s host " << ps.isize << " " << ps.isize_sd << "\n";
      }
      int64_t out[4];
      rsipairs::sample_serial((int64_t)n, t.a[0].data(), t.a[1].data(), t.a[3].data(), t.info(), tid_len, out);
      int isize = -1, sd = -1;
      {   // bam_pair_sample's own expressions
        double m = (double)out[1];
        const double m2 = (double)out[2], c = (double)out[0];
        if (c > 2) { m /= c; const double s = sqrt((m2 - c * m * m) / c); isize = (int)m; sd = (int)s; }
      }
      std::cout << "s core " << out[0] << " " << out[1] << " " << out[2] << " " << out[3] << " " << isize << " " << sd << "\n";
    } else if (kind == "A") {
      std::string table_path;
      size_t n = 0;
      int mean = 0, sd = 0, k = 0;
      in >> table_path >> n >> mean >> sd >> k;
      Table t;
      if (!t.read(table_path, n)) return fail("table " + table_path);
      std::vector<rsih::CallSpan> spans((size_t)k);
      for (auto& c : spans) { in >> c.start >> c.end >> c.type; c.rp = -1; c.q0 = -1.0; }
      if (!in) return fail("job line");
      if (have_bam) {
        std::vector<rsih::CallSpan> host = spans;
        rsih::PairSample ps;
        ps.isize = mean; ps.isize_sd = sd;
        if (!rsih::bam_annotate_calls(bam, bai, tid, ps, host, err)) return fail(err);
        for (const auto& c : host) printf("a host %d %a\n", c.rp, c.q0);
        fflush(stdout);
      }
      rsipairs::Windows win;
      for (const auto& c : spans) {
        const rsipairs::Call call = win.next(c.start, c.end, c.type);
        uint32_t out[3];
        rsipairs::annotate_serial((int64_t)n, t.a[0].data(), t.a[1].data(), t.a[2].data(), t.info(), call, mean, sd, out);
        std::cout << "a core " << out[2] << " " << out[0] << " " << out[1] << "\n";
      }
    } else {
      return fail("unknown job " + kind);
    }
  }
  return 0;
}
