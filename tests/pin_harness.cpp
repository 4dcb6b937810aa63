// pin_harness.cpp -- bam_pin_core.h's serial forms and pin_host.h's host functions as a stand-alone program built with
// -fsanitize=address,undefined (tests/test_pin_host.py).  It reads a job file, one job per line, and prints one block per job:
//   L cnvfile name ...                 the CNV list against the header names: per accepted line "l tid start end type ncell p1e p2e"
//                                      (cnv_stat's window, DIS carried through the file), then "r <stat row>" and "q <pin row>" with fixed values
//   P table n cigs npool tid_len m k start end type ...
//                                      the sample: "s count pos_start pos_end flags l_qseq rd rd_sd drd drd_sd" (doubles as %a), then per
//                                      call "p start end sc1 sc2"
// table: five int32 arrays of n entries (pos, rend, mpos, isize, info); cigs: lq[n], coff[n], pool[npool].
#include <stdio.h>
#include <stdlib.h>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../rsicnv_amd/csrc/bam_pin_core.h"
#include "../rsicnv_amd/csrc/pin_host.h"

namespace {

int fail(const std::string& m) { std::cout << "error " << m << "\n"; return 1; }

bool read_words(FILE* f, std::vector<int32_t>& v, size_t n) {
  v.resize(n);
  return n == 0 || fread(v.data(), 4, n, f) == n;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) return fail("usage: pin_harness JOBFILE");
  std::ifstream jobs(argv[1]);
  std::string line;
  while (std::getline(jobs, line)) {
    std::istringstream in(line);
    std::string kind;
    in >> kind;
    std::cout << "job " << kind << "\n";
    if (kind == "L") {
      std::string path, nm;
      in >> path;
      std::vector<std::string> names;
      while (in >> nm) names.push_back(nm);
      std::vector<rsipinh::CnvLine> lines;
      std::ostringstream err;
      if (!rsipinh::read_cnvlist(path, names, lines, err)) { std::cout << "none\n"; continue; }
      const std::vector<rsipairs::Call> win = rsipinh::stat_windows(lines);
      for (size_t i = 0; i < lines.size(); ++i) {
        const rsipinh::CnvLine& l = lines[i];
        std::cout << "l " << l.tid << " " << l.start << " " << l.end << " " << l.type << " " << l.cell.size() << " " << win[i].p1e << " " << win[i].p2e << "\n";
        std::cout << "r " << rsipinh::stat_row(l, 3, 1.0 / 3) << "\n" << "q " << rsipinh::pin_row(l, l.start + 1, l.end - 1, 2, 0) << "\n";
      }
    } else if (kind == "P") {
      std::string table_path, cig_path;
      size_t n = 0, npool = 0;
      long long tid_len = 0;
      int m = 0, k = 0;
      in >> table_path >> n >> cig_path >> npool >> tid_len >> m >> k;
      std::vector<int32_t> a[5], lq, coff, pool;
      FILE* f = fopen(table_path.c_str(), "rb");
      if (!f) return fail("table " + table_path);
      bool ok = true;
      for (auto& v : a) ok = read_words(f, v, n) && ok;
      fclose(f);
      f = fopen(cig_path.c_str(), "rb");
      if (!f) return fail("cigars " + cig_path);
      ok = read_words(f, lq, n) && read_words(f, coff, n) && read_words(f, pool, npool) && ok;
      fclose(f);
      if (!ok) return fail("short file");
      const uint32_t* info = reinterpret_cast<const uint32_t*>(a[4].data());
      const rsipin::Tab t{lq.data(), reinterpret_cast<const uint32_t*>(coff.data()), reinterpret_cast<const uint32_t*>(pool.data())};
      std::vector<int32_t> rd((size_t)rsipin::kRdcSize);
      const rsipin::SampleState st = rsipin::sample_serial((int64_t)n, a[0].data(), a[1].data(), info, t, tid_len, rd.data());
      rsipinh::SampleStats s;
      if (st.count > 0 && !(st.flags & rsipin::kGrows)) {
        const int l_qseq = rsipinh::l_qseq_of(st.lq_sum, st.count);
        const int len = st.pos_end - st.pos_start, q = l_qseq / 4;
        std::vector<int32_t> drd((size_t)(len > 0 ? len : 1), 0);
        if (l_qseq >= 1) {
          for (int i = q; i < len - q; ++i) drd[(size_t)i] = rsipin::sample_drd(rd.data(), i, l_qseq);
          s = rsipinh::sample_stats(rd.data(), drd.data(), len, l_qseq);
        }
        s.l_qseq = l_qseq;
      }
      printf("s %d %d %d %d %d %a %a %a %a\n", st.count, st.pos_start, st.pos_end, st.flags, s.l_qseq, s.rd, s.rd_sd, s.drd, s.drd_sd);
      fflush(stdout);
      const int r_len = rsipin::r_len_of(m, s.l_qseq);
      std::vector<int32_t> w((size_t)3 * (2 * (size_t)r_len + 1));
      for (int c = 0; c < k; ++c) {
        int32_t start = 0, end = 0, type = 0;
        in >> start >> end >> type;
        if (!in) return fail("job line");
        int32_t ns = start, ne = end, sc[2] = {0, 0};
        if (rsipin::call_pinned(start, end, type)) {
          rsipin::Bp b[2];
          rsipin::bps_of(start, end, type, b);
          int32_t o[2][2];
          for (int e = 0; e < 2; ++e) rsipin::window_serial((int64_t)n, a[0].data(), a[1].data(), info, t, tid_len, b[e], r_len, s.l_qseq, s.drd_sd, w.data(), o[e]);
          sc[0] = o[0][1]; sc[1] = o[1][1];
          ns = rsipin::moved(start, r_len, o[0][0], o[0][1]);
          ne = rsipin::moved(end, r_len, o[1][0], o[1][1]);
        }
        std::cout << "p " << ns << " " << ne << " " << sc[0] << " " << sc[1] << "\n";
      }
    } else {
      return fail("unknown job " + kind);
    }
  }
  return 0;
}
