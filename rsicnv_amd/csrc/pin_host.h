// pin_host.h -- the host side of `rsicnv stat` and `rsicnv pin`, plain C++ for cli.cpp, ingest_bam.hip and
// tests/pin_harness.cpp: the CNV list as read_cnvlist reads it (loaddata.cpp:542 and :606), cnv_stat's windows carried through
// the whole file, the sample's means and deviations by bam_rd_pr_stats' own loops, and the two output rows.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "bam_pairs_core.h"

namespace rsipinh {

enum { kDel = 0, kDup = 1, kUnknown = 2 };   // TYPE_DEL, TYPE_DUP, TYPE_UNKNOWN

// ci_find(field, word) != npos
inline bool has_word(const std::string& field, const char* word) {
  std::string f(field);
  for (char& c : f) c = (char)tolower((unsigned char)c);
  return f.find(word) != std::string::npos;
}
// the later match wins, as the reference's five tests in a row have it
inline int cnv_type_of(const std::string& field) {
  int type = kUnknown;
  if (has_word(field, "del")) type = kDel;
  if (has_word(field, "loss")) type = kDel;
  if (has_word(field, "dup")) type = kDup;
  if (has_word(field, "gain")) type = kDup;
  if (has_word(field, "add")) type = kDup;
  return type;
}

struct CnvLine {
  std::string text;                 // the line as it stands
  std::vector<std::string> cell;    // its fields, split on white space
  int tid = -1, start = 0, end = 0, type = kUnknown;
};
// One line of the list: false for a line the reader passes over (shorter than 5 characters, a comment, fewer than 4 fields --
// *few says which).  names: the BAM header's, matched exactly.
inline bool parse_cnv_line(const std::string& text, const std::vector<std::string>& names, CnvLine& out, bool* few = nullptr) {
  if (few) *few = false;
  if (text.length() < 5 || text[0] == '#') return false;
  out = CnvLine();
  out.text = text;
  std::istringstream iss(text);
  std::string w;
  while (iss >> w) if (!w.empty()) out.cell.push_back(w);
  if (out.cell.size() < 4) { if (few) *few = true; return false; }
  for (size_t k = 0; k < names.size() && out.tid < 0; ++k) if (names[k] == out.cell[0]) out.tid = (int)k;
  out.start = atoi(out.cell[1].c_str());
  out.end = atoi(out.cell[2].c_str());
  out.type = cnv_type_of(out.cell[3]);
  return true;
}
inline bool read_cnvlist(const std::string& path, const std::vector<std::string>& names, std::vector<CnvLine>& lines, std::ostream& err) {
  std::ifstream in(path.c_str());
  if (!in) { err << "File " << path << " not exist" << std::endl; return false; }
  lines.clear();
  std::string text;
  while (std::getline(in, text)) {
    CnvLine l;
    bool few = false;
    if (parse_cnv_line(text, names, l, &few)) lines.push_back(l);
    else if (few) err << "skipping lines with less than 4 fields\nexpecting RNAME cnv_begin_pos cnv_end_pos cnv_type in each line" << std::endl;
  }
  if (lines.empty()) { err << "I can't find any CNV from " << path << std::endl; return false; }
  return true;
}

// cnv_stat's windows: DIS is carried from line to line through the whole file, chromosome changes included.
inline std::vector<rsipairs::Call> stat_windows(const std::vector<CnvLine>& lines) {
  std::vector<rsipairs::Call> out;
  rsipairs::Windows win;
  for (const CnvLine& l : lines) out.push_back(win.next(l.start, l.end, l.type));
  return out;
}

// ---- the sample's figures (bam_rd_pr_stats, pairrd.cpp:213-234) ----
inline int l_qseq_of(int64_t lq_sum, int64_t count) {
  const double l_qseq_sum = (double)lq_sum;
  return (int)(l_qseq_sum / (double)(size_t)count + 0.5);
}
struct SampleStats { int l_qseq = 0; double rd = 0, rd_sd = 0, drd = 0, drd_sd = 0; };
// rd and drd: the last stretch's arrays, index 0 at pos_start; len = pos_end - pos_start.  Serial sums of doubles, as there.
inline SampleStats sample_stats(const int32_t* rd, const int32_t* drd, int len, int l_qseq) {
  SampleStats s;
  s.l_qseq = l_qseq;
  double rdmean = 0.0, drdmean = 0.0;
  for (int k = l_qseq / 4; k < len - l_qseq / 4; ++k) { rdmean += rd[k]; drdmean += drd[k]; }
  rdmean /= (len - l_qseq / 2);
  drdmean /= (len - l_qseq / 2);
  double drdsd = 0.0, rdsd = 0.0;
  for (int k = l_qseq / 4; k < len - l_qseq / 4; ++k) {
    drdsd += (drdmean - drd[k]) * (drdmean - drd[k]);
    rdsd += (rdmean - rd[k]) * (rdmean - rd[k]);
  }
  s.rd = rdmean; s.drd = drdmean;
  s.drd_sd = sqrt(drdsd / (len - l_qseq / 2));
  s.rd_sd = sqrt(rdsd / (len - l_qseq / 2));
  return s;
}
// the six lines optimize_resolution writes behind a sample
inline std::string sample_log(const std::string& chrom, const SampleStats& s) {
  std::ostringstream o;
  o << "sample chr : " << chrom << "\nread length: " << s.l_qseq << "\nrd mean    : " << s.rd << "\nrd sd      : " << s.rd_sd << "\ndrd mean   : " << s.drd
    << "\ndrd sd     : " << s.drd_sd << "\n";
  return o.str();
}

// ---- the rows ----
inline std::string stat_row(const CnvLine& l, int rp, double q0) {
  char buf[64];
  snprintf(buf, sizeof buf, "\tRP=%d;Q0=%g", rp, q0);        // an ostream's default: %g
  return l.text + buf;
}
inline std::string pin_row(const CnvLine& l, int start, int end, int sc1, int sc2) {
  std::string s = l.cell[0] + "\t" + std::to_string(start) + "\t" + std::to_string(end);
  for (size_t k = 3; k < l.cell.size(); ++k) s += "\t" + l.cell[k];
  return s + "\tSC=" + std::to_string(sc1) + ";" + std::to_string(sc2);
}

}  // namespace rsipinh
