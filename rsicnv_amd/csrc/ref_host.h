// ref_host.h -- the host decisions of the reference reader as pure functions: the .fai line parse, where a base
// lies in the file, the text a base range needs, the bases a span of text holds whole, the .gzi parse and the members that cover
// a text range.  No file, no device: ref.hip's rsi_ref_* calls them, tests/test_ref_host.py checks them through the
// rsi_ref_debug_* exports on a machine without a GPU.
#pragma once
#include <stdint.h>
#include <string.h>
#include <sstream>
#include <string>
#include <utility>
#include <vector>

namespace rsiref {

constexpr int kMaxTerminator = 64;                 // linewidth - linebases: "\n" is 1, "\r\n" 2; more is no FASTA any tool writes
constexpr int64_t kMaxLength = (1ll << 31) - 4096; // as everywhere: a sequence's bases are counted in 32 bits

// One .fai line: NAME LENGTH OFFSET LINEBASES LINEWIDTH (samtools faidx; further columns, a FASTQ index's, are ignored)
struct Seq {
  std::string name;
  int64_t length = 0, offset = 0;
  int32_t linebases = 0, linewidth = 0;
  int terminator() const { return linewidth - linebases; }
};

// "" and s filled, or what is wrong with the line
inline std::string parse_fai_line(const std::string& line, Seq& s) {
  std::istringstream iss(line);
  long long len = 0, off = 0, lb = 0, lw = 0;
  if (!(iss >> s.name >> len >> off >> lb >> lw)) return "fewer than five columns (NAME LENGTH OFFSET LINEBASES LINEWIDTH)";
  if (len < 0 || len >= kMaxLength) return "LENGTH " + std::to_string(len) + " is outside [0, 2^31 - 4096)";
  if (off < 0) return "OFFSET " + std::to_string(off) + " is negative";
  if (lb <= 0 || lb > INT32_MAX) return "LINEBASES must be positive, is " + std::to_string(lb);
  if (lw < lb) return "LINEWIDTH " + std::to_string(lw) + " is below LINEBASES " + std::to_string(lb);
  if (lw - lb > kMaxTerminator) return "LINEWIDTH - LINEBASES is " + std::to_string(lw - lb) + ", more than " + std::to_string(kMaxTerminator) + " bytes of line terminator";
  s.length = len; s.offset = off; s.linebases = (int32_t)lb; s.linewidth = (int32_t)lw;
  return std::string();
}

// read_fasta's flen: the bytes of the sequence's lines, the terminator of every full line included (so the last line's too
// when LENGTH is a multiple of LINEBASES)
inline int64_t flen(const Seq& s) { return s.length + (s.length / s.linebases) * (int64_t)s.terminator(); }
// file offset of base k
inline int64_t base_pos(const Seq& s, int64_t k) { return s.offset + (k / s.linebases) * (int64_t)s.linewidth + k % s.linebases; }
// The text [a, b) that unfolding the bases [k0, k1), k0 < k1, reads: from base k0's byte to base k1 - 1's, and the terminator
// behind it when that base ends a full line (it is checked with its line)
inline void text_range(const Seq& s, int64_t k0, int64_t k1, int64_t& a, int64_t& b) {
  a = base_pos(s, k0);
  b = base_pos(s, k1 - 1) + 1 + (k1 % s.linebases == 0 ? s.terminator() : 0);
}
// The bases [k0, k1) a span [a, b) of the text holds whole, each line end with its terminator: text_range(k0, k1) lies inside
// [a, b), and no base in front of k0 begins at or behind a.  at_eof: b is the end of the file, where the last line of the last
// sequence may lack its terminator -- the sequence's last base is then taken without it.  k0 == k1: none.
inline void contained_bases(const Seq& s, int64_t a, int64_t b, bool at_eof, int64_t& k0, int64_t& k1) {
  const int64_t lb = s.linebases, lw = s.linewidth;
  const int64_t x = a - s.offset;
  if (x <= 0) k0 = 0;
  else k0 = x % lw < lb ? (x / lw) * lb + x % lw : (x / lw + 1) * lb;
  const int64_t y = b - s.offset;
  if (y <= 0) k1 = 0;
  else if (y % lw < lb) k1 = (y / lw) * lb + y % lw;                   // y / lw lines with their terminators, then bases of the next
  else k1 = (y / lw) * lb + lb - 1;                                     // a line whose terminator is cut: its last base waits
  if (at_eof && y > 0 && y % lw >= lb && (y / lw) * lb + lb == s.length) k1 = s.length;
  if (k0 > s.length) k0 = s.length;
  if (k1 > s.length) k1 = s.length;
  if (k1 < k0) k1 = k0;
}

// ---- .gzi (bgzip -i): little-endian uint64 count, then count (compressed offset, uncompressed offset) pairs, one for every
// member but the first.  The table gets the first member's (0, 0) in front.  "" or what is wrong: a size that is not 8 + 16
// count, compressed offsets that do not increase, uncompressed offsets that decrease (an empty member repeats one). ----
typedef std::vector<std::pair<int64_t, int64_t>> MemberTable;   // (compressed offset, text offset) of every member, in file order
inline std::string parse_gzi(const uint8_t* p, size_t n, MemberTable& t) {
  t.clear();
  auto u64 = [](const uint8_t* q) { uint64_t v = 0; for (int i = 7; i >= 0; --i) v = (v << 8) | q[i]; return v; };
  if (n < 8) return "shorter than its count field";
  const uint64_t count = u64(p);
  if (count > (n - 8) / 16 || 8 + 16 * count != n) return "holds " + std::to_string(n) + " bytes, not the " + std::to_string(count) + " entries it announces";
  t.reserve((size_t)count + 1);
  t.emplace_back(0, 0);
  for (uint64_t i = 0; i < count; ++i) {
    const uint64_t c = u64(p + 8 + 16 * i), u = u64(p + 16 + 16 * i);
    if (c > (uint64_t)INT64_MAX || u > (uint64_t)INT64_MAX || (int64_t)c <= t.back().first || (int64_t)u < t.back().second)
      return "entry " + std::to_string(i) + " (" + std::to_string(c) + ", " + std::to_string(u) + ") does not come behind the one before: offsets must increase";
    t.emplace_back((int64_t)c, (int64_t)u);
  }
  return std::string();
}

// The members [first, stop) of the table whose text covers [a, b), a < b: `first` is the last member that begins at or in front
// of a (so empty members in front of it are passed over), `stop` the first one that begins at or behind b (t.size(): the text
// runs into the table's last member, whose end the table does not know).  skew = a - (text offset of member `first`).
inline void member_cover(const MemberTable& t, int64_t a, int64_t b, size_t& first, size_t& stop, int64_t& skew) {
  size_t lo = 0, hi = t.size();   // last i with t[i].second <= a (t[0].second == 0 <= a)
  while (hi - lo > 1) { const size_t mid = lo + (hi - lo) / 2; if (t[mid].second <= a) lo = mid; else hi = mid; }
  first = lo;
  size_t l2 = first, h2 = t.size();   // first i > first with t[i].second >= b
  while (h2 - l2 > 1) { const size_t mid = l2 + (h2 - l2) / 2; if (t[mid].second >= b) h2 = mid; else l2 = mid; }
  stop = h2;
  skew = a - t[first].second;
}

// read_fasta's rule (readref.cpp:10-86): the first sequence named rname or "chr" + rname; -1: none
inline int find(const std::vector<Seq>& seqs, const std::string& rname) {
  for (size_t i = 0; i < seqs.size(); ++i) if (seqs[i].name == rname || seqs[i].name == "chr" + rname) return (int)i;
  return -1;
}

}  // namespace rsiref
