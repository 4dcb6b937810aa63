// Host driver of rsicnv_amd/csrc/text_rules.h (the depth-text readers' integer extraction, built here as plain C++ under
// ASan + UBSan) against the reference's own means, std::istringstream with zero-initialised variables.  Per line:
//   ints  `iss >> v0 >> v1 >> ... >> v8` into int: pos, d (the per-base rule) and a cohort chain of 8 columns
//   bed   `iss >> start >> end >> d` into long long, long long, int
//   gen SEED N LINES      N random lines (signs, blanks, digit runs of 1-25 characters, boundary values, junk) into LINES
//   check LINES VALUES    every line of LINES ('\n'-separated) both ways; VALUES gets istringstream's 12 values per line,
//                         tab-separated; prints the counts, exit 1 on any difference
#include "../../rsicnv_amd/csrc/text_rules.h"
#include <stdio.h>
#include <stdlib.h>
#include <fstream>
#include <random>
#include <sstream>
#include <string>
#include <vector>

namespace {

constexpr int kChain = 9;

void by_stream(const std::string& line, long long* out) {
  {
    std::istringstream iss(line);
    int v[kChain] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    iss >> v[0] >> v[1] >> v[2] >> v[3] >> v[4] >> v[5] >> v[6] >> v[7] >> v[8];
    for (int i = 0; i < kChain; ++i) out[i] = v[i];
  }
  std::istringstream iss(line);
  long long a = 0, b = 0;
  int d = 0;
  iss >> a >> b >> d;
  out[kChain] = a; out[kChain + 1] = b; out[kChain + 2] = d;
}

void by_rules(const std::string& line, long long* out) {
  const char* t = line.data();
  const long long e = (long long)line.size();
  long long q = 0;
  bool ok = true;
  for (int i = 0; i < kChain; ++i) { long long v = 0; if (ok) ok = rsitxt::extract_i32(t, q, e, v); out[i] = v; }
  q = 0; ok = true;
  long long v[3] = {0, 0, 0};
  for (int i = 0; i < 3; ++i) if (ok) ok = i < 2 ? rsitxt::extract_i64(t, q, e, v[i]) : rsitxt::extract_i32(t, q, e, v[i]);
  out[kChain] = v[0]; out[kChain + 1] = v[1]; out[kChain + 2] = v[2];
}

std::string random_line(std::mt19937_64& g) {
  static const char* kBoundary[] = {"2147483647", "2147483648", "2147483649", "4294967296", "9223372036854775807",
                                    "9223372036854775808", "9223372036854775809", "18446744073709551615", "18446744073709551616",
                                    "0", "00"};
  static const char* kJunk[] = {"abc", ".", ".5", "e3", "#", "" /* a NUL byte */, "x", "\xff", "+", "-", "0x1f", ","};
  static const char kBlank[] = {' ', '\t', '\r', '\v', '\f'};
  auto u = [&](unsigned m) { return (unsigned)(g() % m); };
  std::string s;
  // half the lines are mostly well formed (short digit runs, few signs, rare junk), so that long chains succeed
  const bool tame = u(2) == 0;
  const unsigned pieces = u(11);
  for (unsigned k = 0; k < pieces; ++k) {
    const unsigned nb = u(8) < 5 ? 1 : u(4);
    for (unsigned i = 0; i < nb; ++i) s += kBlank[u(8) < 5 ? 0 : u(5)];
    const unsigned sg = u(tame ? 60 : 20);
    if (sg < 5) s += '-'; else if (sg < 7) s += '+'; else if (sg == 7) s += "+-"; else if (sg == 8) s += "--";
    const unsigned kind = u(tame ? 50 : 10);
    if (kind < 2) {
      s += kBoundary[u(sizeof(kBoundary) / sizeof(kBoundary[0]))];
    } else if (kind < 9 || tame) {
      const unsigned len = 1 + u(tame ? 9 : 25);
      const bool zeros = u(6) == 0;
      for (unsigned i = 0; i < len; ++i) s += zeros && i < len / 2 ? '0' : (char)('0' + u(10));
    }
    if (u(tame ? 60 : 8) == 0) { const char* j = kJunk[u(sizeof(kJunk) / sizeof(kJunk[0]))]; s += j[0] ? std::string(j) : std::string("\0", 1); }
  }
  if (u(6) == 0) for (unsigned i = 0, nb = 1 + u(3); i < nb; ++i) s += kBlank[u(5)];
  return s;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 5 && std::string(argv[1]) == "gen") {
    std::mt19937_64 g(strtoull(argv[2], nullptr, 10));
    const long n = strtol(argv[3], nullptr, 10);
    std::ofstream f(argv[4], std::ios::binary);
    for (long i = 0; i < n; ++i) f << random_line(g) << '\n';
    printf("gen ok: %ld lines\n", n);
    return 0;
  }
  if (argc == 4 && std::string(argv[1]) == "check") {
    std::ifstream f(argv[2], std::ios::binary);
    std::ofstream o(argv[3], std::ios::binary);
    std::string line;
    long lines = 0, bad = 0, clamped = 0;
    long long a[kChain + 3], b[kChain + 3];
    while (std::getline(f, line)) {
      by_stream(line, a);
      by_rules(line, b);
      ++lines;
      bool same = true;
      for (int i = 0; i < kChain + 3; ++i) {
        same = same && a[i] == b[i];
        if (a[i] == 2147483647 || a[i] == -2147483647 - 1 || a[i] == 9223372036854775807ll) ++clamped;
        o << a[i] << (i + 1 < kChain + 3 ? '\t' : '\n');
      }
      if (!same && bad++ < 20) {
        printf("differs on line %ld:", lines);
        for (int i = 0; i < kChain + 3; ++i) printf(" %lld/%lld", a[i], b[i]);
        printf("\n");
      }
    }
    printf("check %s: %ld lines, %ld differ, %ld bound values\n", bad ? "FAILED" : "ok", lines, bad, clamped);
    return bad ? 1 : 0;
  }
  fprintf(stderr, "usage: %s gen SEED N LINES | check LINES VALUES\n", argv[0]);
  return 2;
}
