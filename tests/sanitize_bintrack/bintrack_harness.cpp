// bintrack_harness.cpp -- the host side of the per-bin track (rsicnv_amd/csrc/track_host.h: bin_plan, bin_table, twice_median)
// alone, under ASan + UBSan:
//   bintrack_harness      every check below; prints "bin track host ok"
#include <stdio.h>
#include <stdlib.h>
#include <string>
#include <vector>

#include "../../rsicnv_amd/csrc/track_host.h"

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

static void plans() {
  using namespace rsitrack;
  BinPlan p;
  const long long ns[] = {0, 1, 9, 10, 999999999, 1000000000, 2147483647, 250000000ll, 1ll << 40, 999999999999999999ll,
                          1000000000000000000ll, INT64_MAX};
  const long long nbs[] = {0, 1, 2, 255, 256, 257, 5000, kSliceBases - 4096, kSliceBases - 4095, kSliceBases, kSliceBases + 1, 30000000ll, 1ll << 40};
  const long long forced[] = {0, 1, 2, 255, 256, 257, 1000, kSliceBases, kSliceBases * 4, INT64_MAX};
  const int nregs[] = {0, 1, 127, 128, 129, 4095, 4096};
  for (int name_len : {1, 5, 255})
    for (int which : {0, 1})
      for (int nreg : nregs)
        for (long long n : ns)
          for (long long nb : nbs)
            for (long long s : forced) {
              CHECK(bin_plan(name_len, n, nb, nreg, which, s, p));
              // the longest line this call can write: name, three tabs and a newline, two coordinates up to n, a value
              char a[32];
              const int coord = snprintf(a, sizeof(a), "%lld", n);
              CHECK(p.max_line == name_len + 4 + 2 * coord + (which ? 18 : 11));
              CHECK(p.slice >= 1);                                       // a slice is at least one bin
              CHECK(p.slice <= kSliceBases && (nb == 0 || p.slice <= nb));
              if (s > 0) CHECK(p.slice <= s);
              CHECK(p.max_pieces == p.slice + nreg);                     // every break cuts at most one bin of the slice
              CHECK(p.max_pieces <= kSliceBases + 1);                    // the pieces fit the depth track's starts workspace
              CHECK(p.text_cap == p.max_pieces * p.max_line && p.text_cap <= kTextBytes);   // every slice's worst-case text fits
              if (nb > 0) {   // the slices tile [0, nb): the last one ends at nb
                const long long count = (nb + p.slice - 1) / p.slice;
                const long long last_begin = (count - 1) * p.slice;
                CHECK(last_begin < nb && std::min<long long>(nb, last_begin + p.slice) == nb);
              }
            }
  // the largest ratio: q = (4000 INT32_MAX + 1) / 2 thousandths, ten digits in front of the point -- inside kRatioBytes
  {
    char a[64];
    const long long q = (4000ll * 2147483647ll + 1) / 2;
    CHECK(snprintf(a, sizeof(a), "%lld.%03lld", q / 1000, q % 1000) <= kRatioBytes);
    CHECK(snprintf(a, sizeof(a), "%d", INT32_MIN) == kMedianBytes);
  }
  CHECK(!bin_plan(4, -1, 1, 0, 0, 0, p) && !bin_plan(4, 10, -1, 0, 0, 0, p));
  CHECK(!bin_plan(4, 10, 1, -1, 0, 0, p) && !bin_plan(4, 10, 1, 4097, 0, 0, p));
  CHECK(!bin_plan(4, 10, 1, 0, 2, 0, p) && !bin_plan(4, 10, 1, 0, -1, 0, p));
  // 19-digit coordinates are handled, as rsitrack::plan handles them: the line is that much longer
  CHECK(bin_plan(255, INT64_MAX, 1ll << 40, 4096, 1, 0, p) && p.max_line == 255 + 4 + 2 * 19 + 18 && p.slice >= 1);
}

static void tables() {
  using rsitrack::bin_table;
  std::vector<int64_t> cb, cum;
  int64_t nc = -1;
  CHECK(bin_table(nullptr, 0, 0, cb, cum, nc) && cb.empty() && cum.size() == 1 && cum[0] == 0 && nc == 0);
  CHECK(bin_table(nullptr, 0, 10, cb, cum, nc) && nc == 10);
  {
    const int32_t p[] = {0, 3, 5, 5, 8, 9};   // from 0, a single base, up to n - 1
    CHECK(bin_table(p, 3, 10, cb, cum, nc));
    CHECK(cb.size() == 3 && cb[0] == 0 && cb[1] == 1 && cb[2] == 3);
    CHECK(cum.size() == 4 && cum[0] == 0 && cum[1] == 4 && cum[2] == 5 && cum[3] == 7 && nc == 3);
    CHECK(!bin_table(p, 3, 9, cb, cum, nc));               // the last region ends outside [0, n)
  }
  { const int32_t p[] = {2, 3, 4, 6}; CHECK(!bin_table(p, 2, 10, cb, cum, nc)); }    // touching
  { const int32_t p[] = {2, 3, 3, 6}; CHECK(!bin_table(p, 2, 10, cb, cum, nc)); }    // overlapping
  { const int32_t p[] = {5, 6, 1, 2}; CHECK(!bin_table(p, 2, 10, cb, cum, nc)); }    // unsorted
  { const int32_t p[] = {4, 3}; CHECK(!bin_table(p, 1, 10, cb, cum, nc)); }          // empty
  { const int32_t p[] = {-1, 3}; CHECK(!bin_table(p, 1, 10, cb, cum, nc)); }
  { const int32_t p[] = {0, 1999999999}; CHECK(bin_table(p, 1, 2000000300ll, cb, cum, nc) && cb[0] == 0 && cum[1] == 2000000000ll && nc == 300); }
  CHECK(!bin_table(nullptr, 1, 10, cb, cum, nc) && !bin_table(nullptr, -1, 10, cb, cum, nc));
  {   // 4096 regions, 130 bases apart, 10 wide
    std::vector<int32_t> p;
    for (int k = 0; k < 4096; ++k) { p.push_back(100 + 130 * k); p.push_back(109 + 130 * k); }
    CHECK(bin_table(p.data(), 4096, 600000, cb, cum, nc) && nc == 600000 - 40960 && cb[4095] == 100 + 130 * 4095 - 40950);
  }
}

static void medians() {
  using rsitrack::twice_median;
  int64_t m2 = -1;
  CHECK(twice_median(0.0, m2) && m2 == 0);
  CHECK(twice_median(30.0, m2) && m2 == 60);
  CHECK(twice_median(30.5, m2) && m2 == 61);
  CHECK(twice_median(2147483647.0, m2) && m2 == 4294967294ll);
  CHECK(!twice_median(30.25, m2) && !twice_median(-1.0, m2) && !twice_median(1e300, m2));
  CHECK(!twice_median(__builtin_nan(""), m2) && !twice_median(__builtin_inf(), m2));
}

int main() {
  plans();
  tables();
  medians();
  printf("bin track host ok\n");
  return 0;
}
