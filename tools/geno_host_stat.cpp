// geno_host_stat.cpp -- what `rsicnv geno` replaces, for tools/geno_probe.py: the same statistic on the host, by hostmath.h's
// grid_quantiles<int> (the restatement of the reference's partition_stat_tp with dy = 1), over the fetched compacted depth.
// The probe compiles this file into a shared object and loads it, so that both roads are timed in one process.
#include <stdint.h>

#include <vector>

#include "../rsicnv_amd/csrc/hostmath.h"

// ranges: six int64 per line (lo, hi, flo0, fhi0, flo1, fhi1), half-open, in rd[]; out: six doubles per line, the body's lower
// quartile, median and upper quartile, then the flank's (zeros for an empty range)
extern "C" void geno_host_stat(const int32_t* rd, int64_t nlines, const int64_t* ranges, double* out) {
  std::vector<int> flank;
  for (int64_t i = 0; i < nlines; ++i) {
    const int64_t* r = ranges + 6 * i;
    double* o = out + 6 * i;
    for (int k = 0; k < 6; ++k) o[k] = 0.0;
    if (r[1] > r[0]) {
      const rsih::Quantiles q = rsih::grid_quantiles<int>(rd + r[0], (size_t)(r[1] - r[0]));
      o[0] = q.lqt; o[1] = q.med; o[2] = q.uqt;
    }
    flank.assign(rd + r[2], rd + r[3]);
    flank.insert(flank.end(), rd + r[4], rd + r[5]);
    if (!flank.empty()) {
      const rsih::Quantiles q = rsih::grid_quantiles<int>(flank.data(), flank.size());
      o[3] = q.lqt; o[4] = q.med; o[5] = q.uqt;
    }
  }
}
