/* bin_track_probe_fprintf.c -- what the device's bin-track writer replaces: a host loop over the fetched arrays, one fprintf per
 * piece of a bin ("NAME<TAB>start<TAB>end<TAB>ratio", the ratio as q / 1000 "." q % 1000), on the files tools/bin_track_probe.py
 * writes.  The loop walks the kept intervals between the removed regions, as a host program would.
 *   bin_track_probe_fprintf BINMED.i32 PAIRS.i32 M N MEDIAN2 OUT   -> prints the seconds of the loop (fopen to fclose), the
 *   lines and the bytes written */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <time.h>

static int32_t* slurp(const char* path, long long* count) {
  FILE* in = fopen(path, "rb");
  if (!in) { perror(path); exit(1); }
  fseek(in, 0, SEEK_END);
  *count = ftell(in) / 4;
  fseek(in, 0, SEEK_SET);
  int32_t* p = (int32_t*)malloc((size_t)(*count ? *count : 1) * 4);
  if (!p || fread(p, 4, (size_t)*count, in) != (size_t)*count) { fprintf(stderr, "cannot read %s\n", path); exit(1); }
  fclose(in);
  return p;
}

int main(int argc, char** argv) {
  if (argc != 7) { fprintf(stderr, "usage: bin_track_probe_fprintf BINMED.i32 PAIRS.i32 M N MEDIAN2 OUT\n"); return 2; }
  long long nb = 0, npair_words = 0;
  const int32_t* v = slurp(argv[1], &nb);
  const int32_t* pairs = slurp(argv[2], &npair_words);
  const long long nreg = npair_words / 2, m = atoll(argv[3]), n = atoll(argv[4]), m2 = atoll(argv[5]);
  if (m < 1 || m2 < 1) { fprintf(stderr, "bad M or MEDIAN2\n"); return 2; }
  struct timespec t0, t1;
  clock_gettime(CLOCK_MONOTONIC, &t0);
  FILE* f = fopen(argv[6], "w");
  if (!f) { perror(argv[6]); return 1; }
  long long lines = 0, k = 0, at = 0;                     /* next region, next kept reference position */
  while (k < nreg && pairs[2 * k] <= at) { at = (long long)pairs[2 * k + 1] + 1; ++k; }
  for (long long b = 0; b < nb; ++b) {
    const long long q = (4000 * (long long)v[b] + m2) / (2 * m2);
    long long need = m;
    while (need > 0) {
      const long long stop = k < nreg ? pairs[2 * k] : n;   /* the kept interval [at, stop) */
      const long long take = stop - at < need ? stop - at : need;
      fprintf(f, "chrProbe\t%lld\t%lld\t%lld.%03lld\n", at, at + take, q / 1000, q % 1000);
      ++lines;
      need -= take; at += take;
      if (at == stop && k < nreg) { at = (long long)pairs[2 * k + 1] + 1; ++k; }
    }
  }
  const long long bytes = ftell(f);
  fclose(f);
  clock_gettime(CLOCK_MONOTONIC, &t1);
  printf("%.6f %lld %lld\n", (double)(t1.tv_sec - t0.tv_sec) + 1e-9 * (double)(t1.tv_nsec - t0.tv_nsec), lines, bytes);
  return 0;
}
