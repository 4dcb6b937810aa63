/* track_probe_fprintf.c -- the loop plain -s saves a chromosome's depth with (cli.cpp, report_chromosome: one fprintf per base,
 * "pos<TAB>depth"), on an int32 array read from a file: the baseline tools/track_probe.py times the track writer against.
 *   track_probe_fprintf DEPTH.i32 OUT   -> prints the seconds of the loop (fopen to fclose) and the bytes written */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <time.h>

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: track_probe_fprintf DEPTH.i32 OUT\n"); return 2; }
  FILE* in = fopen(argv[1], "rb");
  if (!in) { perror(argv[1]); return 1; }
  fseek(in, 0, SEEK_END);
  const long long n = ftell(in) / 4;
  fseek(in, 0, SEEK_SET);
  int32_t* rd = (int32_t*)malloc((size_t)n * 4);
  if (!rd || fread(rd, 4, (size_t)n, in) != (size_t)n) { fprintf(stderr, "cannot read %s\n", argv[1]); return 1; }
  fclose(in);
  struct timespec t0, t1;
  clock_gettime(CLOCK_MONOTONIC, &t0);
  FILE* f = fopen(argv[2], "w");
  if (!f) { perror(argv[2]); return 1; }
  for (long long i = 0; i < n; ++i) fprintf(f, "%lld\t%d\n", i + 1, rd[i]);
  const long long bytes = ftell(f);
  fclose(f);
  clock_gettime(CLOCK_MONOTONIC, &t1);
  printf("%.6f %lld\n", (double)(t1.tv_sec - t0.tv_sec) + 1e-9 * (double)(t1.tv_nsec - t0.tv_nsec), bytes);
  free(rd);
  return 0;
}
