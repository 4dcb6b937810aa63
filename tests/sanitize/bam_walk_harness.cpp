// bam_walk_harness.cpp -- bam_walk_core.h as plain C++ under ASan + UBSan (tests/test_bam_walk_host.py): the guess, the walk
// and the stitch of the record finder, segment by segment, on files of inflated BAM bytes.
//   bam_walk_harness SEG NREF LEN_0 ... LEN_{NREF-1} [FILE START TID]...
// Per file two lines: "report listed seen end flags guessed rewalked passed" and "recs o_0 o_1 ...".  Every file sits in a
// heap block of exactly its size, so a read past the chunk is a sanitizer report.
#include "../../rsicnv_amd/csrc/bam_walk_core.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

int main(int argc, char** argv) {
  if (argc < 3) { fprintf(stderr, "usage: bam_walk_harness SEG NREF LEN... [FILE START TID]...\n"); return 2; }
  const uint32_t seg = (uint32_t)strtoul(argv[1], nullptr, 10);
  const int nref = atoi(argv[2]);
  if (seg < 64 || nref < 0 || argc < 3 + nref || (argc - 3 - nref) % 3 != 0) { fprintf(stderr, "bad arguments\n"); return 2; }
  std::vector<int32_t> reflen;
  for (int r = 0; r < nref; ++r) reflen.push_back((int32_t)atol(argv[3 + r]));
  const uint32_t cap = rsibam::list_cap(seg);
  for (int k = 3 + nref; k < argc; k += 3) {
    FILE* f = fopen(argv[k], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[k]); return 2; }
    fseek(f, 0, SEEK_END);
    const size_t len = (size_t)ftell(f);
    fseek(f, 0, SEEK_SET);
    uint8_t* data = static_cast<uint8_t*>(malloc(len ? len : 1));
    if (len && fread(data, 1, len, f) != len) { fprintf(stderr, "short read on %s\n", argv[k]); return 2; }
    fclose(f);
    const uint64_t start = strtoull(argv[k + 1], nullptr, 10);
    const int32_t tid = (int32_t)atol(argv[k + 2]);
    if (start > len) { fprintf(stderr, "start beyond %s\n", argv[k]); return 2; }
    const rsibam::Span d{data};
    const uint32_t nseg = (uint32_t)((len + seg - 1) / seg);
    std::vector<uint32_t> guess(nseg), acc(nseg), lists((size_t)nseg * cap);
    std::vector<rsibam::SegOut> out(nseg);
    for (uint32_t s = 0; s < nseg; ++s) {
      const uint64_t a = (uint64_t)s * seg, b = a + seg < len ? a + seg : len;
      guess[s] = rsibam::guess_segment(d, len, a, b, nref, reflen.data());
      out[s] = rsibam::SegOut{rsibam::kNone, 0, 0, 0};
      if (guess[s] != rsibam::kNone) out[s] = rsibam::walk_segment(d, len, guess[s], b, tid, lists.data() + (size_t)s * cap, cap);
    }
    const rsibam::Report r = rsibam::stitch(d, len, start, seg, nseg, tid, guess.data(), out.data(), lists.data(), cap, acc.data());
    printf("report %u %u %u %u %u %u %u\nrecs", r.listed, r.seen, r.end, r.flags, r.guessed, r.rewalked, r.passed);
    for (uint32_t s = 0; s < nseg; ++s) for (uint32_t i = 0; i < acc[s]; ++i) printf(" %u", lists[(size_t)s * cap + i]);
    printf("\n");
    free(data);
  }
  return 0;
}
