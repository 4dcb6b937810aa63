// Host driver of rsicnv_amd/csrc/inflate_core.h (the device inflate kernel's decoder, built here as plain C++ under
// ASan + UBSan).  Every member is checked as the kernel checks it: inflate_raw into exactly ISIZE bytes, then the size and
// the CRC32 (as 64 slices combined with the shift constants, the way the kernel's lanes do it).
//   inflate FILE OUT      the BGZF file's members, their text concatenated into OUT; exit 1 on a bad member
//   verdicts FILE OUT     one line per member, "member I: ok" or "member I: <reason>" (rsinf::err_name); the text of the good
//                         members into OUT; exit 0 whatever the verdicts
//   fuzz FILE SEED N      N damaged copies of the file's members (bit flips, truncation, random bytes, random payloads):
//                         each must give an error or exactly the original text; prints counts, exit 1 on a wrong output
#include "../../rsicnv_amd/csrc/inflate_core.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <cstddef>
#include <random>
#include <string>
#include <vector>

namespace {

struct Block { std::vector<uint8_t> payload; uint32_t crc, isize; std::vector<uint8_t> text; };

// the kernel's checks, with nlanes = 1 for the decode and 64 CRC slices
int inflate_member(const std::vector<uint8_t>& payload, uint32_t isize, uint32_t crc, std::vector<uint8_t>& out) {
  if (isize > 65536) return rsinf::kOutputOverrun;
  // exact-size heap copies: a read past the payload or a write past ISIZE is an ASan report
  uint8_t* in = (uint8_t*)malloc(payload.size() ? payload.size() : 1);
  if (!payload.empty()) memcpy(in, payload.data(), payload.size());
  uint8_t* o = (uint8_t*)malloc(isize ? isize : 1);
  rsinf::Work* w = new rsinf::Work;
  uint32_t produced = 0;
  int rc = rsinf::inflate_raw(in, (uint32_t)payload.size(), o, isize, &produced, *w, 0, 1);
  if (rc == rsinf::kOk && produced != isize) rc = rsinf::kSizeMismatch;
  if (rc == rsinf::kOk) {
    static const rsinf::X2n x2n = rsinf::make_x2n();
    const uint32_t slice = (isize + 63) / 64;
    uint32_t c = 0;
    for (uint32_t lane = 0; lane < 64; ++lane) {
      const uint32_t lo = std::min(isize, lane * slice), hi = std::min(isize, lo + slice);
      c ^= rsinf::shift_bytes(x2n.v, rsinf::crc32(0, o + lo, hi - lo), isize - hi);
    }
    if (c != crc) rc = rsinf::kCrcMismatch;
    if (rsinf::crc32(0, o, isize) != c) { fprintf(stderr, "CRC combination differs from the plain CRC\n"); exit(2); }
  }
  if (rc == rsinf::kOk) out.assign(o, o + isize);
  delete w;
  free(o);
  free(in);
  return rc;
}

bool read_blocks(const char* path, std::vector<Block>& blocks) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  std::vector<uint8_t> data;
  uint8_t buf[1 << 16];
  size_t n;
  while ((n = fread(buf, 1, sizeof(buf), f)) > 0) data.insert(data.end(), buf, buf + n);
  fclose(f);
  size_t p = 0;
  while (p < data.size()) {
    rsinf::Member m;
    if (rsinf::bgzf_member(data.data() + p, data.size() - p, m) != 1 || m.bsize > data.size() - p) {
      fprintf(stderr, "not a BGZF member at %zu\n", p);
      return false;
    }
    Block b;
    b.payload.assign(data.begin() + (std::ptrdiff_t)(p + m.hdr), data.begin() + (std::ptrdiff_t)(p + m.hdr + m.clen));
    b.crc = m.crc; b.isize = m.isize;
    blocks.push_back(std::move(b));
    p += m.bsize;
  }
  return true;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 4) { fprintf(stderr, "usage: inflate FILE OUT | verdicts FILE OUT | fuzz FILE SEED N\n"); return 2; }
  std::vector<Block> blocks;
  if (!read_blocks(argv[2], blocks)) return 2;
  const std::string mode = argv[1];
  if (mode == "inflate") {
    FILE* out = fopen(argv[3], "wb");
    if (!out) return 2;
    for (size_t i = 0; i < blocks.size(); ++i) {
      std::vector<uint8_t> t;
      const int rc = inflate_member(blocks[i].payload, blocks[i].isize, blocks[i].crc, t);
      if (rc != rsinf::kOk) { fprintf(stderr, "member %zu: %s\n", i, rsinf::err_name(rc)); fclose(out); return 1; }
      if (!t.empty()) fwrite(t.data(), 1, t.size(), out);
    }
    fclose(out);
    printf("inflate ok: %zu members\n", blocks.size());
    return 0;
  }
  if (mode == "verdicts") {
    FILE* out = fopen(argv[3], "wb");
    if (!out) return 2;
    for (size_t i = 0; i < blocks.size(); ++i) {
      std::vector<uint8_t> t;
      const int rc = inflate_member(blocks[i].payload, blocks[i].isize, blocks[i].crc, t);
      printf("member %zu: %s\n", i, rsinf::err_name(rc));
      if (rc == rsinf::kOk && !t.empty()) fwrite(t.data(), 1, t.size(), out);
    }
    fclose(out);
    return 0;
  }
  if (mode != "fuzz" || argc < 5) return 2;
  for (Block& b : blocks)
    if (inflate_member(b.payload, b.isize, b.crc, b.text) != rsinf::kOk) { fprintf(stderr, "an undamaged member fails\n"); return 1; }
  std::mt19937_64 rng(strtoull(argv[3], nullptr, 0));
  const long iters = strtol(argv[4], nullptr, 0);
  long errors = 0, same = 0, by_kind[4] = {0, 0, 0, 0};
  long by_err[16] = {0};
  for (long it = 0; it < iters; ++it) {
    const Block& b = blocks[rng() % blocks.size()];
    std::vector<uint8_t> p = b.payload;
    uint32_t isize = b.isize, crc = b.crc;
    const int kind = (int)(rng() % 4);
    ++by_kind[kind];
    if (kind == 0 && !p.empty()) {            // 1-8 bit flips
      const int k = 1 + (int)(rng() % 8);
      for (int j = 0; j < k; ++j) p[rng() % p.size()] ^= (uint8_t)(1u << (rng() % 8));
    } else if (kind == 1) {                   // truncated, or a wrong ISIZE
      if (rng() & 1) p.resize(p.empty() ? 0 : rng() % p.size());
      else isize = (uint32_t)(rng() % 65537);
    } else if (kind == 2 && !p.empty()) {     // a run of random bytes
      const size_t at = rng() % p.size(), len = 1 + rng() % 64;
      for (size_t j = at; j < p.size() && j < at + len; ++j) p[j] = (uint8_t)rng();
    } else {                                  // a random payload with the header of a fixed or dynamic block
      p.resize(1 + rng() % 2048);
      for (uint8_t& x : p) x = (uint8_t)rng();
      p[0] = (uint8_t)((p[0] & ~6u) | ((1 + rng() % 2) << 1));
      isize = (uint32_t)(rng() % 65537);
      crc = (uint32_t)rng();
    }
    std::vector<uint8_t> t;
    const int rc = inflate_member(p, isize, crc, t);
    if (rc != rsinf::kOk) { ++errors; ++by_err[rc & 15]; continue; }
    if (t != b.text) { fprintf(stderr, "iteration %ld: accepted output differs from the original\n", it); return 1; }
    ++same;
  }
  printf("fuzz ok: %ld cases, %ld errors, %ld intact;", iters, errors, same);
  for (int e = 1; e < 16; ++e) if (by_err[e]) printf(" %s=%ld", rsinf::err_name(e), by_err[e]);
  printf("\n");
  return 0;
}
