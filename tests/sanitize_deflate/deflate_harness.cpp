// deflate_harness.cpp -- the deflate coder of the device kernel (rsicnv_amd/csrc/deflate_core.h) as plain host C++ (one lane),
// under ASan + UBSan:
//   deflate_harness deflate IN OUT        IN cut into members of 65280 bytes, each a BGZF member in OUT (no end-of-file block);
//                                         prints "deflate ok members M stored S"
//   deflate_harness lengths MAXBITS C...  the code lengths build_codes gives the counts C..., one line "lengths l0 l1 ..."
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <fstream>
#include <iterator>
#include <memory>
#include <string>
#include <vector>

#include "../../rsicnv_amd/csrc/deflate_core.h"

static int run_deflate(const char* in_path, const char* out_path) {
  std::ifstream f(in_path, std::ios::binary);
  if (!f) { fprintf(stderr, "cannot read %s\n", in_path); return 2; }
  const std::string text((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  std::ofstream o(out_path, std::ios::binary);
  auto w = std::make_unique<rsdef::Work>();
  long members = 0, stored_members = 0;
  for (size_t off = 0; off < text.size(); off += rsdef::kMaxText) {
    const uint32_t len = (uint32_t)std::min<size_t>(rsdef::kMaxText, text.size() - off);
    // buffers of exactly the sizes the coder is told: a byte beyond either is a sanitizer report
    std::vector<uint8_t> in(text.begin() + (long)off, text.begin() + (long)off + len);
    const uint32_t cap = len + 5;
    std::vector<uint8_t> member(rsdef::kBgzfHeader + cap + rsdef::kBgzfFooter);
    int stored = 0;
    const uint32_t payload = rsdef::deflate_raw(in.data(), len, member.data() + rsdef::kBgzfHeader, cap, *w, 0, 1, &stored);
    if (payload == 0 || payload > cap) { fprintf(stderr, "member %ld: payload %u of %u\n", members, payload, cap); return 1; }
    rsdef::bgzf_frame(member.data(), payload, rsinf::crc32(0, in.data(), len), len);
    o.write(reinterpret_cast<const char*>(member.data()), rsdef::kBgzfHeader + payload + rsdef::kBgzfFooter);
    ++members;
    stored_members += stored;
  }
  // a capacity one byte short of the stored form, and an empty text: refused, nothing written
  {
    std::vector<uint8_t> in(100, 'a'), out(104, 0xee);
    int stored = 0;
    if (rsdef::deflate_raw(in.data(), 100, out.data(), 104, *w, 0, 1, &stored) != 0 || out[0] != 0xee) return 1;
    if (rsdef::deflate_raw(in.data(), 0, out.data(), 104, *w, 0, 1, &stored) != 0 || out[0] != 0xee) return 1;
  }
  if (!o.flush()) { fprintf(stderr, "cannot write %s\n", out_path); return 2; }
  printf("deflate ok members %ld stored %ld\n", members, stored_members);
  return 0;
}

static int run_lengths(int argc, char** argv) {
  const int maxbits = atoi(argv[2]);
  const int n = argc - 3;
  if (maxbits < 1 || maxbits > 15 || n < 1 || n > 288) { fprintf(stderr, "lengths: bad arguments\n"); return 2; }
  std::vector<uint32_t> cnt((size_t)n);
  for (int i = 0; i < n; ++i) cnt[(size_t)i] = (uint32_t)strtoul(argv[3 + i], nullptr, 10);
  std::vector<uint8_t> len((size_t)n);
  std::vector<uint16_t> code((size_t)n);
  auto w = std::make_unique<rsdef::Work>();
  rsdef::build_codes(cnt.data(), n, maxbits, len.data(), code.data(), *w, 0, 1);
  printf("lengths");
  for (int i = 0; i < n; ++i) printf(" %d", len[(size_t)i]);
  printf("\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 4 && strcmp(argv[1], "deflate") == 0) return run_deflate(argv[2], argv[3]);
  if (argc >= 4 && strcmp(argv[1], "lengths") == 0) return run_lengths(argc, argv);
  fprintf(stderr, "usage: deflate_harness deflate IN OUT | lengths MAXBITS COUNT...\n");
  return 2;
}
