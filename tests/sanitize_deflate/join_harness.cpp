// join_harness.cpp -- the command line's part files joined into a BGZF track (rsicnv_amd/csrc/track_host.h), under ASan + UBSan:
//   join_harness DIR      files under DIR (an empty directory); prints "bgzf join ok"
#include <stdio.h>
#include <stdlib.h>
#include <sys/stat.h>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "../../rsicnv_amd/csrc/track_host.h"

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

static std::string slurp(const std::string& p) {
  std::ifstream f(p, std::ios::binary);
  return std::string(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}
static void spit(const std::string& p, const std::string& s) { std::ofstream f(p, std::ios::binary); f << s; }
static bool exists(const std::string& p) { struct stat st; return stat(p.c_str(), &st) == 0; }

int main(int argc, char** argv) {
  using namespace rsitrack;
  if (argc != 2) { fprintf(stderr, "usage: join_harness DIR\n"); return 2; }
  const std::string dir = argv[1], t = dir + "/t.bedgraph.gz";
  const std::string eof(bgzf_eof(), kBgzfEofBytes);
  CHECK(eof.size() == 28 && (unsigned char)eof[0] == 0x1f && (unsigned char)eof[16] == 27 && eof[18] == 3);
  std::string err;
  // three parts (any bytes: the join does not look inside), one missing: the parts in order, then exactly one end-of-file block
  const std::string big(size_t(3) << 19, 'm');   // longer than the copy buffer
  spit(part_path(t, 2), "two"); spit(part_path(t, 0), big);
  CHECK(join_parts(t, {0, 1, 2}, 3, err, true));
  CHECK(slurp(t) == big + "two" + eof);
  for (size_t i = 0; i < 3; ++i) CHECK(!exists(part_path(t, i)));
  // no parts: the end-of-file block alone, a valid empty BGZF file
  CHECK(join_parts(t, {}, 0, err, true) && slurp(t) == eof);
  // a plain join adds nothing
  spit(part_path(t, 0), "zero\n");
  CHECK(join_parts(t, {0}, 1, err) && slurp(t) == "zero\n");
  // appended to a file, and to one that does not exist yet
  CHECK(append_bgzf_eof(t.c_str()) && slurp(t) == "zero\n" + eof);
  unlink(t.c_str());
  CHECK(append_bgzf_eof(t.c_str()) && slurp(t) == eof);
  CHECK(!append_bgzf_eof((dir + "/no_such_dir/t.gz").c_str()));
  // a failed join leaves nothing, compressed or not
  const std::string bad = dir + "/d.gz";
  CHECK(mkdir(bad.c_str(), 0755) == 0);
  spit(part_path(bad, 0), "zero");
  err.clear();
  CHECK(!join_parts(bad, {0}, 1, err, true) && !err.empty() && !exists(part_path(bad, 0)));
  rmdir(bad.c_str());
  unlink(t.c_str());
  printf("bgzf join ok\n");
  return 0;
}
