// track_harness.cpp -- the host side of the depth-track writer (rsicnv_amd/csrc/track_host.h) alone, under ASan + UBSan:
//   track_harness DIR      every check below, files under DIR (an empty directory); prints "track host ok"
#include <stdio.h>
#include <stdlib.h>
#include <sys/stat.h>
#include <sys/wait.h>
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

static void names() {
  using rsitrack::name_length;
  CHECK(name_length(nullptr) == -1 && name_length("") == -1);
  CHECK(name_length("c") == 1 && name_length("chr 1") == 5);
  CHECK(name_length("chr\t1") == -1 && name_length("chr1\n") == -1 && name_length("\t") == -1);
  const std::string n255(255, 'N'), n256(256, 'N'), n4k(4096, 'N');
  CHECK(name_length(n255.c_str()) == 255 && name_length(n256.c_str()) == -1 && name_length(n4k.c_str()) == -1);
  std::string late = n255; late[254] = '\t';
  CHECK(name_length(late.c_str()) == -1);
}

static void digits() {
  using rsitrack::dec_len;
  char buf[32];
  const long long xs[] = {0, 9, 10, 99, 100, 999999999, 1000000000, 2147483647, 2147483648ll, 9999999999ll, 10000000000ll,
                          INT64_MAX, -1, -9, -10, -2147483648ll, INT64_MIN, INT64_MIN + 1};
  for (long long x : xs) CHECK(dec_len(x) == snprintf(buf, sizeof(buf), "%lld", x));
}

static void plans() {
  using namespace rsitrack;
  Plan p;
  const long long ns[] = {1, 2, 255, 256, 5000, kSliceBases - 1, kSliceBases, kSliceBases + 1, 250000000ll, 1ll << 40};
  const long long p0s[] = {0, 1, -40, 2147483000ll, 9999999990ll, INT64_MAX - (1ll << 40)};
  const long long forced[] = {0, 1, 255, 1024, 65536, kSliceBases, kSliceBases * 4, INT64_MAX};
  for (int name_len : {1, 5, 255})
    for (long long n : ns)
      for (long long pos0 : p0s)
        for (long long s : forced) {
          CHECK(plan(name_len, pos0, n, s, p));
          CHECK(p.slice >= 1 && p.slice <= kSliceBases && p.slice <= n);
          if (s > 0) CHECK(p.slice <= s);
          // the longest line this call can write: name, three tabs and a newline, two coordinates, a value
          char a[32], b[32];
          const int coord = std::max(snprintf(a, sizeof(a), "%lld", pos0), snprintf(b, sizeof(b), "%lld", pos0 + n));
          CHECK(p.max_line == name_len + 4 + 2 * coord + 11);
          CHECK(p.text_cap == (p.slice + 1) * p.max_line && p.text_cap <= kTextBytes);   // one line per base and the carried one fit
        }
  CHECK(!plan(4, 0, -1, 0, p));
  CHECK(!plan(4, INT64_MAX, 1, 0, p) && !plan(4, INT64_MAX - 5, 6, 0, p) && plan(4, INT64_MAX - 5, 5, 0, p));
  CHECK(plan(4, INT64_MIN, 7, 0, p) && p.max_line == 4 + 4 + 2 * 20 + 11);
}

static void writes(const std::string& dir) {
  // a pipe takes 64 KiB at a time: write_all goes on after the short writes while a reader drains it
  int fds[2];
  CHECK(pipe(fds) == 0);
  std::string big(size_t(3) << 20, 'x');
  for (size_t i = 0; i < big.size(); ++i) big[i] = (char)('a' + i % 23);
  const pid_t child = fork();
  CHECK(child >= 0);
  if (child == 0) {
    close(fds[1]);
    std::string got;
    char buf[7001];
    ssize_t k;
    while ((k = read(fds[0], buf, sizeof(buf))) > 0) got.append(buf, (size_t)k);
    _exit(got == big ? 0 : 1);
  }
  close(fds[0]);
  CHECK(rsitrack::write_all(fds[1], big.data(), big.size()));
  close(fds[1]);
  int status = 0;
  CHECK(waitpid(child, &status, 0) == child && WIFEXITED(status) && WEXITSTATUS(status) == 0);
  // a descriptor that cannot be written: false, errno set
  const int ro = open((dir + "/ro").c_str(), O_RDONLY | O_CREAT, 0644);
  CHECK(ro >= 0);
  errno = 0;
  CHECK(!rsitrack::write_all(ro, "abc", 3) && errno != 0);
  close(ro);
  unlink((dir + "/ro").c_str());
  CHECK(rsitrack::write_all(-1, "abc", 0));   // nothing to write: nothing tried
}

static void parts(const std::string& dir) {
  using namespace rsitrack;
  const std::string t = dir + "/t.bedgraph";
  CHECK(part_path(t, 12) == t + ".part.12");
  std::string err;
  // five chromosomes, finished out of order; 1 wrote none; 3's rows were not written (not in the order): its part goes all the same
  std::string big(size_t(5) << 19, 'q');   // longer than the copy buffer
  spit(part_path(t, 4), "four\n"); spit(part_path(t, 0), "zero\n"); spit(part_path(t, 2), big); spit(part_path(t, 3), "three\n");
  spit(t, "an older track\n");
  CHECK(join_parts(t, {0, 1, 2, 4}, 5, err));
  CHECK(slurp(t) == "zero\n" + big + "four\n");
  for (size_t i = 0; i < 5; ++i) CHECK(!exists(part_path(t, i)));
  // no parts at all: an empty track
  CHECK(join_parts(t, {}, 0, err) && exists(t) && slurp(t).empty());
  // the track cannot be created: the parts are deleted, nothing is left, the reason is given
  const std::string bad = dir + "/missing_dir/t.bedgraph";
  CHECK(mkdir((dir + "/missing_dir").c_str(), 0755) == 0);
  spit(part_path(bad, 0), "zero\n"); spit(part_path(bad, 1), "one\n");
  CHECK(mkdir(bad.c_str(), 0755) == 0);   // a directory where the file should go
  err.clear();
  CHECK(!join_parts(bad, {0, 1}, 2, err) && !err.empty());
  CHECK(!exists(part_path(bad, 0)) && !exists(part_path(bad, 1)));
  rmdir(bad.c_str());
  // a part that cannot be read (a directory): failure, everything removed, the track too
  spit(part_path(bad, 0), "zero\n");
  CHECK(mkdir(part_path(bad, 1).c_str(), 0755) == 0);
  err.clear();
  CHECK(!join_parts(bad, {0, 1}, 2, err) && err.find(".part.1") != std::string::npos);
  CHECK(!exists(bad) && !exists(part_path(bad, 0)));
  rmdir(part_path(bad, 1).c_str());
  rmdir((dir + "/missing_dir").c_str());
  remove_parts(t, 3);   // parts that are not there: no complaint
  unlink(t.c_str());
}

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: track_harness DIR\n"); return 2; }
  names();
  digits();
  plans();
  writes(argv[1]);
  parts(argv[1]);
  printf("track host ok\n");
  return 0;
}
