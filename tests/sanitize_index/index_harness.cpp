// index_harness.cpp -- the tabix index's host side (rsicnv_amd/csrc/track_index_host.h) alone, under ASan + UBSan:
//   index_harness build DIR          drives the builder with hand-made slice records, checks what it holds, and writes DIR/one.tbi,
//                                    DIR/two.tbi and DIR/joined.tbi, which tests/test_track_index_host.py parses back field by field
//   index_harness parse FILE NAME    parses a .tbi / .csi and prints "ok KIND MIN_SHIFT DEPTH NREF BEG END" for NAME's range
//                                    ("ok ... none" when the index holds no line of it), or "error: ..." and exit status 2
#include "../../rsicnv_amd/csrc/track_index_host.h"
#include <stdlib.h>

using rsitbx::Rec;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

static uint64_t vo(uint64_t coff, uint64_t uoff) { return coff << 16 | uoff; }

static int build(const std::string& dir) {
  rsi_track_index one;
  // chrA, slice 0: bytes [0, 1000) of the file; the records arrive out of order, as an atomic counter leaves them
  {
    const Rec c[] = {{vo(400, 7), 4682, 0}, {vo(0, 0), 4681, 0}, {vo(700, 0), 585, 0}};
    const Rec w[] = {{vo(400, 7), 1, 1}, {vo(0, 0), 0, 0}, {vo(700, 0), 2, 2}};
    CHECK(one.add_slice("chrA", 0, 1000, c, 3, w, 3) == rsitbx::kOk);
  }
  // slice 1: bytes [1000, 1600): its first chunk goes on in bin 585 and touches -> merged; its first line reaches no new window,
  // its second one windows 3 .. 6 of which 3 is new ground behind window 2
  {
    const Rec c[] = {{vo(0, 0), 585, 0}, {vo(300, 50), 4681 + 6, 0}};
    const Rec w[] = {{vo(0, 0), 2, 2}, {vo(300, 50), 3, 6}};
    CHECK(one.add_slice("chrA", 1000, 600, c, 2, w, 2) == rsitbx::kOk);
  }
  // a slice without a line, then another call of the same name: goes on with chrA, merged again; windows 7 and 8 stay untouched
  CHECK(one.add_slice("chrA", 1600, 100, nullptr, 0, nullptr, 0) == rsitbx::kOk);
  {
    const Rec c[] = {{vo(0, 0), 4681 + 6, 0}, {vo(10, 3), 4681 + 9, 0}};
    const Rec w[] = {{vo(0, 0), 6, 6}, {vo(10, 3), 9, 9}};
    CHECK(one.add_slice("chrA", 1600, 200, c, 2, w, 2) == rsitbx::kOk);
  }
  // a chromosome that wrote no line is not listed; chrB begins in window 2: windows 0 and 1 take its first line
  CHECK(one.add_slice("chrEmpty", 1800, 50, nullptr, 0, nullptr, 0) == rsitbx::kOk);
  {
    const Rec c[] = {{vo(0, 0), 4681 + 2, 0}};
    const Rec w[] = {{vo(0, 0), 2, 2}};
    CHECK(one.add_slice("chrB", 1800, 64, c, 1, w, 1) == rsitbx::kOk);
  }
  CHECK(one.chroms.size() == 2 && one.chroms[0].name == "chrA" && one.chroms[1].name == "chrB");
  const std::vector<rsitbx::Chunk>& k = one.chroms[0].chunks;
  CHECK(k.size() == 5);
  CHECK(k[0].bin == 4681 && k[0].beg == vo(0, 0) && k[0].end == vo(400, 7));
  CHECK(k[1].bin == 4682 && k[1].end == vo(700, 0));
  CHECK(k[2].bin == 585 && k[2].beg == vo(700, 0) && k[2].end == vo(1300, 50));      // across the slice boundary at 1000
  CHECK(k[3].bin == 4687 && k[3].beg == vo(1300, 50) && k[3].end == vo(1610, 3));    // across the call boundary at 1600
  CHECK(k[4].bin == 4690 && k[4].end == vo(1800, 0));
  const std::vector<uint64_t>& lin = one.chroms[0].linear;
  CHECK(lin.size() == 10 && lin[2] == vo(700, 0) && lin[3] == vo(1300, 50) && lin[6] == vo(1300, 50));
  CHECK(lin[7] == rsitbx::kNoOffset && lin[8] == rsitbx::kNoOffset && lin[9] == vo(1610, 3));
  int64_t nref = 0, nchunks = 0, nwin = 0;
  one.counts(nref, nchunks, nwin);
  CHECK(nref == 2 && nchunks == 6 && nwin == 13);
  CHECK(one.write_tbi((dir + "/one.tbi").c_str()));

  // the 2^29 limit: a window record beyond the last window is refused, with the limit in the message, and nothing is added
  rsi_track_index two;
  {
    const Rec c[] = {{vo(0, 0), 4681 + 32767, 0}};
    const Rec far[] = {{vo(0, 0), 32767, 32768}};
    CHECK(two.add_slice("chrC", 0, 100, c, 1, far, 1) == rsitbx::kUnsupported && two.err.find("536870912") != std::string::npos);
    CHECK(two.chroms.empty());
    const Rec w[] = {{vo(0, 0), 32767, 32767}};
    CHECK(two.add_slice("chrC", 0, 100, c, 1, w, 1) == rsitbx::kOk);
    CHECK(two.chroms[0].linear.size() == 32768);
  }
  // records that cannot be: an offset behind the slice, a bin that does not exist, a first chunk not at the slice's start
  {
    rsi_track_index bad;
    const Rec c1[] = {{vo(100, 0), 4681, 0}}, c2[] = {{vo(0, 0), 37449, 0}}, c3[] = {{vo(5, 0), 4681, 0}}, ok[] = {{vo(0, 0), 4681, 0}};
    const Rec w[] = {{vo(0, 0), 0, 0}}, w2[] = {{vo(0, 0), 3, 2}};
    CHECK(bad.add_slice("x", 0, 100, c1, 1, w, 1) == rsitbx::kBadRecords);
    CHECK(bad.add_slice("x", 0, 100, c2, 1, w, 1) == rsitbx::kBadRecords);
    CHECK(bad.add_slice("x", 0, 100, c3, 1, w, 1) == rsitbx::kBadRecords);
    CHECK(bad.add_slice("x", 0, 100, ok, 1, w2, 1) == rsitbx::kBadRecords);
    CHECK(bad.add_slice("x", -1, 100, ok, 1, w, 1) == rsitbx::kBadRecords);
    CHECK(bad.chroms.empty());
  }
  CHECK(two.write_tbi((dir + "/two.tbi").c_str()));

  // append: two's chromosome behind one's, moved by 5000 bytes; a second append moves by 0
  rsi_track_index joined;
  CHECK(joined.append(one, 0) == rsitbx::kOk && joined.append(two, 5000) == rsitbx::kOk);
  CHECK(joined.append(two, -1) == rsitbx::kBadRecords);
  CHECK(joined.chroms.size() == 3 && joined.chroms[2].chunks[0].beg == vo(5000, 0) && joined.chroms[2].chunks[0].end == vo(5100, 0));
  CHECK(joined.chroms[2].linear[0] == rsitbx::kNoOffset && joined.chroms[2].linear[32767] == vo(5000, 0));
  CHECK(joined.chroms[0].chunks[2].end == vo(1300, 50) && two.chroms[0].chunks[0].beg == vo(0, 0));
  CHECK(joined.write_tbi((dir + "/joined.tbi").c_str()));
  CHECK(!joined.write_tbi((dir + "/no_such_dir/x.tbi").c_str()) && joined.err.find("no_such_dir") != std::string::npos);

  // two parts of one chromosome: the second part's index goes on with the chromosome the first ends with, as a later slice would
  {
    rsi_track_index front, back;
    const Rec c1[] = {{vo(0, 0), 4681, 0}, {vo(50, 9), 4682, 0}}, w1[] = {{vo(0, 0), 0, 0}, {vo(50, 9), 1, 1}};
    const Rec c2[] = {{vo(0, 0), 4682, 0}, {vo(30, 2), 4685, 0}}, w2[] = {{vo(0, 0), 1, 1}, {vo(30, 2), 2, 4}};
    CHECK(front.add_slice("chrA", 0, 100, c1, 2, w1, 2) == rsitbx::kOk);
    CHECK(back.add_slice("chrA", 0, 80, c2, 2, w2, 2) == rsitbx::kOk);
    const Rec c3[] = {{vo(0, 0), 4681, 0}}, w3[] = {{vo(0, 0), 0, 0}};
    CHECK(back.add_slice("chrB", 80, 20, c3, 1, w3, 1) == rsitbx::kOk);
    CHECK(front.append(back, 100) == rsitbx::kOk);
    CHECK(front.chroms.size() == 2 && front.chroms[0].name == "chrA" && front.chroms[1].name == "chrB");
    const std::vector<rsitbx::Chunk>& m = front.chroms[0].chunks;
    CHECK(m.size() == 3 && m[1].bin == 4682 && m[1].beg == vo(50, 9) && m[1].end == vo(130, 2) && m[2].end == vo(180, 0));
    const std::vector<uint64_t>& l = front.chroms[0].linear;
    CHECK(l.size() == 5 && l[0] == vo(0, 0) && l[1] == vo(50, 9) && l[2] == vo(130, 2) && l[4] == vo(130, 2) && front.chroms[0].reached == 4);
    CHECK(front.chroms[1].chunks[0].beg == vo(180, 0));
  }
  // an index without a chromosome is a valid, empty .tbi
  rsi_track_index none;
  CHECK(none.write_tbi((dir + "/none.tbi").c_str()));
  // what the library wrote, its own parser reads
  rsitbx::FileIndex fi;
  std::string err;
  CHECK(rsitbx::read_index(dir + "/joined.tbi", fi, err) && !fi.csi && fi.refs.size() == 3);
  uint64_t b = 0, e = 0;
  CHECK(rsitbx::locate(fi, "A", b, e) && b == vo(0, 0) && e == vo(1800, 0));
  CHECK(rsitbx::locate(fi, "chrC", b, e) && b == vo(5000, 0) && e == vo(5100, 0));
  CHECK(!rsitbx::locate(fi, "chrEmpty", b, e));
  CHECK(rsitbx::read_index(dir + "/none.tbi", fi, err) && fi.refs.empty());
  printf("index host ok\n");
  return 0;
}

static int parse(const std::string& file, const std::string& name) {
  rsitbx::FileIndex fi;
  std::string err;
  if (!rsitbx::read_index(file, fi, err)) { printf("error: %s\n", err.c_str()); return 2; }
  uint64_t b = 0, e = 0;
  if (rsitbx::locate(fi, name, b, e))
    printf("ok %s %d %d %zu %llu %llu\n", fi.csi ? "csi" : "tbi", fi.min_shift, fi.depth, fi.refs.size(), (unsigned long long)b, (unsigned long long)e);
  else
    printf("ok %s %d %d %zu none\n", fi.csi ? "csi" : "tbi", fi.min_shift, fi.depth, fi.refs.size());
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 3 && std::string(argv[1]) == "build") return build(argv[2]);
  if (argc == 4 && std::string(argv[1]) == "parse") return parse(argv[2], argv[3]);
  fprintf(stderr, "usage: index_harness build DIR | parse FILE NAME\n");
  return 64;
}
