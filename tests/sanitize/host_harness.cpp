// host_harness.cpp -- CPU-only driver of the product's HOST code for the sanitizer build (tests/sanitize/Makefile: ASan +
// UBSan; test infrastructure, never shipped).  It runs, on seeded synthetic chromosomes,
//   * hostmath.h's histogram quantiles against the oracle's (the CPU restatement, pinned to the reference elsewhere),
//   * host_calls.cpp's candidate stages (block tests, sharpening, neighbourhood tests, merge, final filters) on their
//     host path -- the depth in host memory, no device tester -- from the oracle's bin arrays and segments, and compares
//     blocks / raw calls / final calls with the oracle's,
//   * pipeline_steps.h's host decisions between the pipeline's kernels (regions and compaction table, chromosome statistics, NB
//     levels, scan parameters, filterstatus' level choice, segments) from the oracle's arrays of the same chromosomes against the
//     oracle's results, and on hand-made edge inputs,
//   * bam_host.cpp's BGZF / BAM / BAI reader and the read-pair annotation on a BAM given on the command line, then on
//     truncated and bit-flipped copies of it (errors are fine, memory errors are not).
// Exit status 0 = everything agreed and the sanitizers stayed quiet.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <fstream>
#include <random>
#include <string>
#include <vector>

#include "../../include/rsi_hot.h"
#include "../../include/rsi_synth.h"
#include "../../rsicnv_amd/csrc/bam_host.h"
#include "../../rsicnv_amd/csrc/host_calls.h"
#include "../../rsicnv_amd/csrc/hostmath.h"
#include "../../rsicnv_amd/csrc/pipeline_steps.h"

extern "C" {   // oracle/rsi_oracle.cpp
struct orc_params { int32_t m, gcadjust, trans, merge, maxchkbp, debug; double cap, epsilon, threshold, chklen, minmlen, buffer, p; };
struct orc_call { int32_t start, end, type, geno, status, length, qscore, pad; double score, p1, cnvmed, cnvsd, cnviqr, refmed, refsd, refiqr; };
void* orc_create(void);
void orc_destroy(void* h);
void orc_default_params(orc_params* p);
int orc_run(void* h, const orc_params* p, const int32_t* depth, const uint8_t* fasta, int32_t n, int32_t keep_snapshots);
int64_t orc_get_i32(void* h, const char* name, int32_t* out, int64_t cap);
int64_t orc_get_f32(void* h, const char* name, float* out, int64_t cap);
int64_t orc_get_f64(void* h, const char* name, double* out, int64_t cap);
int orc_get_calls(void* h, const char* which, orc_call* out, int32_t cap);
double orc_median_i32(const int32_t* x, int64_t n);
double orc_median_f32(const float* x, int64_t n);
double orc_median_f64(const double* x, int64_t n);
}

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); ++g_fail; } } while (0)

static std::vector<int32_t> geti(void* h, const char* name) {
  const int64_t k = orc_get_i32(h, name, nullptr, 0);
  std::vector<int32_t> v((size_t)(k > 0 ? k : 0));
  if (k > 0) orc_get_i32(h, name, v.data(), k);
  return v;
}
static std::vector<float> getf(void* h, const char* name) {
  const int64_t k = orc_get_f32(h, name, nullptr, 0);
  std::vector<float> v((size_t)(k > 0 ? k : 0));
  if (k > 0) orc_get_f32(h, name, v.data(), k);
  return v;
}
static std::vector<orc_call> getc(void* h, const char* which) {
  const int k = orc_get_calls(h, which, nullptr, 0);
  std::vector<orc_call> v((size_t)(k > 0 ? k : 0));
  if (k > 0) orc_get_calls(h, which, v.data(), k);
  return v;
}

static void quantile_checks() {
  std::mt19937_64 rng(7);
  for (int n : {1, 2, 3, 4, 5, 31, 100, 1001, 50000}) {
    std::vector<int> xi((size_t)n); std::vector<float> xf((size_t)n); std::vector<double> xd((size_t)n);
    std::poisson_distribution<int> po(30); std::gamma_distribution<double> ga(9.0, 3.3);
    for (int i = 0; i < n; ++i) { xi[(size_t)i] = po(rng); xf[(size_t)i] = (float)ga(rng); xd[(size_t)i] = (double)xf[(size_t)i] * 1.37; }
    CHECK(rsih::grid_quantiles(xi.data(), (size_t)n).med == orc_median_i32(xi.data(), n), "int median, n=%d", n);
    CHECK(rsih::grid_quantiles(xf.data(), (size_t)n).med == orc_median_f32(xf.data(), n), "float median, n=%d", n);
    CHECK(rsih::grid_quantiles(xd.data(), (size_t)n).med == orc_median_f64(xd.data(), n), "double median, n=%d", n);
    // device-style integer histogram -> quantiles
    int lo = xi[0], hi = xi[0];
    for (int v : xi) { lo = v < lo ? v : lo; hi = v > hi ? v : hi; }
    std::vector<uint64_t> h((size_t)hi + 1, 0);
    for (int v : xi) ++h[(size_t)v];
    rsih::Quantiles q;
    CHECK(rsih::hist_quantiles_int(h.data(), h.size(), (uint64_t)n, q) && q.med == orc_median_i32(xi.data(), n), "histogram median, n=%d", n);
  }
}

static bool same_calls(const std::vector<rsih::Candidate>& a, const std::vector<orc_call>& b, const char* what) {
  if (a.size() != b.size()) { CHECK(false, "%s: %zu calls, oracle %zu", what, a.size(), b.size()); return false; }
  for (size_t i = 0; i < a.size(); ++i) {
    const bool ok = a[i].start == b[i].start && a[i].end == b[i].end && a[i].type == b[i].type && a[i].status == b[i].status &&
                    a[i].length == b[i].length && fabs(a[i].p1 - b[i].p1) <= 1e-9 * fabs(b[i].p1) + 1e-300 &&
                    fabs(a[i].cnvmed - b[i].cnvmed) <= 1e-9 * fabs(b[i].cnvmed) && fabs(a[i].refmed - b[i].refmed) <= 1e-9 * fabs(b[i].refmed);
    CHECK(ok, "%s: call %zu differs (%d-%d type %d vs %d-%d type %d)", what, i, a[i].start, a[i].end, a[i].type, b[i].start, b[i].end, b[i].type);
    if (!ok) return false;
  }
  return true;
}

static void pipeline_step_checks(void* O, const orc_params& P, const std::vector<uint8_t>& fasta, uint64_t seed);   // below

static void candidate_stage_case(uint64_t seed, int n, int model, const orc_params& P, int deep_bimodal = 0) {
  // a chromosome with N runs at the ends, one gap and a few events (layout as tests/conftest.py's plans)
  std::vector<rsi_synth_interval_c> nruns = {{0, 4000, 0, 0}, {n / 2, n / 2 + 6000, 0, 0}, {n - 4000, n, 0, 0}};
  std::vector<rsi_synth_interval_c> events;
  const int codes[5] = {2, 3, 1, 4, 2};
  for (int e = 0; e < 5; ++e) { const int64_t b = 20000 + (int64_t)e * (n / 6); events.push_back({b, b + 3000 + 4000 * e, codes[e], 0}); }
  for (auto& ev : events) if (ev.beg < n / 2 + 6000 && ev.end > n / 2) { ev.beg += 20000; ev.end += 20000; }
  rsi_synth_spec spec;
  memset(&spec, 0, sizeof(spec));
  spec.seed = seed; spec.n = n; spec.model = model; spec.mean = 30.0; spec.nb_size = 10.0;
  spec.events = events.data(); spec.n_events = (int)events.size(); spec.nruns = nruns.data(); spec.n_nruns = (int)nruns.size();
  std::vector<uint8_t> fasta((size_t)n); std::vector<int32_t> depth((size_t)n);
  CHECK(rsi_synth_generate_host(&spec, fasta.data(), depth.data()) == 0, "generator");
  if (deep_bimodal) {   // 300x with the second half three times as deep: ~1800 segments, hundreds of candidates, neighbour chains
                        // cut at 48, a candidate whose first edge refinement leaves end < start (the reference indexes its
                        // vector out of range there; oracle and library search the entries that exist -- this case under
                        // AddressSanitizer is what keeps both honest), thinned neighbourhoods of a 170 kb candidate
    for (int i = 0; i < n; ++i) if (depth[(size_t)i] > 0) depth[(size_t)i] = depth[(size_t)i] * 10 + (int)((seed + (uint64_t)i * 2654435761u) % 10);
    for (int i = n * 9 / 20; i < n; ++i) if (depth[(size_t)i] > 0) depth[(size_t)i] = depth[(size_t)i] * 3 + 1;
  }
  void* O = orc_create();
  orc_run(O, &P, depth.data(), fasta.data(), n, 0);
  const std::vector<int32_t> rdc = geti(O, "rd_concat"), medint = geti(O, "binmedint"), noncode = geti(O, "noncode");
  const bool med = P.trans == 1;
  const std::vector<int32_t> st2 = geti(O, med ? "med_status2" : "nb_status2");
  const std::vector<orc_call> segs_o = getc(O, med ? "segs_med" : "segs_nb");
  double chrom[4];
  orc_get_f64(O, "chrom", chrom, 4);
  rsih::CallerInput in;
  memset(&in.P, 0, sizeof(in.P));
  in.P.m = P.m; in.P.gcadjust = P.gcadjust; in.P.trans = P.trans; in.P.merge = P.merge; in.P.maxchkbp = P.maxchkbp; in.P.debug = 0;
  in.P.cap = P.cap; in.P.epsilon = P.epsilon; in.P.threshold = P.threshold; in.P.chklen = P.chklen; in.P.minmlen = P.minmlen; in.P.buffer = P.buffer; in.P.p = P.p;
  in.RDmedian = chrom[0]; in.RDsd = chrom[1]; in.ncompact = (int64_t)rdc.size();
  std::vector<rsih::Region> regions;
  for (size_t i = 0; i + 1 < noncode.size(); i += 2) regions.push_back({noncode[i], noncode[i + 1]});
  in.noncode = &regions;
  std::vector<int> mi(medint.begin(), medint.end()), status(st2.begin(), st2.end());
  in.binmedint = rsih::IntSpan(mi);
  std::vector<rsih::Candidate> segs;
  for (const orc_call& c : segs_o) { rsih::Candidate k; k.start = c.start; k.end = c.end; k.type = c.type; k.score = c.score; segs.push_back(k); }
  rsih::test_block_segments(in, status, segs);                        // areblockscnv, rsi.cpp:1847
  rsih::DepthPager pager(rdc.data(), (int64_t)rdc.size());
  std::vector<rsih::Candidate> blocks, raw, kept;
  rsih::call_from_segments(in, segs, pager, blocks, raw, kept);       // rsi.cpp:1860-1931 + sd_filters
  same_calls(blocks, getc(O, "blocks"), "blocks");
  same_calls(raw, getc(O, "calls_raw"), "calls_raw");
  same_calls(kept, getc(O, "calls"), "calls");
  CHECK(!raw.empty(), "the case should call something (seed %llu)", (unsigned long long)seed);
  if (deep_bimodal) CHECK(raw.size() > 100, "the bimodal case should be crowded (%zu raw calls)", raw.size());
  pipeline_step_checks(O, P, fasta, seed);
  orc_destroy(O);
}

// ---- the pipeline's host decisions (pipeline_steps.h) -------------------------------------------------------------------------------
// Run boundaries (pos << 1 | is_end) of a status array as k_resolve_runs emits them (a run: adjacent marked bins of one sign),
// shuffled: the device appends them unordered.  Then the runs in the reference's sense (the last one is not emitted, Q11).
static std::vector<rsih::Region> marked_runs(const std::vector<int32_t>& st, std::mt19937_64& rng) {
  std::vector<uint64_t> ent;
  const int64_t nb = (int64_t)st.size();
  for (int64_t i = 0; i < nb; ++i) {
    const int s = st[(size_t)i];
    if (s == 0) continue;
    const int p = i > 0 ? st[(size_t)i - 1] : 0, q = i + 1 < nb ? st[(size_t)i + 1] : 0;
    if (p == 0 || ((p > 0) != (s > 0))) ent.push_back((uint64_t)i << 1);
    if (q == 0 || ((q > 0) != (s > 0))) ent.push_back(((uint64_t)i << 1) | 1);
  }
  std::shuffle(ent.begin(), ent.end(), rng);
  std::vector<rsih::Region> runs;
  CHECK(rsih::boundary_pairs(ent.data(), ent.size(), false, runs), "run boundaries of a status array are balanced");
  if (!runs.empty()) runs.pop_back();
  return runs;
}

static void pipeline_step_checks(void* O, const orc_params& P, const std::vector<uint8_t>& fasta, uint64_t seed) {
  const int n = (int)fasta.size();
  const bool med = P.trans == 1;
  const char* pre = med ? "med" : "nb";
  auto name = [&](const char* what) { return std::string(pre) + what; };
  std::mt19937_64 rng(seed);
  const std::vector<int32_t> rdc = geti(O, "rd_concat"), noncode = geti(O, "noncode");
  double chrom[4], nbv[6], sc[11];
  orc_get_f64(O, "chrom", chrom, 4);
  orc_get_f64(O, "nb", nbv, 6);                                   // median, MAD, r, raw minimum, factor, LmaxBase
  CHECK(orc_get_f64(O, med ? "scan_med" : "scan_nb", sc, 11) == 11, "the oracle's scan record has 11 entries");   // ..., [6] target, [7] Lmax, [8] cal_max, [10] absmed

  // regions and compaction table: the N runs of the FASTA by a plain loop
  std::vector<uint64_t> ent;
  for (int i = 0; i < n; ++i) {
    if (fasta[(size_t)i] != 'N') continue;
    if (i == 0 || fasta[(size_t)i - 1] != 'N') ent.push_back((uint64_t)i << 1);
    if (i == n - 1 || fasta[(size_t)i + 1] != 'N') ent.push_back(((uint64_t)(i + 1) << 1) | 1);   // exclusive end
  }
  std::shuffle(ent.begin(), ent.end(), rng);
  std::vector<rsih::Region> nruns;
  CHECK(rsih::boundary_pairs(ent.data(), ent.size(), true, nruns), "N-run boundaries are balanced");
  const std::vector<rsih::Region> regs = rsih::noncode_regions(nruns, n, std::max(50, P.m / 4));
  bool same = regs.size() * 2 == noncode.size();
  for (size_t k = 0; same && k < regs.size(); ++k) same = regs[k].start == noncode[2 * k] && regs[k].end == noncode[2 * k + 1];
  CHECK(same, "noncode_regions: %zu regions, oracle %zu, or a pair differs", regs.size(), noncode.size() / 2);
  const rsih::CompactTable ct = rsih::compact_table(regs, n);
  CHECK(ct.ncompact == (int64_t)rdc.size(), "compact_table: n' %lld, oracle %zu", (long long)ct.ncompact, rdc.size());

  // chromosome statistics from the residue-class histogram ([value][32], kernels.h: class = index mod 31 below 31 * (n' / 31),
  // class 31 for the tail) and from the array itself
  const int64_t nc = (int64_t)rdc.size(), body = 31 * (nc / 31);
  const size_t res_vals = (size_t)*std::max_element(rdc.begin(), rdc.end()) + 1;
  std::vector<uint32_t> hres(res_vals * rsik::kResClasses, 0);
  for (int64_t i = 0; i < nc; ++i) ++hres[(size_t)rdc[(size_t)i] * rsik::kResClasses + (size_t)(i < body ? i % 31 : 31)];
  auto sd_close = [&](double sd) { return fabs(sd - chrom[1]) <= 1e-12 * fabs(chrom[1]); };
  rsih::ChromStats hs, as;
  double hmads[31] = {0}, amads[31] = {0};
  CHECK(rsih::hist_chrom_stats(hres.data(), res_vals, nc, hs) && hs.median == chrom[0], "histogram median %g, oracle %g", hs.median, chrom[0]);
  CHECK(sd_close(hs.sd), "histogram SD %.17g, oracle %.17g", hs.sd, chrom[1]);
  CHECK(rsih::hist_subsample_mads(hres.data(), res_vals, chrom[0], (uint64_t)(nc / 31), hmads) && rsih::grid_quantiles(hmads, (size_t)31).med == nbv[1],
        "histogram MAD, oracle %g", nbv[1]);
  rsih::array_chrom_stats(rdc, as, amads);
  CHECK(as.median == chrom[0] && sd_close(as.sd) && rsih::grid_quantiles(amads, (size_t)31).med == nbv[1],
        "array statistics: median %g SD %.17g, oracle %g %.17g MAD %g", as.median, as.sd, chrom[0], chrom[1], nbv[1]);
  for (int j = 0; j < 31; ++j) CHECK(hmads[j] == amads[j], "subsample %d: MAD %g from the histogram, %g from the array", j, hmads[j], amads[j]);

  // NB reference levels: bins 0 and 2 of the transformed array carry the scaled DEL and median levels (App. A Q9)
  const std::vector<float> binnb = getf(O, "binnb");
  const rsih::NbLevels lev = rsih::nb_reference_levels(nbv[0], P.m, nbv[2]);
  const rsih::NbScaled lv = rsih::nb_scaled_levels(nbv[3], lev.med_raw, lev.del_raw, nbv[0]);
  CHECK(lv.t0 == binnb[0] && lv.t2 == binnb[2], "NB levels %.9g %.9g, oracle %.9g %.9g", lv.t0, lv.t2, binnb[0], binnb[2]);

  // scan parameters
  const std::vector<float> T = med ? getf(O, "binmed") : binnb;
  const int64_t nb = (int64_t)T.size();
  const rsih::ScanSetup su = rsih::scan_first_pass(med, sc[0], sc[10], nbv[4], (int)nbv[5], T[0], T[2], P.threshold, nb);
  CHECK(su.tsigma == sc[1] && su.tlamda == sc[2] && su.target == sc[6] && su.cal_max == (int)sc[8] && su.Lmax_ref == (int)sc[7],
        "scan parameters: tsigma %.17g tlamda %.17g target %.17g cal_max %d Lmax %d, oracle %.17g %.17g %.17g %d %d", su.tsigma, su.tlamda,
        su.target, su.cal_max, su.Lmax_ref, sc[1], sc[2], sc[6], (int)sc[8], (int)sc[7]);
  CHECK(!su.clipped && su.Lmax == su.Lmax_ref, "a synthetic chromosome has more bins than scan lengths");

  // filterstatus: the host loop and the level choice against rsi.cpp:948-1002 restated over the same arrays
  const std::vector<int32_t> st1 = geti(O, name("_status1").c_str()), st1f = geti(O, name("_status1f").c_str());
  const int Lmax = su.Lmax;
  std::vector<float> wsum((size_t)(2 * Lmax + 1), 1.0f);
  std::vector<int> wcnt((size_t)(2 * Lmax + 1), 1);
  rsih::level_sums_host(T.data(), st1.data(), nb, Lmax, wsum, wcnt);
  const rsih::LevelChoice lc = rsih::choose_levels(wsum, wcnt, Lmax, su.dev);
  int minl = st1[0], maxl = st1[0];
  for (int32_t v : st1) { minl = std::min(minl, v); maxl = std::max(maxl, v); }
  const int nl = maxl - minl + 1;
  std::vector<float> lsum((size_t)nl, 0.0f);
  std::vector<int> lcnt((size_t)nl, 0);
  for (int64_t i = 0; i < nb; ++i) { lsum[(size_t)(st1[(size_t)i] - minl)] += T[(size_t)i]; ++lcnt[(size_t)(st1[(size_t)i] - minl)]; }   // float accumulators
  for (int l = 0; l < nl; ++l) if (lcnt[(size_t)l] != 0) lsum[(size_t)l] /= (double)lcnt[(size_t)l];
  const bool level0 = !(-minl < 0 || -minl >= nl);
  CHECK(lc.lo == minl && lc.hi == maxl && lc.has_level0 == level0, "level range [%d, %d], restated [%d, %d]", lc.lo, lc.hi, minl, maxl);
  std::vector<int32_t> trimmed = st1;
  if (level0 && lc.has_level0) {
    const float m0 = lsum[(size_t)-minl];
    int leveldel = minl, leveladd = maxl;
    for (int l = 0; l < nl; ++l) if (lsum[(size_t)l] < m0 - su.dev) { leveldel = l + minl; break; }
    for (int l = nl - 1; l >= 0; --l) if (lsum[(size_t)l] > m0 + su.dev) { leveladd = l + minl; break; }
    const bool trim = !(leveldel > 0 || leveladd < 0 || leveldel > leveladd);
    CHECK(lc.m0 == m0 && lc.leveldel == leveldel && lc.leveladd == leveladd && lc.trim == trim,
          "level choice m0 %.9g del %d add %d trim %d, restated %.9g %d %d %d", lc.m0, lc.leveldel, lc.leveladd, (int)lc.trim, m0, leveldel, leveladd, (int)trim);
    size_t populated = 0;
    for (int c : lcnt) populated += c != 0;
    CHECK(lc.lines.size() == populated + 2 + (trim ? 0 : 1), "level table: %zu lines for %zu populated levels", lc.lines.size(), populated);
    if (lc.trim) {   // k_trim_runs' rule (rsi.cpp:1023-1044) in plain C++, over the runs as the pipeline gets them
      const double delthr = (double)lc.m0 - su.dev, addthr = (double)lc.m0 + su.dev;
      for (const rsih::Region& r : marked_runs(st1, rng)) {
        int i1 = r.start, i2 = r.end;
        auto within = [&](int i) { return (T[(size_t)i] > delthr && trimmed[(size_t)i] < 0) || (T[(size_t)i] < addthr && trimmed[(size_t)i] > 0); };
        while (within(i1)) { trimmed[(size_t)i1] = 0; ++i1; if (i1 >= i2) break; }
        while (within(i2)) { trimmed[(size_t)i2] = 0; --i2; if (i2 <= i1) break; }
      }
    }
  }
  CHECK(trimmed == st1f, "status after the level choice and the trim differs from the oracle's %s_status1f", pre);

  // segments: runs of the second pass' status, the item plan, a plain best subsegment per item (the kernel's visiting order:
  // larger score, then smaller L, then smaller offset), one candidate per run
  const std::vector<int32_t> st2 = geti(O, name("_status2").c_str());
  const std::vector<rsih::Region> runs = marked_runs(st2, rng);
  const double tmedian2 = sc[3], tlamda2 = sc[5];
  std::vector<int64_t> poff;
  std::vector<rsik::SegItem> items;
  rsih::segment_items(runs, (int64_t)1 << 13, poff, items);
  CHECK(poff.size() == runs.size() + 1 && (runs.empty() || !items.empty()), "item plan: offsets and items");
  std::vector<rsik::BestSeg> best(items.size(), rsik::BestSeg{0.0, 0, 0});
  std::vector<double> prefix;
  for (size_t i = 0; i < items.size(); ++i) {
    const rsik::SegItem& it = items[i];
    const rsih::Region& r = runs[(size_t)it.run];
    CHECK(it.len == r.end - r.start + 1 && it.Lbeg >= 1 && it.Lbeg < it.Lend && it.Lend <= it.len + 1 &&
          (i == 0 || items[i - 1].run != it.run ? it.Lbeg == 1 : it.Lbeg == items[i - 1].Lend), "item %zu does not continue its run's lengths", i);
    if (it.Lbeg == 1) {
      prefix.assign((size_t)it.len + 1, 0.0);
      for (int e = 0; e < it.len; ++e) prefix[(size_t)e + 1] = prefix[(size_t)e] + (double)T[(size_t)(r.start + e)];
    }
    for (int L = it.Lbeg; L < it.Lend; ++L)
      for (int off = 0; off + L <= it.len; ++off) {
        const double score = fabs((prefix[(size_t)(off + L)] - prefix[(size_t)off]) / (double)L - tmedian2) * sqrt((double)L);
        if (score > best[i].score) best[i] = rsik::BestSeg{score, off, L};
      }
  }
  for (size_t r = 0; r < runs.size(); ++r) {
    bool closed = false;
    for (const rsik::SegItem& it : items) closed = closed || (it.run == (int32_t)r && it.Lend == it.len + 1);
    CHECK(closed, "run %zu: no item reaches its full length", r);
  }
  const std::vector<int> s2(st2.begin(), st2.end());
  std::vector<rsih::Candidate> segs;
  rsih::segments_from_best(runs, items, best.data(), rsih::IntSpan(s2), tlamda2, segs);
  const std::vector<orc_call> segs_o = getc(O, name("").insert(0, "segs_").c_str());
  if (same_calls(segs, segs_o, "segments"))
    for (size_t i = 0; i < segs.size(); ++i)
      CHECK(fabs(segs[i].score - segs_o[i].score) <= 1e-9 * fabs(segs_o[i].score), "segment %zu: score %.17g, oracle %.17g", i, segs[i].score, segs_o[i].score);
  printf("pipeline steps (%s): %zu regions, n' %lld, Lmax %d, level choice %d..%d trim %d, %zu runs in %zu items -> %zu segments\n", pre, regs.size(),
         (long long)ct.ncompact, su.Lmax, lc.leveldel, lc.leveladd, (int)lc.trim, runs.size(), items.size(), segs.size());
}

// kernels_bin.hip's encoder of the order-preserving key, restated
static uint32_t f32_key(float f) { uint32_t b; memcpy(&b, &f, 4); return (b & 0x80000000u) ? ~b : (b | 0x80000000u); }

// Hand-made inputs for what a synthetic chromosome does not reach.
static void pipeline_step_edges() {
  using rsih::Region;
  {   // boundary lists
    std::vector<Region> out = {{1, 2}};
    CHECK(rsih::boundary_pairs(nullptr, 0, true, out) && out.empty(), "empty boundary list");
    const uint64_t one[2] = {(9u << 1) | 1, 5u << 1};
    CHECK(rsih::boundary_pairs(one, 2, true, out) && out.size() == 1 && out[0].start == 5 && out[0].end == 8, "one run, exclusive end");
    CHECK(rsih::boundary_pairs(one, 2, false, out) && out.size() == 1 && out[0].start == 5 && out[0].end == 9, "one run, inclusive end");
    const uint64_t odd[3] = {5u << 1, (9u << 1) | 1, 20u << 1};
    CHECK(!rsih::boundary_pairs(odd, 3, true, out), "unbalanced boundary list");
  }
  {   // region merge: padded by 50, [100, 110] ends at 160
    auto regions = [](std::vector<Region> runs) { return rsih::noncode_regions(runs, 1000, 50); };
    std::vector<Region> r = regions({{100, 110}, {211, 220}});   // 211 - 50 == 160 + 1: touch
    CHECK(r.size() == 1 && r[0].start == 50 && r[0].end == 270, "padded regions that touch merge");
    r = regions({{100, 110}, {212, 220}});                       // one base between them
    CHECK(r.size() == 2 && r[0].end == 160 && r[1].start == 162, "padded regions one base apart stay two");
    r = regions({{0, 3}, {990, 999}});
    CHECK(r.size() == 2 && r[0].start == 0 && r[0].end == 53 && r[1].start == 940 && r[1].end == 999, "runs at base 0 and up to n - 1 are clamped");
    const rsih::CompactTable t = rsih::compact_table(r, 1000);
    CHECK(t.ncompact == 1000 - 54 - 60 && t.cbreak[0] == 0 && t.cbreak[1] == 940 - 54 && t.cum.back() == 114, "compaction table of two regions");
    const rsih::CompactTable none = rsih::compact_table({}, 1000);
    CHECK(none.ncompact == 1000 && none.cbreak.empty() && none.cum.size() == 1 && none.cum[0] == 0, "compaction table without regions");
    CHECK(rsih::compact_table(regions({{0, 999}}), 1000).ncompact == 0, "a chromosome of N only compacts to nothing");
  }
  {   // cap
    rsik::ValueMedian vm{1000, 3, 90, 30, 0};
    CHECK(rsih::cap_median(vm, 1000).med == 30.0 && !rsih::cap_median(vm, 1000).beyond, "cap median from the device's walk");
    vm.hi = 3;
    CHECK(rsih::cap_median(vm, 1000).med == 3.0, "one value only: the minimum");
    vm.inrange = 499;
    CHECK(rsih::cap_median(vm, 1000).beyond && !rsih::cap_median(vm, 999).beyond, "the median lies beyond the histogram");
    CHECK(rsih::cap_value(30.0, 4.0) == 120 && rsih::cap_value(30.0, 63.5 / 30) == 63, "cap value, truncated");
  }
  {   // order key
    std::mt19937_64 rng(11);
    std::vector<float> xs = {0.0f, -0.0f, 1.4e-45f, -1.4e-45f, 1.1e-38f, -1.1e-38f, 3.402823466e38f, -3.402823466e38f, 1.0f, -1.0f};
    for (int k = 0; k < 1000; ++k) { uint32_t b = (uint32_t)rng(); if ((b & 0x7f800000u) == 0x7f800000u) b &= ~0x00800000u; float f; memcpy(&f, &b, 4); xs.push_back(f); }
    for (float x : xs) {
      const float y = rsih::unkey_f32(f32_key(x));
      CHECK(memcmp(&x, &y, 4) == 0, "order key does not give %.9g back", x);
    }
    for (size_t i = 0; i + 1 < xs.size(); ++i) if (xs[i] < xs[i + 1]) CHECK(f32_key(xs[i]) < f32_key(xs[i + 1]), "order key does not keep the order of %.9g and %.9g", xs[i], xs[i + 1]);
  }
  {   // level choice
    std::vector<float> wsum(7, 0.0f);
    std::vector<int> wcnt(7, 0);
    wsum[3] = 50.0f; wcnt[3] = 10;   // Lmax 3: only level 0
    rsih::LevelChoice c = rsih::choose_levels(wsum, wcnt, 3, 3.0);
    CHECK(c.has_level0 && c.lo == 0 && c.hi == 0 && c.m0 == 5.0f && c.leveldel == 0 && c.leveladd == 0 && c.trim && c.lines.size() == 3 &&
          c.lines[0] == "0\t10\t5" && c.lines[1] == "0\t5", "only level 0 populated");
    wsum[3] = 100.0f; wsum[4] = 8.0f; wcnt[4] = 4;   // level +1 lies BELOW level 0: the DEL level comes out positive
    c = rsih::choose_levels(wsum, wcnt, 3, 3.0);
    CHECK(c.has_level0 && c.leveldel == 1 && !c.trim && c.lines.back() == "warning level error, status not filtered", "level error");
    wsum[3] = 0.0f; wcnt[3] = 0;   // no unmarked bin
    CHECK(!rsih::choose_levels(wsum, wcnt, 3, 3.0).has_level0, "no level 0");
  }
  {   // scan parameters
    rsih::ScanSetup s = rsih::scan_first_pass(false, 20.0, 0.6745, 5.0, 99, 10.0f, 20.0f, -1.0, 1000);
    CHECK(s.tsigma == 1.0 && s.target == 10.0 * sqrt(2.5) && s.tlamda == s.target && s.cal_max == 9 && s.Lmax_ref == 99 && s.Lmax == 99 && !s.clipped && s.dev == 3.0,
          "cal_max below LmaxBase: tlamda %.17g cal_max %d Lmax %d", s.tlamda, s.cal_max, s.Lmax);
    s = rsih::scan_first_pass(false, 20.0, 0.6745, 5.0, 99, 10.0f, 20.0f, -1.0, 50);
    CHECK(s.clipped && s.Lmax == 50 && s.Lmax_ref == 99, "more lengths than bins");
    s = rsih::scan_first_pass(true, 30.0, 2.0, 6.6, 20, 0.0f, 0.0f, 0.5, 1000);
    CHECK(s.tlamda == 30.0 * 0.5 && s.target == 30.0 * sqrt(2.0) && s.tsigma == 2.0 / 0.6745 && s.cal_max == 3 && s.Lmax == 20 && s.dev == 30.0 * 0.6, "-threshold in the median branch");
    s = rsih::scan_first_pass(true, 30.0, 2.0, 6.6, 20, 0.0f, 0.0f, -1.0, 1000);
    const rsih::Lamda l = rsih::lamda_from_mad(2.0, 6.6, 30.0 * sqrt(2.0));
    CHECK(s.tlamda == l.tlamda && s.tsigma == l.tsigma && l.tlamda == 30.0 * sqrt(2.0), "the second pass' update is the first pass' rule");
  }
  {   // pairs per work item of the segment search, by hand: len (len + 1) / 2 pairs a run, 150 - 2 runs items of room (8 at least)
    auto one = [](int s, int e) { return std::vector<Region>{Region{s, e}}; };
    CHECK(rsih::segment_pairs_per_item(one(0, 99), false) == 65536 && rsih::segment_pairs_per_item(one(0, 8191), false) == 65536, "a shared chip: 65 536 pairs");
    CHECK(rsih::segment_pairs_per_item(one(0, 99), true) == 8192, "5050 pairs over 148 items: the floor of 8192");
    CHECK(rsih::segment_pairs_per_item(one(10, 2009), true) == 13521, "2 001 000 pairs over 148 items: 13 520 and a fraction, + 1");
    CHECK(rsih::segment_pairs_per_item(one(0, 8191), true) == 65536, "33 558 528 pairs over 148 items: the ceiling of 65 536");
    std::vector<Region> many;
    for (int k = 0; k < 80; ++k) many.push_back(Region{100 * k, 100 * k + 39});
    CHECK(rsih::segment_pairs_per_item(many, true) == 8201, "80 runs of 40 bins: 65 600 pairs over the 8 items of room left, + 1");
    CHECK(rsih::segment_pairs_per_item(std::vector<Region>(), true) == 8192, "no runs");
  }
  {   // scan record: 100 bins, the 20 % rule by one bin
    const int Lmax = 4, stride = rsik::scan_level_stride(Lmax);
    std::vector<uint32_t> w((size_t)(rsik::kScanRecLevels + 2 * stride), 0u);
    w[rsik::kScanRecEscapes] = 7; w[rsik::kScanRecInexact] = 1; w[rsik::kScanRecStop] = 2; w[rsik::kScanRecStop + 1] = 3; w[rsik::kScanRecTiles] = 5;
    uint32_t* del = w.data() + rsik::kScanRecLevels;
    uint32_t* dup = del + stride;
    del[1] = 10; del[2] = 11; del[3] = 50;   // [3] lies behind the stop level
    dup[1] = 7; dup[2] = 7; dup[3] = 7;
    const rsih::ScanRecord rec{w.data(), Lmax};
    CHECK(rec.escapes() == 7 && rec.inexact() == 1 && rec.stop_level(0) == 2 && rec.stop_level(1) == 3 && rec.tiles_listed() == 5 &&
          rec.level_counts(0) == del && rec.level_counts(1) == dup, "scan record fields");
    CHECK(rec.sweeps_stopped(100), "21 of 100 bins marked in both sweeps");
    del[2] = 10;
    CHECK(!rec.sweeps_stopped(100), "20 of 100 bins is not more than 20 %%");
    del[2] = 11; dup[3] = 6;
    CHECK(!rec.sweeps_stopped(100), "the DUP sweep one bin short");
  }
}

static void bam_checks(const char* path) {
  std::ifstream f(path, std::ios::binary);
  std::vector<char> raw((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  CHECK(!raw.empty(), "cannot read %s", path);
  auto walk = [&](const std::string& p, bool must_work) {
    std::string err;
    rsih::BamFile bam;
    std::vector<std::pair<std::string, int64_t>> refs;
    uint64_t first = 0;
    if (!bam.open(p, err) || !bam.read_header(refs, first, err)) { CHECK(!must_work, "header of %s: %s", p.c_str(), err.c_str()); return; }
    rsih::BamReader rd(bam);
    if (!rd.seek(first, err)) { CHECK(!must_work, "seek: %s", err.c_str()); return; }
    rsih::BamRecord r;
    long n = 0;
    int rc;
    while ((rc = rd.next(r, err)) == 1 && n < 2000000) ++n;
    CHECK(!must_work || (rc == 0 && n > 0), "record walk of %s ended with %d after %ld records: %s", p.c_str(), rc, n, err.c_str());
    for (size_t t = 0; t < refs.size() && t < 3; ++t) {
      rsih::PairSample ps;
      (void)rsih::bam_pair_sample(bam, p + ".bai", (int)t, refs[t].second, 1000, refs[t].second, ps, err);
      std::vector<rsih::CallSpan> calls = {{2000, 9000, 0, -1, -1.0}, {(int)(refs[t].second / 2), (int)(refs[t].second / 2) + 5000, 1, -1, -1.0}};
      (void)rsih::bam_annotate_calls(bam, p + ".bai", (int)t, ps, calls, err);
      uint64_t v = 0;
      (void)rsih::bai_first_offset(p + ".bai", (int)t, v);
    }
  };
  walk(path, true);
  std::mt19937_64 rng(99);
  const std::string tmp = std::string(path) + ".mangled";
  for (int trial = 0; trial < 24; ++trial) {
    std::vector<char> bad = raw;
    if (trial < 6) bad.resize(raw.size() * (size_t)(trial + 1) / 8);           // cut off
    else for (int k = 0; k < 1 + trial; ++k) bad[rng() % bad.size()] ^= (char)(1u << (rng() % 8));   // bit flips
    std::ofstream(tmp, std::ios::binary).write(bad.data(), (std::streamsize)bad.size());
    walk(tmp, false);
  }
  remove(tmp.c_str());
}

// IntSpan's sparse form (the status array inside the marked runs only, as the pipeline hands it to the block tests) against the
// dense array it stands for: every index inside a range, at its ends, between ranges and outside all of them.
static void span_checks() {
  std::vector<int> dense(5000, 0), values;
  std::vector<rsih::IntSpan::Range> ranges;
  const int bounds[][2] = {{0, 0}, {7, 19}, {20, 20}, {100, 1099}, {4990, 4999}};
  int v = 1;
  for (const auto& b : bounds) {
    ranges.push_back({b[0], b[1], (int64_t)values.size()});
    for (int i = b[0]; i <= b[1]; ++i) { dense[(size_t)i] = (v % 7) - 3 ? (v % 7) - 3 : 5; values.push_back(dense[(size_t)i]); ++v; }
  }
  const rsih::IntSpan sparse(values.data(), (int64_t)dense.size(), &ranges), full(dense);
  for (int64_t i = 0; i < (int64_t)dense.size(); ++i) CHECK(sparse[i] == full[i], "sparse span differs from the dense array");
  CHECK(sparse.at(100)[999] == dense[1099] && *sparse.at(4999) == dense[4999] && *sparse.at(50) == 0, "sparse span: at()");
}

// rsi_hot_run's narrowed upload (host_calls.cpp: narrow_depth_u8): bytes + list give the int32 array back, value for value --
// depths of 254 / 255 / 256, 32767 / 32768 / 65535 / 65536 (a saturating pack reads 16-bit intermediates as SIGNED: the first
// version turned everything from 32768 on into 0), INT32_MAX, negative ones; every length around the 32-value vector loop; a list
// that is too short reports how many there were.
static void narrow_checks() {
  uint64_t rs = 0x9E3779B97F4A7C15ull;
  auto rnd = [&]() { rs ^= rs << 13; rs ^= rs >> 7; rs ^= rs << 17; return rs; };
  const int32_t odd[] = {254, 255, 256, 300, 32767, 32768, 65535, 65536, 70000, 1 << 24, 2147483647, -1, -2147483647 - 1, 0};
  for (int64_t n : {0, 1, 31, 32, 33, 63, 64, 65, 1000, 700001}) {
    std::vector<int32_t> d((size_t)n);
    for (auto& x : d) x = (int32_t)(rnd() % 90);
    for (int k = 0; k < 14 && n > 0; ++k) d[(size_t)(rnd() % (uint64_t)n)] = odd[k];
    for (int k = 0; k < 200 && n > 1000; ++k) d[(size_t)(rnd() % (uint64_t)n)] = (int32_t)(255 + rnd() % 3000000);
    const int64_t cap = n / 64 + 16;
    std::vector<uint8_t> b((size_t)n + 64, 0xAB);
    std::vector<int32_t> pos((size_t)cap), val((size_t)cap);
    const int64_t ne = rsih::narrow_depth_u8(d.data(), n, b.data(), pos.data(), val.data(), cap);
    int64_t expect = 0;
    for (int32_t x : d) expect += (uint32_t)x >= 255u;
    CHECK(ne == expect, "narrow_depth_u8: %lld escapes reported, %lld present (n = %lld)", (long long)ne, (long long)expect, (long long)n);
    if (ne <= cap) {
      std::vector<int32_t> back((size_t)n);
      for (int64_t i = 0; i < n; ++i) back[(size_t)i] = b[(size_t)i];
      for (int64_t k = 0; k < ne; ++k) { CHECK(pos[(size_t)k] >= 0 && pos[(size_t)k] < n && b[(size_t)pos[(size_t)k]] == 255, "narrow_depth_u8: bad list entry"); back[(size_t)pos[(size_t)k]] = val[(size_t)k]; }
      CHECK(back == d, "narrow_depth_u8: bytes + list do not give the array back (n = %lld)", (long long)n);
    }
    for (int k = 0; k < 64; ++k) CHECK(b[(size_t)n + k] == 0xAB, "narrow_depth_u8 wrote behind the array");
  }
  std::vector<int32_t> deep(4096, 1000), pos(8), val(8);
  std::vector<uint8_t> b(4096 + 64);
  CHECK(rsih::narrow_depth_u8(deep.data(), 4096, b.data(), pos.data(), val.data(), 8) == 4096, "narrow_depth_u8: a list that is too short must report the full count");
}

int main(int argc, char** argv) {
  quantile_checks();
  span_checks();
  narrow_checks();
  pipeline_step_edges();
  orc_params P;
  orc_default_params(&P);
  candidate_stage_case(0x5A11, 400007, 0, P);
  orc_params Q = P; Q.m = 51; Q.trans = 1;
  candidate_stage_case(0x5A12, 350013, 1, Q);
  orc_params R = P; R.merge = 0; R.chklen = 1.5; R.maxchkbp = 2000;
  candidate_stage_case(0x5A13, 300000, 1, R);
  candidate_stage_case(0x5A14, 2000003, 1, P, 1);
  if (argc > 1) bam_checks(argv[1]);
  if (g_fail) { fprintf(stderr, "%d check(s) failed\n", g_fail); return 1; }
  printf("host harness ok\n");
  return 0;
}
