// cli.cpp -- `rsicnv rsi ...`: the reference's command line (rsi.cpp:1949-2068, 2069-2217) in
// front of librsi_hot.so.  Same flags and defaults, same output file (header lines, columns,
// number formatting).  Inputs: a depth file (-d RDFILE -c RNAME, parsed on the device), a whole-genome
// depth file (-d GENOME.depth without -c: "RNAME pos depth" lines, every chromosome in one pass, each run
// as soon as its lines are parsed) or a BAM file (-b BAMFILE [-c RNAME], piled up on the device, calls
// annotated with RP / Q0 from its read pairs); `rsicnv stat` and `rsicnv pin` annotate and sharpen a CNV list (-v CNVFILE) from
// a BAM (run_cnvlist); `rsicnv geno` runs the chromosomes such a list names as rsi does and appends every region's copy
// number, reduced on the device from the depth the run leaves there (geno_chromosome); `rsicnv depth` loads every
// chromosome as rsi does and writes its coverage summary, distribution, per-base track and window / region means from HBM, with
// no run (run_depth); `rsicnv view` draws the figures of such a list from the raw depth in HBM (run_view), and
// -plots device takes the numbers of rsi's own figures from there too; `rsicnv plot` is not yet an alias of view and says that it is
// outside the accelerated path.  A whole-genome file with several depth columns (a cohort, RNAME POS D1 ... DK) is
// called sample by sample with -samples all|LIST: one OUT.k per selected column k.  A bedGraph depth file (RNAME START END
// DEPTH: mosdepth, bedtools genomecov -bg / -bga) runs as the per-base file it stands for, whole or one chromosome (-c).
// -track FILE saves the depth every chromosome was called from (raw, or GC-adjusted with -trackdepth gc) as one bedGraph file,
// written by the device (rsi_hot_write_track) chromosome by chromosome into part files that are joined in row order at the end.
// -bintrack FILE saves the signal the calls are made from, one value per bin (its median, or with -bintrackvalue ratio its ratio
// to the chromosome's median), the same way (rsi_hot_write_bin_track).
// -f REFFILE is read by read_fasta's host loop, or -- a BGZF file always, a plain one with -refread device -- by the device reader
// (rsi_ref: the sequence unfolded in HBM, handed to the _dfasta entry points and rsi_hot_run_device without a host copy).
#include <fcntl.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <chrono>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include <atomic>
#include <mutex>
#include <thread>
#include <algorithm>
#include <condition_variable>
#include <deque>
#include <iterator>
#include <memory>
#include <set>
#include <zlib.h>

#include "../../include/rsi_hot.h"
#include "hostmath.h"
#include "track_host.h"
#include "pin_host.h"
#include "geno_host.h"
#include "depth_host.h"

namespace {

struct Options {
  std::string function = "rsi", rdfile, bamfile, reffile, cnvfile, outfile = "rsiout.txt", chr = "1-22XY", plotfolder = "cnv_plots";
  rsi_params P;
  int minq = 0, min_baseQ = 13, device = 0;
  int gpus = 0;      // -gpus N: chromosomes spread over N devices, several in flight per device (0: one context, one at a time)
  int workers = 4;   // -workers W: chromosomes in flight per device with -gpus, and on -gpu for a whole-genome depth file
  bool saverd = false, plot = true, plotfiles = false;
  std::string plots = "host";   // -plots device|host: the figures' numbers from the depth in HBM (rsi_hot_plot_run), or from a host copy of it
  std::string samples;   // -samples all|k1,k2,...: the depth columns of a cohort file to call (without: the first one, as always)
  bool samples_given = false, chr_given = false;
  std::string dformat;   // -dformat depth|bedgraph: the -d file's format (without: from its name, is_bedgraph_name)
  std::string excludefile;   // -x FILE: BED file of regions left out of calling, treated as N of the reference
  std::string trackfile;     // -track FILE: the depth of every called chromosome as bedGraph (with -samples: FILE.k per column k)
  std::string trackdepth = "raw";   // -trackdepth raw|gc: the depth as read, or after the GC adjustment
  std::string bintrackfile;  // -bintrack FILE: one value per bin of every called chromosome as bedGraph (with -samples: FILE.k per column k)
  std::string bintrackvalue = "ratio";   // -bintrackvalue ratio|median: the bin's median over the chromosome's, or the median itself
  std::string trackformat;   // -trackformat text|bgzf: both tracks as text or as BGZF, whatever their names (empty: by the name)
  bool track_bgzf = false, bintrack_bgzf = false;   // what the rule gives -track's and -bintrack's FILE (main sets them)
  std::string dindex;        // -dindex PATH|none: the .tbi / .csi of a BGZF bedGraph -d FILE for -c RNAME (empty: FILE.tbi, else FILE.csi, when there)
  std::string dindex_path;   // what that gives (main sets it); empty: the whole file is read
  bool trackindex = false;   // -trackindex: FILE.tbi beside every track that is BGZF, built from the device's records
  std::string pairs;         // -pairs device|host: RP / Q0 from the pair table the BAM load keeps on the GPU (rsi_hot_set_bam_pairs), or from a second pass over the file on the host (empty: host)
  std::string bamread;       // -bamread device|host: the BAM's records inflated and found on the GPU (rsi_hot_set_bam_read), or by the host threads (empty: host)
  std::string refread;       // -refread device|host: the reference through the device reader (rsi_ref) or read_fasta (empty: host for text, device for BGZF)
  std::string refindex;      // -refindex PATH|none: the .gzi of a BGZF reference (empty: REFFILE.gzi when there, else the members are walked)
  bool ref_device = false;   // what that gives (main sets it)
  std::string by;            // -by W | REGIONS.bed (depth): mean depth per window of W bases, or per line of a BED file
  bool nobase = false;       // -nobase (depth): no PREFIX.per-base.bed.gz
  bool out_given = false;    // -o was given (depth has no default prefix)
  double ploidy = 2.0;       // -ploidy P (geno): CN = P x the body's median over the chromosome's
  const std::vector<rsipinh::CnvLine>* geno = nullptr;   // `rsicnv geno`: the lines of -v CNVFILE (main sets it); every chromosome's run then
                                                         // ends in geno_chromosome instead of rows and plots
};

// `rsicnv geno`: a list names a chromosome as the reference's index does, with or without a leading "chr"
bool same_chrom(const std::string& a, const std::string& b) { return a == b || "chr" + a == b || a == "chr" + b; }
bool geno_names(const std::vector<rsipinh::CnvLine>& lines, const std::string& chr) {
  for (const rsipinh::CnvLine& l : lines) if (same_chrom(l.cell[0], chr)) return true;
  return false;
}
struct GenoRow { size_t line; std::string field, cn; };   // what a line gets: the appended field, and its CN alone for OUT.matrix

// The reference through the device reader: one rsi_ref per device, shared by that device's workers (a handle loads
// one sequence at a time), and what all of a run's loads read, for the log's one "#reference:" line.
struct RefTotals {
  std::mutex mu;
  int64_t loads = 0, bytes = 0, text = 0, members = 0;
  double kernel_ms = 0, wall_ms = 0;
};
struct RefReader {
  rsi_ref* ref = nullptr;
  int device = 0;
  RefTotals* totals = nullptr;
  // Sequence buffers handed back by release(), kept for the next chromosome: a device allocation or free per chromosome would
  // synchronise the device under the workers' feet.  At most as many exist as sequences were ever held at once.
  std::mutex pool_mu;
  std::vector<std::pair<void*, int64_t>> spare, lent;   // (buffer, its bytes)
  ~RefReader() {
    for (auto& b : spare) rsi_ref_device_free(device, b.first);
    for (auto& b : lent) rsi_ref_device_free(device, b.first);
    rsi_ref_close(ref);
  }
  void* take(int64_t bytes) {
    std::lock_guard<std::mutex> lk(pool_mu);
    size_t best = spare.size();   // the smallest spare buffer that is large enough
    for (size_t k = 0; k < spare.size(); ++k) if (spare[k].second >= bytes && (best == spare.size() || spare[k].second < spare[best].second)) best = k;
    if (best < spare.size()) { lent.push_back(spare[best]); spare.erase(spare.begin() + (ptrdiff_t)best); return lent.back().first; }
    if (!spare.empty()) {   // none fits: the largest of them makes room for the new one
      size_t big = 0;
      for (size_t k = 1; k < spare.size(); ++k) if (spare[k].second > spare[big].second) big = k;
      rsi_ref_device_free(device, spare[big].first);
      spare.erase(spare.begin() + (ptrdiff_t)big);
    }
    void* p = rsi_ref_device_alloc(device, bytes);
    if (p) lent.emplace_back(p, bytes);
    return p;
  }
  bool open(const Options& o, int dev, RefTotals* t, std::string& err) {
    device = dev; totals = t;
    const char* gzi = o.refindex.empty() ? nullptr : o.refindex.c_str();
    if (rsi_ref_open(o.reffile.c_str(), nullptr, gzi, &ref) == RSI_OK) return true;
    err = rsi_ref_last_error(nullptr);
    return false;
  }
  // The sequence read_fasta would take for `chr`, unfolded into a device buffer of its own (release() frees it); false: err says why
  // (missing: no such sequence, which read_fasta tells stderr alone)
  bool load(const std::string& chr, void*& d_fasta, int64_t& n, std::string& err, bool* missing = nullptr) {
    d_fasta = nullptr;
    const int i = rsi_ref_find(ref, chr.c_str());
    if (missing) *missing = i < 0;
    if (i < 0) { err = chr + " not found in fai index"; return false; }
    rsi_ref_seq s;
    rsi_ref_sequence(ref, i, &s);
    n = s.length;
    d_fasta = take(n + 64);
    if (!d_fasta) { err = "out of device memory for the sequence of " + chr; return false; }
    rsi_ref_stats st;
    if (rsi_ref_load_device(ref, device, i, d_fasta, n + 64, nullptr, &st) != RSI_OK) {
      err = rsi_ref_last_error(ref);
      release(d_fasta);
      d_fasta = nullptr;
      return false;
    }
    std::lock_guard<std::mutex> lk(totals->mu);
    ++totals->loads; totals->bytes += st.bytes_read; totals->text += st.text_bytes; totals->members += st.members;
    totals->kernel_ms += st.t_kernel_ms; totals->wall_ms += st.t_wall_ms;
    return true;
  }
  void release(void* d_fasta) {
    std::lock_guard<std::mutex> lk(pool_mu);
    for (size_t k = 0; k < lent.size(); ++k) if (lent[k].first == d_fasta) { spare.push_back(lent[k]); lent.erase(lent.begin() + (ptrdiff_t)k); return; }
  }
  // in the style of inflate_line
  std::string line() const {
    std::ostringstream o;
    const bool bgzf = rsi_ref_format(ref) == 1;
    const std::string gzi = rsi_ref_index_path(ref);
    std::lock_guard<std::mutex> lk(totals->mu);
    o << "#reference: " << (bgzf ? "BGZF" : "text");
    if (bgzf) o << ", " << (gzi.empty() ? std::string("members walked") : "index " + gzi);
    o << ", " << totals->loads << " sequences, " << totals->bytes << (bgzf ? " compressed bytes read, " : " bytes read, ");
    if (bgzf) o << totals->text << " text bytes, " << totals->members << " members inflated, ";
    o << "kernels " << totals->kernel_ms << " ms, loads " << totals->wall_ms << " ms (device)\n";
    return o.str();
  }
};

int usage() {
  std::cerr << "Usage:\n\n1. detect CNV\n\n"
            << "   rsicnv rsi <options> [-b BAMFILE | -d RDFILE -c RNAME ] -f REFFILE \n"
            << "   rsicnv rsi <options> -d GENOME.depth -f REFFILE      (every chromosome of a whole-genome depth file)\n"
            << "\n2. annotate or sharpen a list of CNVs (RNAME START END TYPE ... per line; TYPE holds del / loss or dup / gain / add)\n\n"
            << "   rsicnv stat <options> -b BAMFILE -v CNVFILE -o OUT   every line with RP=#support_read_pairs;Q0=#fraction_of_Q0_reads appended\n"
            << "   rsicnv pin  <options> -b BAMFILE -v CNVFILE -o OUT   RNAME START END moved to where clipped reads pile up and the depth\n"
            << "             steps, the line's other fields, SC=#clipped_reads_at_START;#clipped_reads_at_END; calls below 800 bases and\n"
            << "             of unknown type stay.  Both take -m, -gpu and -bamread, read each chromosome of the list once (no .bai) and\n"
            << "             count on the GPU; lines of a chromosome the BAM does not name, or pin cannot sample from 10 Mb on, are\n"
            << "             written unchanged and OUT.log says why\n"
            << "\n3. copy number of a list of regions (the same lines), per sample\n\n"
            << "   rsicnv geno <options> -f REFFILE (-d DEPTH [-c RNAME] | -b BAMFILE [-c RNAME]) -v CNVFILE -o OUT [-ploidy P]\n"
            << "             runs the chromosomes the list names as rsi does (-m -cap -NOGC -x -q -Q -refread -bamread -dformat -dindex\n"
            << "             -workers as there), writes no calls and no plots, and appends to every line\n"
            << "             CN=;RATIO=;MED=;FLANK=;CHR=;N= -- N kept bases between START and END, MED their median depth (GC-adjusted,\n"
            << "             capped), RATIO = MED over the chromosome's median CHR, CN = RATIO x P (default 2), FLANK the median of\n"
            << "             max(N, m) kept bases on each side; computed on the GPU from the depth the run leaves there.  With -samples\n"
            << "             OUT.k per column k and OUT.matrix (one CN per sample and line).  Lines of a chromosome the input lacks or\n"
            << "             whose run fails are written unchanged and OUT.log says why\n"
            << "\n4. coverage of a sample before calling: summary, distribution, per-base depth, windows or regions\n\n"
            << "   rsicnv depth (-b BAMFILE | -f REFFILE -d DEPTH) [-c RNAME] -o PREFIX [-by W | -by REGIONS.bed] [-nobase]\n"
            << "             the chromosomes rsi would process (-q -Q -bamread -dformat -dindex -gpu as there; of -f only the .fai is read),\n"
            << "             each loaded once and summed on the GPU, no calling run: PREFIX.mosdepth.summary.txt (length, bases, mean,\n"
            << "             min, max per chromosome and in total), PREFIX.mosdepth.global.dist.txt (share of bases at least d deep, d\n"
            << "             from the maximum, at most 65535, down to 0), PREFIX.per-base.bed.gz (one line per run of equal depth,\n"
            << "             BGZF; -trackindex adds its .tbi, -nobase leaves it out) and with -by PREFIX.regions.bed.gz: the mean depth\n"
            << "             of every window of W bases, or of every line of a BED file in the file's order (names with or without\n"
            << "             chr, lines clipped to the chromosome).  -trackformat text writes both tracks as plain text, without .gz.\n"
            << "             The files are laid out as mosdepth's; the depth is this program's pileup (M and = bases of base quality\n"
            << "             -Q or more), not mosdepth's read spans.  Means and shares have two decimals, rounded half up.\n"
            << "             -d PREFIX.per-base.bed.gz reads the per-base file back\n"
            << "\n5. the figures of a list of CNVs that exists already (this program's rows, pin's output, a published set)\n\n"
            << "   rsicnv view -f REFFILE (-d RDFILE -c RNAME | -b BAMFILE [-c RNAME]) -v CNVFILE [-p FOLDER] [-m INT] [-plotfiles]\n"
            << "             what the reference's plot does: raw depth, no GC adjustment, no cap, nothing removed (-q -Q -bamread -gpu as for\n"
            << "             rsi; -f is needed with -d only, for the .fai).  Every chromosome the list names is loaded once, the numbers of\n"
            << "             its lines' figures come from the GPU, and FOLDER/rsi_RNAME_START_END_TYPE.ps is drawn by gnuplot (-plotfiles:\n"
            << "             the .dat and .gp files are written and kept, gnuplot or not).  Names match with or without chr; files and\n"
            << "             titles carry the input's name.  A line on a chromosome the input lacks, or whose call the writer refuses, gets\n"
            << "             a line in FOLDER/view.log and no file.  A BAM's figures are those of its depth file (the reference's pile up\n"
            << "             where windows overlap, and lack the chromosome's median line), and -p names the folder with -b too.\n"
            << "             rsicnv plot is not this command yet: it still answers that it is not part of the accelerated path\n"
            << "\nOptions:\n"
            << "   -m   INT  bin size, default=101\n"
            << "   -q   INT  minimum mapping quality, default=0\n"
            << "   -Q   INT  minimum base quality, default=10\n"
            << "   -cap INT  cap read depth at INT*median, dafault=4\n"
            << "             if INT<0, do not cap read depth\n"
            << "   -NOGC     do not adjust GC content, default=adjust\n"
            << "   -MED      only use median transformation \n"
            << "   -NB       only use negative binomial transformation (default)\n"
            << "   -o   STR  output file, default=rsiout.txt \n"
            << "   -np       do not plot CNV\n"
            << "   -p   STR  folder of the plots, default=cnv_plots\n"
            << "   -plotfiles  write and keep every call's gnuplot data and script file, with or without a gnuplot\n"
            << "   -plots device|host  the numbers of the plots from the depth on the GPU (about 20 bytes per plotted point cross PCIe), or\n"
            << "             from a host copy of the whole chromosome's depth (default: host); the files are the same\n"
            << "   -gpu INT  HIP device to run on, default=0\n"
            << "   -gpus INT spread the chromosomes of a BAM over INT devices (longest first), several in flight per\n"
            << "             device (-workers INT, default=4); rows are written in BAM header order all the same\n"
            << "   -workers INT chromosomes in flight (with -gpus; and on -gpu for a whole-genome depth file), default=4\n"
            << "   -samples all|k1,k2,... call depth columns k of RNAME POS D1 ... DK (1-based, at most 64) as samples: OUT.k each\n"
            << "   -dformat depth|bedgraph  read -d as per-base lines or as bedGraph (default: from the file name, see below)\n"
            << "   -x   FILE exclude the regions of a BED file (plain or gzip) from calling, see below\n"
            << "   -track FILE  save the depth of every called chromosome as bedGraph (bedtools genomecov -bga), see below\n"
            << "   -trackdepth raw|gc  the depth -track saves: as read (default), or GC-adjusted (what the calls are made from)\n"
            << "   -bintrack FILE  save one value per bin of every called chromosome as bedGraph, see below\n"
            << "   -bintrackvalue ratio|median  the value -bintrack saves: the bin's median over the chromosome's (default), or the median\n"
            << "   -trackformat text|bgzf  -track and -bintrack as plain text or as BGZF (default: BGZF when FILE ends in .gz or .bgz)\n"
            << "   -trackindex  write the tabix index FILE.tbi beside every BGZF track, see below\n"
            << "   -dindex PATH|none  the tabix / CSI index of a BGZF bedGraph -d FILE, used with -c RNAME (default: FILE.tbi, else FILE.csi)\n"
            << "   -bamread device|host  with -b: inflate the BAM's BGZF blocks and find its records on the GPU, or on host threads (default: host)\n"
            << "   -pairs device|host  with -b: RP / Q0 from the reads the BAM load keeps on the GPU, or from a second pass over the file on the host (default: host)\n"
            << "   -refread device|host  read REFFILE on the GPU, or with the host loop (default: host for plain text, device for BGZF), see below\n"
            << "   -refindex PATH|none  the .gzi of a BGZF REFFILE (default: REFFILE.gzi when there; none: the members are walked)\n"
            << "\nNote:\n"
            << "   This build runs the read-depth hot path on an MI355X; input is a read depth file\n"
            << "   (samtools mpileup BAM | cut -f2,4) with -c RNAME, a whole-genome depth file without -c\n"
            << "   (samtools depth -a BAM, or samtools mpileup BAM | cut -f1,2,4: RNAME POS DEPTH, each\n"
            << "   chromosome's lines together; rows follow the file's order), or a coordinate-sorted BAM file\n"
            << "   (all chromosomes with reads, or the one named with -c), plus the indexed reference.\n"
            << "   -s saves the BAM's depth to OUT.RNAME_rd.\n"
            << "   A depth file may be BGZF (bgzip; inflated on the GPU) or gzip (inflated on the host): the format is\n"
            << "   read from the file's first bytes (1f 8b 08 with a BC extra subfield: BGZF; other 1f 8b: gzip; else text).\n"
            << "   A depth file whose name ends in .bed, .bedgraph or .bg (case-insensitive; then optionally .gz or .bgz), or\n"
            << "   any -d file with -dformat bedgraph, is bedGraph: RNAME START END DEPTH, 0-based half-open runs (mosdepth\n"
            << "   per-base.bed.gz, bedtools genomecov -bg / -bga; track and browser lines skipped), read as the per-base\n"
            << "   lines RNAME POS DEPTH, POS = START+1 .. END, that it stands for.  Without -c every chromosome is called;\n"
            << "   -c RNAME calls that chromosome's lines alone.\n"
            << "   -x FILE: the bases of the BED file's intervals (CHROM START END, 0-based half-open, tabs or blanks, any order,\n"
            << "   overlaps allowed; #, track, browser and empty lines skipped; any other malformed line is an error) are\n"
            << "   treated as N of the reference: not GC, padded by max(50, m/4) and merged like N runs, removed before binning.\n"
            << "   Names match with or without a leading chr; names of no processed chromosome are ignored.  Works with every\n"
            << "   input (-d with -c, whole-genome -d, -samples, bedGraph, -b, -gpus).  A mask adds to the chromosome's N regions,\n"
            << "   so their limits apply: above 128 merged regions the general compaction kernel runs instead of the streaming\n"
            << "   one, above 512 runs the regions are built on the host, above 4096 merged regions the chromosome is refused.\n"
            << "   -track FILE: one line RNAME START END DEPTH per run of equal depth (0-based half-open, zero runs included), the\n"
            << "   chromosomes in the order of the output rows; run-length encoded and formatted on the GPU.  Genome browsers and\n"
            << "   bedtools read it, and so does -d FILE (name it .bedgraph, or -dformat bedgraph).  Works with every input but -gpus\n"
            << "   above 1; with -samples it writes FILE.k per column k.  The depth of bases excluded with -x is saved unchanged.\n"
            << "   -trackdepth gc saves the depth after the GC adjustment, before the cap (not with -NOGC).\n"
            << "   -bintrack FILE: one line RNAME START END VALUE per bin of -m kept bases (0-based half-open), the signal the calls\n"
            << "   are made from: the bin's median over the chromosome's median with three decimals (a DUP is a plateau at 1.5), or\n"
            << "   with -bintrackvalue median the bin's median itself.  A bin is cut where N or -x regions lie inside it, so no line\n"
            << "   covers a removed base; the bases behind the last whole bin get no line.  Chromosomes in the order of the output\n"
            << "   rows; formatted on the GPU.  Works with every input but -gpus above 1, and beside -track; with -samples it writes\n"
            << "   FILE.k per column k.\n"
            << "   A track whose FILE ends in .gz or .bgz (in any case; with -samples the FILE given, not FILE.k) is written as BGZF,\n"
            << "   what bgzip makes of the text: the text is deflated on the GPU in members of 65280 bytes and the file ends with the\n"
            << "   end-of-file block, so tabix, IGV and bedtools take it and -d FILE.bedgraph.gz reads it back.  -trackformat text or\n"
            << "   bgzf decides for both tracks whatever their names.\n"
            << "   -d FILE.bed.gz -c RNAME with FILE.tbi or FILE.csi beside a BGZF FILE (tabix's, mosdepth's or -trackindex's; -dindex PATH\n"
            << "   names another, -dindex none reads without) inflates RNAME's members alone instead of the whole file.  An index that\n"
            << "   does not fit the file is an error, never wrong depth; one older than the file gets a warning.\n"
            << "   -trackindex writes FILE.tbi beside every BGZF track (with -samples: FILE.k.tbi): the index tabix -p bed would make,\n"
            << "   collected on the GPU while the track is written, so that IGV and tabix FILE chr7:1-2000000 take the file as it\n"
            << "   is.  Chromosomes longer than 2^29 bases are beyond that format; a plain-text track has no index.\n"
            << "   -f REFFILE may be BGZF (bgzip REFFILE; samtools faidx gives REFFILE.fai, bgzip -i or -r REFFILE.gzi), told from its\n"
            << "   first bytes, not its name: the members that hold a chromosome's lines are found through the .gzi (without one the\n"
            << "   members' sizes are walked once), inflated on the GPU, and the lines are unfolded there by the .fai's arithmetic.\n"
            << "   -refread device reads a plain-text REFFILE the same way; -refread host keeps the host loop (plain text only).\n"
            << "   Works with every input and option.  An index that does not fit the file is an error, never a wrong sequence; a\n"
            << "   plain-gzip REFFILE is refused: recompress it with bgzip.\n"
            << std::endl;
  return 0;
}

// get_parameters, rsi.cpp:1986-2068
void parse(int argc, char** argv, Options& o) {
  rsi_default_params(&o.P);
  std::vector<std::string> a(argv, argv + argc);
  if (a.size() < 2) exit(usage());
  size_t i = 1;
  if (a[1][0] != '-') {
    o.function = a[1];
    if (o.function != "rsi" && o.function != "plot" && o.function != "stat" && o.function != "pin" && o.function != "geno" && o.function != "depth" && o.function != "view") {
      std::cerr << "no such function " << o.function << std::endl;
      exit(usage());
    }
    i = 2;
  }
  auto need = [&](size_t k) { if (k + 1 >= a.size()) exit(usage()); return a[k + 1]; };
  for (; i < a.size(); ++i) {
    const std::string& s = a[i];
    if (s == "-d") { o.rdfile = need(i); ++i; }
    else if (s == "-b") { o.bamfile = need(i); ++i; }
    else if (s == "-f") { o.reffile = need(i); ++i; }
    else if (s == "-v") { o.cnvfile = need(i); ++i; }
    else if (s == "-o") { o.outfile = need(i); o.out_given = true; ++i; }
    else if (s == "-c") { o.chr = need(i); o.chr_given = true; ++i; }
    else if (s == "-s") o.saverd = true;
    else if (s == "-m") { o.P.m = atoi(need(i).c_str()); ++i; }
    else if (s == "-q") { o.minq = atoi(need(i).c_str()); ++i; }
    else if (s == "-Q") { o.min_baseQ = atoi(need(i).c_str()); ++i; }
    else if (s == "-L") { need(i); ++i; }
    else if (s == "-p") { o.plotfolder = need(i); ++i; }
    else if (s == "-np") o.plot = false;
    else if (s == "-plotfiles") o.plotfiles = true;
    else if (s == "-plots") { o.plots = need(i); ++i; }
    else if (s == "-threshold") { o.P.threshold = atof(need(i).c_str()); ++i; }
    else if (s == "-e") { o.P.epsilon = atof(need(i).c_str()); ++i; }
    else if (s == "-cap") { o.P.cap = atof(need(i).c_str()); ++i; }
    else if (s == "-reflen") { o.P.chklen = atof(need(i).c_str()); ++i; }
    else if (s == "-maxchkbp") { o.P.maxchkbp = atoi(need(i).c_str()); ++i; }
    else if (s == "-debug") o.P.debug = 1;
    else if (s == "-MED") o.P.trans = 1;
    else if (s == "-NB") o.P.trans = 0;
    else if (s == "-ALL") o.P.trans = 2;
    else if (s == "-nomerge") o.P.merge = 0;
    else if (s == "-hist" || s == "-overlap" || s == "-combine" || s == "-nocode") {}
    else if (s == "-NOGC") o.P.gcadjust = 0;
    else if (s == "-gpu") { o.device = atoi(need(i).c_str()); ++i; }
    else if (s == "-gpus") { o.gpus = atoi(need(i).c_str()); ++i; }
    else if (s == "-workers") { o.workers = atoi(need(i).c_str()); ++i; }
    else if (s == "-samples") { o.samples = need(i); o.samples_given = true; ++i; }
    else if (s == "-dformat") { o.dformat = need(i); ++i; }
    else if (s == "-x") { o.excludefile = need(i); ++i; }
    else if (s == "-track") { o.trackfile = need(i); ++i; }
    else if (s == "-trackdepth") { o.trackdepth = need(i); ++i; }
    else if (s == "-bintrack") { o.bintrackfile = need(i); ++i; }
    else if (s == "-bintrackvalue") { o.bintrackvalue = need(i); ++i; }
    else if (s == "-trackformat") { o.trackformat = need(i); ++i; }
    else if (s == "-trackindex") o.trackindex = true;
    else if (s == "-dindex") { o.dindex = need(i); ++i; }
    else if (s == "-refread") { o.refread = need(i); ++i; }
    else if (s == "-bamread") { o.bamread = need(i); ++i; }
    else if (s == "-pairs") { o.pairs = need(i); ++i; }
    else if (s == "-refindex") { o.refindex = need(i); ++i; }
    else if (s == "-ploidy") { o.ploidy = atof(need(i).c_str()); ++i; }
    else if (s == "-by") { o.by = need(i); ++i; }
    else if (s == "-nobase") o.nobase = true;
    else { std::cerr << "unknown option " << s << std::endl; exit(usage()); }
  }
  if (o.rdfile.empty() && o.bamfile.empty()) { std::cerr << "need input file " << std::endl; exit(usage()); }
  if (o.reffile.empty() && (o.function == "rsi" || o.function == "geno" || ((o.function == "depth" || o.function == "view") && o.bamfile.empty()))) { std::cerr << "need reference file " << std::endl; exit(usage()); }
  if (o.outfile == o.bamfile || o.outfile == o.rdfile) { std::cerr << "output file is same as input file " << std::endl; exit(usage()); }
  if (!o.rdfile.empty() && o.chr.empty()) { std::cerr << "readdepth file and chromosome must be specified together" << std::endl; exit(usage()); }
  if ((o.P.m % 2) != 1) { o.P.m += 1; std::cerr << "m is changed to " << o.P.m << std::endl; }   // rsi.cpp:2061-2064
}

// read_fasta, readref.cpp:10-86: one chromosome through the .fai index
bool read_fasta(const std::string& fasta, const std::string& chr, std::string& ref) {
  std::ifstream fai((fasta + ".fai").c_str());
  if (!fai) { std::cerr << "[read_fasta] Index file " << fasta << ".fai not found\n"; return false; }
  std::string name, line;
  long len = 0, offset = 0, nbases = 0, lwidth = 0;
  bool found = false;
  while (std::getline(fai, line)) {
    std::istringstream iss(line);
    iss >> name >> len >> offset >> nbases >> lwidth;
    if (name == chr || name == "chr" + chr) { found = true; break; }
  }
  if (!found) { std::cerr << chr << " not found in fai index\n"; return false; }
  const long flen = len + (len / nbases) * (lwidth - nbases);
  std::vector<char> buf((size_t)flen + 1);
  std::ifstream fin(fasta.c_str(), std::ios::binary);
  fin.seekg(offset, std::ios::beg);
  fin.read(buf.data(), flen);
  const long got = (long)fin.gcount();
  ref.resize((size_t)len);
  long k = 0;
  for (long i = 0; i < got && k < len; ++i) if (buf[i] != '\n') ref[(size_t)k++] = buf[i];
  if (k != len) { std::cerr << "Error reading the reference fasta\nread " << k << " bases\nexpecting " << len << " bases" << std::endl; return false; }
  return true;
}

const char* kHeader =
    "#CHROM\tSTART\tEND\tTYPE\tSCORE\tLENGTH\tCNV_MED(CNV_SD);NEIGHBOR_MED(NEIGHBOR_RUNMEANSD);CHR_MED(CHR_SD)\t"
    "RP=#support_read_pairs;Q0=#fraction_of_Q0_reads\tMETHOD";

double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// What one iteration of the reference's chromosome loop (rsi.cpp:2189-2217) leaves behind: its log lines and its rows.
struct ChromOutput {
  std::string log;                 // everything the iteration prints (stderr + OUT.log), in order
  std::vector<std::string> rows;   // output rows (cnv_format1), without the header
  bool populated = false;          // the chromosome was processed (has reads / could be read): it counts for the header
  bool fatal = false;              // the single-chromosome modes stop here (the reference exits)
  bool bad_input = false;          // the compressed depth file is broken: exit 1, no output file
  size_t track_index = 0;          // -track, -bintrack: the chromosome's place in the order of the rows (set by the caller: names its part files)
  bool track_failed = false;       // -track: its part could not be written (the reason is in the log): no track file
  bool bintrack_failed = false;    // -bintrack: likewise
  std::shared_ptr<rsi_track_index> track_ix, bintrack_ix;   // -trackindex: the index of this chromosome's part (offsets from the part's start)
  std::vector<GenoRow> geno;       // `geno`: what this chromosome's lines get
  bool geno_done = false;          // ... and that they got it
};

std::shared_ptr<rsi_track_index> new_track_index() { return std::shared_ptr<rsi_track_index>(rsi_track_index_create(), rsi_track_index_free); }
// ", index: C chunks, W windows" for the log's track lines
std::string index_counts(const rsi_track_index* ix) {
  int64_t refs = 0, chunks = 0, windows = 0;
  if (!ix || rsi_track_index_counts(ix, &refs, &chunks, &windows) != RSI_OK) return "";
  return ", index: " + std::to_string(chunks) + " chunks, " + std::to_string(windows) + " windows";
}

// One log line for a compressed depth file (none for plain text, whose logs stay as they were)
std::string inflate_line(const rsi_inflate_stats& s) {
  if (s.format == 0) return "";
  std::ostringstream o;
  o << "#depth file: " << (s.format == 1 ? "BGZF" : "gzip") << ", " << s.compressed_bytes << " compressed bytes, " << s.text_bytes
    << " text bytes, inflate " << (s.format == 1 ? s.t_inflate_kernel_ms : s.t_host_inflate_ms) << " ms ("
    << (s.format == 1 ? "device" : "host") << ")" << (s.format == 1 && !s.eof_block ? ", no BGZF EOF block at the end" : "") << "\n";
  return o.str();
}

// The log's line for a BAM load that went through the device reader (-bamread device)
std::string bam_read_line(rsi_ctx* ctx) {
  rsi_bam_read_stats brs;
  if (rsi_hot_last_bam_read_stats(ctx, &brs) != RSI_OK) return "";
  std::ostringstream info;
  info << "#bam: read on the device, " << brs.chunks << " chunks, " << brs.members << " BGZF blocks, " << brs.segments << " segments (" << brs.guessed
       << " guessed right, " << brs.rewalked << " walked again, " << brs.passed << " passed over), upload " << brs.t_upload_ms << " ms, inflate "
       << brs.t_inflate_ms << " ms, record finder " << brs.t_find_ms << " ms\n";
  return info.str();
}

// The chromosomes to process: -c RNAME, or (BAM input, rsi.cpp:2114-2131) every reference of the header that is not a
// mitochondrial / decoy name (and, for `geno`, that its list names).  false: the BAM's header cannot be read (stderr says why).
bool select_chromosomes(const Options& o, std::vector<std::string>& todo, std::vector<int64_t>& todo_len, std::ostream& log) {
  if (!o.bamfile.empty() && (o.chr.empty() || o.chr == "1-22XY")) {
    std::vector<char> names(1 << 20);
    std::vector<int64_t> lens(1 << 16);
    const int nref = rsi_bam_references(o.bamfile.c_str(), names.data(), (int)names.size(), lens.data(), (int)lens.size());
    if (nref < 0) { std::cerr << rsi_hot_last_error(nullptr) << std::endl; return false; }
    std::istringstream iss(names.data());
    std::string nm;
    std::cerr << "#Check bam header for 1-22XY \n"; log << "#Check bam header for 1-22XY \n";
    int k = 0;
    while (std::getline(iss, nm)) {
      const int64_t len = k < (int)lens.size() ? lens[(size_t)k] : 0;
      ++k;
      if (nm.find("MT") != std::string::npos || nm.find(".") != std::string::npos) continue;
      if (o.geno && !geno_names(*o.geno, nm)) continue;   // `geno` runs the chromosomes its list names
      todo.push_back(nm); todo_len.push_back(len);
    }
  } else {
    todo.push_back(o.chr); todo_len.push_back(0);
  }
  return true;
}

void report_chromosome(rsi_ctx* ctx, const Options& o, const std::string& chr, rsi_result* res, const rsi_text_stats* ts,
                       const rsi_bam_stats* bs, double t_fasta, double t_path, std::ostringstream& info, ChromOutput& co);

// What the plot step of rsi and `view` share around the files.  gnuplot_version() (plotcnv.cpp:51-65), once per process: what
// `gnuplot -V` reports, -1 without a gnuplot.
double gnuplot_found() {
  static const double gv = [] {
    double v = -1.0;
    if (FILE* pp = popen("gnuplot -V 2>/dev/null | cut -d' ' -f2", "r")) { char b[64] = {0}; if (fgets(b, sizeof(b), pp) && atof(b) > 0) v = atof(b); pclose(pp); }
    return v;
  }();
  return gv;
}
// a call's script through gnuplot, its two files deleted, as the reference does
void draw_figure(const std::string& dat, const std::string& gp, const std::string& img, std::vector<std::string>& psfiles) {
  (void)!system(("gnuplot < " + gp).c_str());
  remove(dat.c_str());
  remove(gp.c_str());
  psfiles.push_back(img);
}
// plot_cnv's last step (plotcnv.cpp:665-677): with ImageMagick at hand every figure also becomes a .png
void convert_figures(const std::vector<std::string>& psfiles, std::ostream& info) {
  static const bool have_convert = [] {
    bool yes = false;
    if (FILE* pp = popen("convert -version 2>/dev/null | grep Image", "r")) { char b[256]; while (fgets(b, sizeof(b), pp)) if (strstr(b, "ImageMagick")) yes = true; pclose(pp); }
    return yes;
  }();
  if (have_convert) for (const std::string& ps : psfiles) {
    info << "converting: " << ps << "\n";
    (void)!system(("convert -limit thread 1 -limit area 256MB -limit disk 512MB -density 72 -rotate 90 -background white -render -antialias -flatten " +
                   ps + " " + ps.substr(0, ps.size() - 3) + ".png").c_str());
  }
}
void geno_chromosome(rsi_ctx* ctx, const Options& o, const std::string& chr, rsi_result* res, std::ostringstream& info, ChromOutput& co);

// -x FILE: the BED file's intervals on `chr` (n bases) arm the context for the run that follows (the mask is spent by that run);
// one log line.  false: the file could not be read (the message is in the log line).
bool arm_exclude(rsi_ctx* ctx, const Options& o, const std::string& chr, int64_t n, std::ostringstream& info) {
  if (o.excludefile.empty()) return true;
  int k = rsi_exclude_read_bed(o.excludefile.c_str(), chr.c_str(), n, nullptr, nullptr, 0);
  std::vector<int64_t> s((size_t)std::max(k, 1)), e((size_t)std::max(k, 1));
  if (k > 0) k = std::min(k, rsi_exclude_read_bed(o.excludefile.c_str(), chr.c_str(), n, s.data(), e.data(), k));
  if (k < 0 || rsi_hot_set_exclude(ctx, s.data(), e.data(), k) != RSI_OK) {
    info << "#exclude: " << (k < 0 ? rsi_hot_last_error(nullptr) : rsi_hot_last_error(ctx)) << "\n";
    return false;
  }
  int64_t bases = 0;
  for (int i = 0; i < k; ++i) bases += e[(size_t)i] - s[(size_t)i];
  info << "#exclude: " << o.excludefile << ", " << k << " intervals, " << bases << " bases on " << chr << "\n";
  return true;
}

// One chromosome on one context, first half: FASTA, depth (text or BAM, on the device), the hot path; then report_chromosome.
// rr (the device reader, -refread device or a BGZF reference): the sequence is unfolded into a device buffer of this call's and
// the _dfasta entry points take it from there; without it read_fasta's host string is uploaded as always.
void process_chromosome(rsi_ctx* ctx, const Options& o, const std::string& chr, bool many, ChromOutput& co, RefReader* rr = nullptr) {
  const bool from_bam = !o.bamfile.empty();
  std::ostringstream info;
  info << "#processing " << chr << "\n";
  const double t0 = now_s();
  std::string fasta;
  void* d_fasta = nullptr;
  int64_t nref = 0;
  struct Free { RefReader* rr; void*& p; ~Free() { if (rr && p) rr->release(p); } } free_fasta{rr, d_fasta};
  if (rr) {
    std::string err;
    bool missing = false;
    if (!rr->load(chr, d_fasta, nref, err, &missing)) {
      std::cerr << err << "\n";
      if (!missing) info << err << "\n";
      co.log = info.str(); co.fatal = !many; return;
    }
  } else {
    if (!read_fasta(o.reffile, chr, fasta)) { co.log = info.str(); co.fatal = !many; return; }
    nref = (int64_t)fasta.size();
  }
  const double t1 = now_s();
  if (!arm_exclude(ctx, o, chr, nref, info)) { co.log = info.str(); co.fatal = true; return; }

  if (from_bam && !o.bamread.empty() && rsi_hot_set_bam_read(ctx, o.bamread == "device" ? RSI_BAM_READ_DEVICE : RSI_BAM_READ_HOST, 0) != RSI_OK) {
    info << rsi_hot_last_error(ctx) << "\n"; co.log = info.str(); co.fatal = true; return;
  }
  if (from_bam && o.pairs == "device" && rsi_hot_set_bam_pairs(ctx, 1) != RSI_OK) {
    info << rsi_hot_last_error(ctx) << "\n"; co.log = info.str(); co.fatal = true; return;
  }
  rsi_result* res = nullptr;
  rsi_text_stats ts;
  rsi_bam_stats bs;
  memset(&ts, 0, sizeof(ts)); memset(&bs, 0, sizeof(bs));
  // the depth comes from a text file parsed on the device (load_data_from_text's loop, loaddata.cpp:496-517) or from
  // the BAM file's reads, inflated on the host and piled up on the device (load_data_from_bam, loaddata.cpp:277-333)
  const int rc = rr
      ? (from_bam ? rsi_hot_run_bam_dfasta(ctx, &o.P, o.bamfile.c_str(), chr.c_str(), o.minq, o.min_baseQ, d_fasta, nref, &res, &bs)
                  : rsi_hot_run_text_dfasta(ctx, &o.P, o.rdfile.c_str(), d_fasta, nref, &res, &ts))
      : from_bam
      ? rsi_hot_run_bam(ctx, &o.P, o.bamfile.c_str(), chr.c_str(), o.minq, o.min_baseQ, reinterpret_cast<const uint8_t*>(fasta.data()), (int64_t)fasta.size(), &res, &bs)
      : rsi_hot_run_text(ctx, &o.P, o.rdfile.c_str(), reinterpret_cast<const uint8_t*>(fasta.data()), (int64_t)fasta.size(), &res, &ts);
  if (rc != RSI_OK) {   // the reference prints its message and exits with status 0
    info << rsi_hot_last_error(ctx) << "\n";
    co.log = info.str();
    rsi_inflate_stats is;
    if (!from_bam && rsi_hot_last_inflate_stats(ctx, &is) == RSI_OK && is.input_error) co.bad_input = true;
    co.fatal = !(many && from_bam && bs.on_chrom == 0);   // a reference without reads is simply not "populated" (rsi.cpp:2125)
    return;
  }
  const double t2 = now_s();
  if (!from_bam) {
    rsi_inflate_stats is;
    if (rsi_hot_last_inflate_stats(ctx, &is) == RSI_OK) info << inflate_line(is);
  }
  if (from_bam && many && bs.on_chrom == 0) {   // not "populated": the reference does not process it (rsi.cpp:2125)
    info << "no reads on " << chr << "\n";
    co.log = info.str();
    rsi_result_free(res);
    return;
  }
  report_chromosome(ctx, o, chr, res, from_bam ? nullptr : &ts, from_bam ? &bs : nullptr, t1 - t0, t2 - t1, info, co);
}

// `geno` behind a chromosome's run, for every input: its lines' regions reduced on the device (rsi_hot_geno_calls), formatted here.
void geno_chromosome(rsi_ctx* ctx, const Options& o, const std::string& chr, rsi_result* res, std::ostringstream& info, ChromOutput& co) {
  std::vector<size_t> mine;
  std::vector<int32_t> start, end;
  for (size_t i = 0; i < o.geno->size(); ++i)
    if (same_chrom((*o.geno)[i].cell[0], chr)) { mine.push_back(i); start.push_back((*o.geno)[i].start); end.push_back((*o.geno)[i].end); }
  const rsi_chrom_stats* S = rsi_result_stats(res);
  info << "region  : " << chr << ":1-" << S->n_compact << "\nmedian  : " << S->RDmedian << "\nrs::m   : " << o.P.m << "\nrs::cap : " << o.P.cap << "\n";
  std::vector<rsi_geno_record> rec(std::max<size_t>(mine.size(), 1));
  if (rsi_hot_geno_calls(ctx, o.P.m, (int)mine.size(), start.data(), end.data(), rec.data()) != RSI_OK) {
    info << "#geno: " << chr << ": " << rsi_hot_last_error(ctx) << "\n";
    return;
  }
  for (size_t k = 0; k < mine.size(); ++k) {
    const rsi_geno_record& r = rec[k];
    co.geno.push_back(GenoRow{mine[k], rsigeno::format_field(r.n_body, r.n_flank, r.body_q[1], r.flank_q[1], r.chrom_median, o.ploidy),
                              rsigeno::cn_text(r.n_body, r.body_q[1], r.chrom_median, o.ploidy)});
  }
  co.geno_done = true;
  rsi_geno_stats gs;
  memset(&gs, 0, sizeof(gs));
  (void)rsi_hot_last_geno_stats(ctx, &gs);
  info << "#geno: " << chr << ": " << mine.size() << " lines, " << gs.jobs << " jobs, " << gs.tiles << " tiles, " << gs.launches << " launches, " << gs.ms
       << " ms (device)\n";
}

// Second half, shared by every input: a chromosome's result (run on ctx, which still holds it) -> its log block, RP / Q0
// (BAM input), its rows, its plots.  Frees res.
void report_chromosome(rsi_ctx* ctx, const Options& o, const std::string& chr, rsi_result* res, const rsi_text_stats* ts,
                       const rsi_bam_stats* bs, double t_fasta, double t_path, std::ostringstream& info, ChromOutput& co) {
  const bool from_bam = bs != nullptr;
  co.populated = true;
  if (from_bam && o.saverd) {   // -s: write_rd_to_file, loaddata.cpp:340-344, 464-470
    const std::string dump = o.outfile + "." + chr + "_rd";
    std::vector<int32_t> rd((size_t)bs->n);
    rsi_hot_fetch_i32(ctx, "depth_in", rd.data(), bs->n);
    FILE* f = fopen(dump.c_str(), "w");
    if (f) { for (int64_t i = 0; i < bs->n; ++i) fprintf(f, "%lld\t%d\n", (long long)i + 1, rd[(size_t)i]); fclose(f); }
    info << "RD of " << chr << " is saved to " << dump << "\n";
  }
  if (o.geno) {   // `geno`: the list's lines on this chromosome, from the depth the run has left in HBM; no rows, no plots
    geno_chromosome(ctx, o, chr, res, info, co);
    co.log = info.str();
    rsi_result_free(res);
    return;
  }
  if (!o.trackfile.empty()) {   // -track: this chromosome's lines into its part file, from the depth the context still holds
    rsi_track_stats tk;
    const std::string part = rsitrack::part_path(o.trackfile, co.track_index);
    if (o.trackindex && o.track_bgzf) co.track_ix = new_track_index();
    if (rsi_hot_set_track_format(ctx, o.track_bgzf ? RSI_TRACK_BGZF : RSI_TRACK_TEXT) != RSI_OK ||
        rsi_hot_set_track_index(ctx, co.track_ix.get()) != RSI_OK ||
        rsi_hot_write_track(ctx, o.trackdepth == "gc" ? 1 : 0, chr.c_str(), part.c_str(), 0, &tk) != RSI_OK) {
      info << "track: " << chr << ": " << rsi_hot_last_error(ctx) << "\n";
      co.track_failed = true;
    } else {
      info << "track: " << chr << " " << tk.lines << " lines, " << tk.bytes << " bytes, " << tk.t_total_ms * 1e-3 << " s (kernels "
           << tk.t_kernel_ms * 1e-3 << " s, write " << tk.t_write_ms * 1e-3 << " s)" << index_counts(co.track_ix.get()) << "\n";
    }
    (void)rsi_hot_set_track_index(ctx, nullptr);
  }
  if (!o.bintrackfile.empty()) {   // -bintrack: this chromosome's bins into their part file, while the context still holds the run
    rsi_track_stats tk;
    const std::string part = rsitrack::part_path(o.bintrackfile, co.track_index);
    if (o.trackindex && o.bintrack_bgzf) co.bintrack_ix = new_track_index();
    if (rsi_hot_set_track_format(ctx, o.bintrack_bgzf ? RSI_TRACK_BGZF : RSI_TRACK_TEXT) != RSI_OK ||
        rsi_hot_set_track_index(ctx, co.bintrack_ix.get()) != RSI_OK ||
        rsi_hot_write_bin_track(ctx, o.bintrackvalue == "median" ? 0 : 1, chr.c_str(), part.c_str(), 0, &tk) != RSI_OK) {
      info << "bintrack: " << chr << ": " << rsi_hot_last_error(ctx) << "\n";
      co.bintrack_failed = true;
    } else {
      info << "bintrack: " << chr << " " << tk.lines << " lines, " << tk.bytes << " bytes, " << tk.t_total_ms * 1e-3 << " s (kernels "
           << tk.t_kernel_ms * 1e-3 << " s, write " << tk.t_write_ms * 1e-3 << " s)" << index_counts(co.bintrack_ix.get()) << "\n";
    }
    (void)rsi_hot_set_track_index(ctx, nullptr);
  }
  const rsi_chrom_stats* S = rsi_result_stats(res);
  info << "#Noseq regions excluded\n";
  {
    std::vector<int32_t> pairs((size_t)S->n_noncode * 2 + 2);
    const int k = rsi_result_noncode(res, pairs.data(), S->n_noncode);
    for (int i = 0; i < k; ++i) info << chr << "\t" << pairs[2 * i] << "\t" << pairs[2 * i + 1] << "\n";
  }
  if (o.P.gcadjust) info << "RD mean before GC adjust = " << S->gc_rdmean << "\n";
  if (o.P.cap > 1) info << "applying cap " << o.P.cap << " times of mean " << S->cap_median << "\ncap = " << o.P.cap * S->cap_median << "\n";
  info << "region  : " << chr << ":1-" << S->n_compact << "\nmedian  : " << S->RDmedian << "\nrs::m   : " << o.P.m << "\nrs::cap : " << o.P.cap << "\n";
  {   // the scan's diagnostic lines as the reference logs them: the NB transform's median / MAD (rsi.cpp:1140-1141), the per-L
      // lines of the two rsistatus passes (rsi.cpp:1221-1224, 1251-1254), filterstatus' level table between them (rsi.cpp:991-1002)
    char line[256];
    int n = 0;
    while ((n = rsi_result_log_line(res, n, line, (int)sizeof(line))) > 0) info << line << "\n";
  }
  info << "first pass\n\tmedian of transformations : " << S->tmedian1 << "\n\tsigma : " << S->tsigma1 << "\n\tlamda : " << S->tlamda1 << "\n"
       << "second pass\n\tmedian of transformations : " << S->tmedian2 << "\n\tsigma : " << S->tsigma2 << "\n\tlamda : " << S->tlamda2 << "\n"
       << "Selected " << rsi_result_ncalls(res, 3) << " segments for testing\n"
       << "Found " << rsi_result_ncalls(res, 1) << " CNVs before sd_filters, " << rsi_result_ncalls(res, 0) << " written\n"
       << "timing: fasta " << t_fasta << " s, ";
  if (from_bam)
    info << "BAM pileup " << bs->t_total_ms * 1e-3 << " s (" << bs->bytes_compressed << " bytes compressed, " << bs->records << " reads read, " << bs->used
         << " counted, inflate " << bs->t_inflate_ms * 1e-3 << " s" << (bs->indexed ? ", index used" : ", no index: scanned from the top") << ")";
  else
    info << "depth text " << ts->t_total_ms * 1e-3 << " s (" << ts->bytes << " bytes, " << ts->lines << " lines"
         << (ts->fallback ? ", host parser: positions not increasing" : "") << ")";
  info << ", whole device path " << t_path << " s (" << S->t_device_ms << " ms on resident inputs)\n";
  if (from_bam && o.bamread == "device") info << bam_read_line(ctx);
  if (from_bam) {   // if ( fp_in ) cnv_stat(fp_in, bamidx, cnvlist), rsi.cpp:2210
    const bool on_device = o.pairs == "device";   // the pair table of the load, still in HBM; else a second pass over the file
    if ((on_device ? rsi_result_annotate_device(ctx, res) : rsi_result_annotate_bam(res, o.bamfile.c_str(), chr.c_str())) != RSI_OK)
      info << "RP / Q0 annotation failed: " << rsi_hot_last_error(nullptr) << "\n";
    rsi_pairs_stats ps;
    if (on_device && rsi_hot_last_pairs_stats(ctx, &ps) == RSI_OK && ps.records + ps.table_bytes > 0)
      info << "#pairs: " << ps.records << " records, " << ps.table_bytes * 1e-6 << " MB, sample S " << ps.sample_stop << " isize " << ps.isize << " +- "
           << ps.isize_sd << ", " << ps.calls << " calls, " << ps.examined << " records examined, table " << ps.t_table_ms << " ms, sample "
           << ps.t_sample_ms << " ms, annotation " << ps.t_annotate_ms << " ms\n";
  }
  char row[1024];
  for (int i = 0; i < rsi_result_ncalls(res, 0); ++i) {
    rsi_result_format_row(res, i, chr.c_str(), row, (int)sizeof(row));
    co.rows.push_back(row);
  }
  // ---- plots (rsi.cpp:2213-2216: expand_data, plot_cnv): the data / script files of every written call, piped through gnuplot
  // and deleted, as the reference does -- and like the reference only when there is a gnuplot.  -plotfiles (not a reference
  // flag) writes and keeps the files without one. ----
  const double gv = gnuplot_found();
  if (o.plot && rsi_result_ncalls(res, 0) > 0 && gv <= 0 && !o.plotfiles) info << "gnuplot not found\n";
  if (o.plot && rsi_result_ncalls(res, 0) > 0 && (gv > 0 || o.plotfiles)) {
    const int64_t nc = S->n_compact, nfull = S->n;
    const bool on_device = o.plots == "device";   // -plots device: the figures' numbers come from HBM (rsi_hot_plot_run)
    std::vector<int32_t> full;
    double med = 0;
    std::shared_ptr<rsi_plot_batch> batch;
    const rsi_call* calls = rsi_result_calls(res, 0);
    bool have = false;
    if (on_device) {
      batch.reset(rsi_plot_batch_new(nfull, o.P.m, o.P.minmlen, o.P.chklen), rsi_plot_batch_free);
      for (int i = 0; batch && i < rsi_result_ncalls(res, 0); ++i) (void)rsi_plot_batch_add(batch.get(), &calls[i]);
      have = batch && rsi_hot_plot_run(ctx, res, batch.get()) == RSI_OK;
      rsi_plot_stats ps;
      if (have && rsi_hot_last_plot_stats(ctx, &ps) == RSI_OK)
        info << "#plots: " << chr << ": " << ps.calls << " calls, " << ps.queries << " points, " << ps.batches << " batches, " << ps.launches << " launches, "
             << ps.bytes_up << " bytes up, " << ps.bytes_down << " bytes down, " << ps.ms << " ms (expansion " << ps.expand_ms << " ms)\n";
    } else {
      std::vector<int32_t> rdc((size_t)nc), pairs((size_t)S->n_noncode * 2 + 2);
      full.resize((size_t)nfull);
      const int np = rsi_result_noncode(res, pairs.data(), S->n_noncode);
      have = rsi_hot_fetch_i32(ctx, "rd_concat", rdc.data(), nc) == nc && rsi_plot_expand(rdc.data(), nc, pairs.data(), np, full.data(), nfull) == RSI_OK;
      // plot::RDmed = _median over the expanded array (plotcnv.cpp:625): zeros of the N regions included
      if (have) med = rsih::grid_quantiles<int>(full.data(), (size_t)nfull).med;   // partition_stat_tp's walk, its degenerate case included
    }
    if (have) {
      (void)!system(("mkdir -p " + o.plotfolder).c_str());
      if (gv <= 0) info << "plot data and scripts are left in " << o.plotfolder << "\n";
      static const char* kT[3] = {"DEL", "DUP", "UNKNOWN"};
      std::vector<std::string> psfiles;
      for (int i = 0; i < rsi_result_ncalls(res, 0); ++i) {
        const rsi_call& c = calls[i];
        std::ostringstream base, title;
        base << o.plotfolder << "/rsi_" << chr << "_" << c.start << "_" << c.end << "_" << kT[c.type < 0 || c.type > 2 ? 2 : c.type];
        title << chr << ":" << c.start << "-" << c.end << " " << c.end - c.start + 1 << " " << kT[c.type < 0 || c.type > 2 ? 2 : c.type];
        const std::string dat = base.str() + ".dat", gp = base.str() + ".gp", img = base.str() + ".ps";
        info << "plotting: " << title.str() << "\n";
        const int rc = on_device ? rsi_plot_batch_write(batch.get(), i, title.str().c_str(), "ps", gv > 0 ? gv : 5.0, dat.c_str(), gp.c_str(), img.c_str())
                                 : rsi_plot_write_files(&c, title.str().c_str(), full.data(), nfull, med, o.P.m, o.P.minmlen, o.P.chklen, "ps", gv > 0 ? gv : 5.0, dat.c_str(), gp.c_str(), img.c_str());
        if (rc != RSI_OK) {
          info << "CNV exceeds reference length\n";
          continue;
        }
        if (gv > 0) draw_figure(dat, gp, img, psfiles);
      }
      convert_figures(psfiles, info);
    } else if (on_device) info << "plots skipped: " << rsi_hot_last_error(ctx) << "\n";
    else info << "plots skipped: the per-base depth could not be fetched\n";
  }
  co.log = info.str();
  rsi_result_free(res);
}

// Columns of the first data line of a depth file (-1: none): a whole-genome file has three, RNAME POS DEPTH, a cohort file
// RNAME POS D1 ... DK.  header: the tokens of the last "#CHROM ..." line in front of it (samtools depth -H), if any.
int first_line_columns(const std::string& path, std::vector<std::string>* header = nullptr) {   // through gzip / BGZF compression
  gzFile f = gzopen(path.c_str(), "rb");                                                        // (zlib reads plain text as it is)
  if (!f) return -1;
  struct Close { gzFile f; ~Close() { gzclose(f); } } closer{f};
  std::string line, tok;
  std::vector<char> buf(1 << 16);
  while (gzgets(f, buf.data(), (int)buf.size())) {
    line = buf.data();
    while (!line.empty() && line.back() == '\n') line.pop_back();
    if (header && line.compare(0, 6, "#CHROM") == 0) {
      std::istringstream iss(line);
      header->clear();
      while (iss >> tok) header->push_back(tok);
    }
    if (line.empty() || line[0] == '#') continue;
    std::istringstream iss(line);
    int k = 0;
    while (iss >> tok) ++k;
    if (k) return k;
  }
  return -1;
}

// bedGraph by name: after one optional .gz / .bgz, the name ends in .bed, .bedgraph or .bg (case-insensitive)
bool is_bedgraph_name(const std::string& path) {
  std::string n = path.substr(path.find_last_of('/') == std::string::npos ? 0 : path.find_last_of('/') + 1);
  std::transform(n.begin(), n.end(), n.begin(), [](unsigned char c) { return (char)std::tolower(c); });
  auto ends = [&](const char* x) { const size_t k = strlen(x); return n.size() > k && n.compare(n.size() - k, k, x) == 0; };
  if (ends(".gz")) n.resize(n.size() - 3);
  else if (ends(".bgz")) n.resize(n.size() - 4);
  return ends(".bed") || ends(".bedgraph") || ends(".bg");
}

// A track is BGZF by name: it ends in .gz or .bgz (case-insensitive), the suffixes is_bedgraph_name looks behind
bool gz_name(const std::string& path) {
  std::string n = path.substr(path.find_last_of('/') == std::string::npos ? 0 : path.find_last_of('/') + 1);
  std::transform(n.begin(), n.end(), n.begin(), [](unsigned char c) { return (char)std::tolower(c); });
  auto ends = [&](const char* x) { const size_t k = strlen(x); return n.size() > k && n.compare(n.size() - k, k, x) == 0; };
  return ends(".gz") || ends(".bgz");
}

// The .fai's names and lengths, in its order (read_fasta's index, readref.cpp:10-86)
bool read_fai(const std::string& fasta, std::vector<std::string>& names, std::vector<int64_t>& lens) {
  std::ifstream fai((fasta + ".fai").c_str());
  if (!fai) { std::cerr << "[read_fasta] Index file " << fasta << ".fai not found\n"; return false; }
  std::string line, name;
  while (std::getline(fai, line)) {
    std::istringstream iss(line);
    long len = 0;
    if (iss >> name >> len) { names.push_back(name); lens.push_back(len); }
  }
  return true;
}

// -d GENOME.depth without -c: the main thread drives the genome reader (ingest_genome.hip) and reads each finished chromosome's FASTA;
// `workers` threads, each on a context of one pool on -gpu, run the chromosomes whose depth is already in HBM and format them
// (report_chromosome, on the context that ran them: the plots fetch from it).  At most workers + 1 depth buffers exist: before
// asking for the next chromosome the main thread waits until one of the `workers` it may hold has come back.  cols (-samples):
// the cohort file's depth columns; a job is one (chromosome, sample), and a depth buffer goes back once all its samples have
// run.  Returns the outputs in the file's order of first appearance, outs[i][j] for sample j (one sample without cols); false
// (message in `err`) when the file cannot be read through.
// bed: a bedGraph file (rsi_genome_bedgraph_open); with `only` (-c RNAME) the reader knows RNAME's .fai sequence alone, and
// the file's other chromosomes are passed over.
bool run_genome(const Options& o, const std::vector<int32_t>& cols, std::vector<std::string>& chroms, std::vector<std::vector<ChromOutput>>& outs,
                std::string& err, std::string& summary, bool bed = false, const std::string* only = nullptr, RefReader* rr = nullptr) {
  std::vector<std::string> names;
  std::vector<int64_t> lens;
  if (!read_fai(o.reffile, names, lens)) { err = "no reference index"; return false; }
  if (only) {   // read_fasta's rule: the first sequence named RNAME or chrRNAME
    size_t k = 0;
    while (k < names.size() && names[k] != *only && names[k] != "chr" + *only) ++k;
    if (k == names.size()) { err = *only + " not found in fai index"; return false; }
    names = {names[k]}; lens = {lens[k]};
  }
  std::vector<const char*> cnames;
  for (const std::string& nm : names) cnames.push_back(nm.c_str());
  const int nwork = std::max(1, std::min(o.workers, 32));
  int st = 0;
  rsi_pool* pool = rsi_pool_create(o.device, nwork, &st);
  if (!pool) { err = rsi_hot_last_error(nullptr); return false; }
  const bool indexed = bed && only && !o.dindex_path.empty();
  rsi_genome_text* g = indexed ? rsi_genome_bedgraph_open_indexed(o.device, o.rdfile.c_str(), o.dindex_path.c_str(), (int)cnames.size(), cnames.data(), lens.data(), nwork + 1, 0, &st)
      : bed ? rsi_genome_bedgraph_open(o.device, o.rdfile.c_str(), (int)cnames.size(), cnames.data(), lens.data(), nwork + 1, 0, &st)
      : cols.empty()
      ? rsi_genome_text_open(o.device, o.rdfile.c_str(), (int)cnames.size(), cnames.data(), lens.data(), nwork + 1, 0, &st)
      : rsi_genome_text_open_samples(o.device, o.rdfile.c_str(), (int)cnames.size(), cnames.data(), lens.data(), cols.data(), (int)cols.size(),
                                     nwork + 1, 0, &st);
  if (!g) { err = rsi_hot_last_error(nullptr); rsi_pool_destroy(pool); return false; }
  const double t0 = now_s();
  const int nsamp = std::max<int>(1, (int)cols.size());
  const int max_held = rsi_genome_text_max_resident(g) - 1;   // the reader needs one free depth buffer for each new chromosome
  std::vector<Options> so(nsamp, o);   // sample k's plots go under <plotfolder>/k
  for (int j = 0; j < (int)cols.size(); ++j) {
    so[j].plotfolder = o.plotfolder + "/" + std::to_string(cols[j]);
    if (!o.trackfile.empty()) so[j].trackfile = o.trackfile + "." + std::to_string(cols[j]);   // as -o: FILE.k
    if (!o.bintrackfile.empty()) so[j].bintrackfile = o.bintrackfile + "." + std::to_string(cols[j]);
  }

  // fasta: read_fasta's host string, uploaded by every job; with the device reader (rr) d_fasta instead: the chromosome's sequence
  // in a device buffer that belongs to its slot, loaded once, read by all its samples' jobs, freed when the slot is released
  struct Job { size_t idx; int j; rsi_genome_chrom c; const void* d_depth; std::shared_ptr<const std::string> fasta; const void* d_fasta; double t_fasta; };
  std::vector<void*> slot_fasta((size_t)rsi_genome_text_max_resident(g), nullptr);
  auto free_slot_fasta = [&](int slot) { if (rr && slot_fasta[(size_t)slot]) { rr->release(slot_fasta[(size_t)slot]); slot_fasta[(size_t)slot] = nullptr; } };
  std::deque<Job> jobs;
  std::deque<std::vector<ChromOutput>> done_outs;   // stable references while the main thread appends
  std::vector<int> pending(rsi_genome_text_max_resident(g), 0);   // samples of each held depth buffer not run yet
  std::vector<int> returned;           // depth buffers whose chromosome has been run (all its samples)
  std::mutex mu;
  std::condition_variable cv_job, cv_back;
  bool closing = false;
  std::vector<std::thread> threads;
  for (int w = 0; w < nwork; ++w)
    threads.emplace_back([&, w]() {
      rsi_ctx* ctx = rsi_pool_worker(pool, w);
      for (;;) {
        Job j;
        {
          std::unique_lock<std::mutex> lk(mu);
          cv_job.wait(lk, [&] { return closing || !jobs.empty(); });
          if (jobs.empty()) return;
          j = std::move(jobs.front());
          jobs.pop_front();
        }
        ChromOutput co;
        co.track_index = j.idx;
        std::ostringstream info;
        const std::string chr = j.c.name;
        info << "#processing " << chr << "\n";
        rsi_result* res = nullptr;
        const double t1 = now_s();
        const bool armed = arm_exclude(ctx, o, chr, j.c.n, info);   // (false: it has logged why)
        const int rc = !armed ? RSI_ERR_BAD_ARG
            : j.d_fasta ? rsi_hot_run_device(ctx, &o.P, j.d_depth, j.d_fasta, j.c.n, &res)
                        : rsi_hot_run_depth_device(ctx, &o.P, j.d_depth, reinterpret_cast<const uint8_t*>(j.fasta->data()), j.c.n, &res);
        if (rc != RSI_OK) {   // as the BAM walk: a chromosome that has data and fails stops the run (rsi.cpp exits) -- of its sample
          if (armed) info << rsi_hot_last_error(ctx) << "\n";
          co.log = info.str();
          co.fatal = true;
        } else {
          // -track reads the reader's depth buffer through the context (rsi_hot_write_track: borrowed): the slot goes back only
          // below, once every sample's report is through -- checked, since a buffer released early would be another chromosome's
          bool slot_held;
          { std::lock_guard<std::mutex> lk(mu); slot_held = pending[(size_t)j.c.slot] > 0; }
          Options oj = so[(size_t)j.j];
          if (!slot_held && !oj.trackfile.empty()) {
            info << "track: " << chr << ": the depth buffer has been released\n";
            co.track_failed = true;
            oj.trackfile.clear();
          }
          report_chromosome(ctx, oj, chr, res, &j.c.stats, nullptr, j.t_fasta, now_s() - t1, info, co);
        }
        std::lock_guard<std::mutex> lk(mu);
        done_outs[j.idx][(size_t)j.j] = std::move(co);
        if (--pending[(size_t)j.c.slot] == 0) {
          returned.push_back(j.c.slot);
          cv_back.notify_one();
        }
      }
    });
  int held = 0;
  bool ok = true;
  for (;;) {
    {   // hand the run chromosomes' buffers back; hold at most max_held (nwork when memory allows)
      std::unique_lock<std::mutex> lk(mu);
      for (;;) {
        for (int slot : returned) { free_slot_fasta(slot); rsi_genome_text_release(g, slot); --held; }
        returned.clear();
        if (held < max_held) break;
        cv_back.wait(lk, [&] { return !returned.empty(); });
      }
    }
    rsi_genome_chrom c;
    const int rc = rsi_genome_text_next(g, &c);
    if (rc == 0) break;
    if (rc < 0) { err = rsi_genome_text_last_error(g); ok = false; break; }
    const std::string chr = c.name;
    if (only && c.slot < 0) continue;   // another chromosome of the file
    if (o.geno && !geno_names(*o.geno, chr)) {   // `geno` runs the chromosomes its list names
      if (c.slot >= 0) rsi_genome_text_release(g, c.slot);
      continue;
    }
    size_t idx;
    { std::lock_guard<std::mutex> lk(mu); idx = done_outs.size(); done_outs.emplace_back((size_t)nsamp); }
    chroms.push_back(chr);
    if (c.slot < 0) {
      std::lock_guard<std::mutex> lk(mu);
      for (ChromOutput& co : done_outs[idx]) co.log = chr + " not found in fai index, skipped\n";
      continue;
    }
    const double tf = now_s();
    auto fasta = std::make_shared<std::string>();
    bool have_fasta;
    if (rr) {
      std::string why;
      bool missing = false;
      int64_t nref = 0;
      have_fasta = rr->load(chr, slot_fasta[(size_t)c.slot], nref, why, &missing);
      if (have_fasta && nref != c.n) { have_fasta = false; why = chr + ": the reference has " + std::to_string(nref) + " bases, the depth reader " + std::to_string(c.n); }
      if (!have_fasta) { std::cerr << why << "\n"; free_slot_fasta(c.slot); }
    } else have_fasta = read_fasta(o.reffile, chr, *fasta);
    if (!have_fasta) {   // not fatal for a run over many chromosomes (process_chromosome with `many`)
      rsi_genome_text_release(g, c.slot);
      std::lock_guard<std::mutex> lk(mu);
      for (ChromOutput& co : done_outs[idx]) co.log = "#processing " + chr + "\n";
      continue;
    }
    const double t_fasta = now_s() - tf;
    std::lock_guard<std::mutex> lk(mu);
    pending[(size_t)c.slot] = nsamp;
    for (int j = 0; j < nsamp; ++j)
      jobs.push_back(Job{idx, j, c, cols.empty() ? c.d_depth : rsi_genome_text_sample_depth(g, c.slot, j), fasta, rr ? slot_fasta[(size_t)c.slot] : nullptr, t_fasta});
    ++held;
    cv_job.notify_all();
  }
  { std::lock_guard<std::mutex> lk(mu); closing = true; }
  cv_job.notify_all();
  for (auto& t : threads) t.join();
  for (size_t slot = 0; slot < slot_fasta.size(); ++slot) free_slot_fasta((int)slot);
  double bound_ms = 0, parse_ms = 0;
  rsi_genome_text_kernel_ms(g, &bound_ms, &parse_ms);
  std::ostringstream sm;
  if (only && ok && chroms.empty()) { ok = false; err = "no lines for " + *only + " in " + o.rdfile; }
  if (bed) sm << "#depth file: bedGraph (RNAME START END DEPTH), read as the per-base lines it stands for\n";
  if (indexed) {
    int64_t from = 0, stop = 0;
    (void)rsi_genome_text_index_range(g, &from, &stop);
    struct stat si, sd;
    if (stat(o.dindex_path.c_str(), &si) == 0 && stat(o.rdfile.c_str(), &sd) == 0 && si.st_mtime < sd.st_mtime)
      sm << "#depth index: warning: " << o.dindex_path << " is older than " << o.rdfile << "\n";
    sm << "#depth index: " << o.dindex_path << ", members at compressed offsets " << from << "-" << stop << " of the file\n";
  }
  sm << "timing: whole-genome depth text " << (now_s() - t0) << " s, " << chroms.size() << " chromosomes, boundary kernels " << bound_ms
     << " ms, parse kernels " << parse_ms << " ms\n";
  rsi_inflate_stats is;
  if (rsi_genome_text_inflate_stats(g, &is) == RSI_OK) sm << inflate_line(is);
  summary = sm.str();
  rsi_genome_text_close(g);
  rsi_pool_destroy(pool);
  outs.assign(std::make_move_iterator(done_outs.begin()), std::make_move_iterator(done_outs.end()));
  return ok;
}

// -samples all|k1,k2,...: the depth columns to call, checked against the file's K (its first data line's columns minus RNAME
// POS) before anything touches the device.  false: `err` says why.
bool select_samples(const Options& o, std::vector<int32_t>& cols, std::vector<std::string>& names, std::string& err) {
  if (o.chr_given) { err = "-samples: a cohort file is read as a whole genome, without -c"; return false; }
  if (!o.bamfile.empty() || o.rdfile.empty()) { err = "-samples: the samples are the depth columns of a whole-genome depth file (-d), not a BAM file"; return false; }
  if (o.gpus > 1) { err = "-gpus: a whole-genome depth file runs on one device (-gpu INT picks it)"; return false; }
  std::vector<std::string> header;
  const int ncol = first_line_columns(o.rdfile, &header);
  if (ncol < 0) { err = "-samples: no data line in " + o.rdfile; return false; }
  if (ncol < 3) { err = "-samples: " + o.rdfile + " has no RNAME POS DEPTH lines (readdepth file and chromosome must be specified together)"; return false; }
  const int K = ncol - 2;
  if (o.samples == "all") {
    if (K > 64) { err = "-samples all: the file has " + std::to_string(K) + " depth columns, more than 64 samples: select at most 64 with a list"; return false; }
    for (int k = 1; k <= K; ++k) cols.push_back(k);
  } else {
    std::stringstream ss(o.samples);
    std::string tok;
    std::set<int> seen;
    while (std::getline(ss, tok, ',')) {
      char* end = nullptr;
      const long k = tok.empty() ? 0 : strtol(tok.c_str(), &end, 10);
      if (tok.empty() || *end != '\0' || k < 1 || k > K) {
        err = "-samples: \"" + tok + "\" is not a depth column of " + o.rdfile + " (1.." + std::to_string(K) + ")";
        return false;
      }
      if (!seen.insert((int)k).second) { err = "-samples: column " + tok + " is selected twice"; return false; }
      cols.push_back((int32_t)k);
    }
    if (cols.empty() || o.samples.back() == ',') { err = "-samples: expected all or a list k1,k2,... of depth columns"; return false; }
    if (cols.size() > 64) { err = "-samples: " + std::to_string(cols.size()) + " columns selected, at most 64"; return false; }
  }
  if ((int)header.size() == ncol)   // "#CHROM POS name1 ... nameK"
    for (int32_t k : cols) names.push_back(header[(size_t)k + 1]);
  else
    names.assign(cols.size(), "");
  return true;
}

// -track and -bintrack (`what`: "track" / "bin track", `flag`: the option), after the run: the parts of the chromosomes whose rows
// were written (`order`, in row order) become FILE; every part 0 .. count - 1 is deleted whatever happened.  failed: a
// chromosome's part could not be written -- then there is no FILE.  bgzf: the parts are BGZF members; the end-of-file block ends FILE.
// index (-trackindex, a BGZF track): per entry of `order` its part's index; they are appended in row order, each moved by its
// part's offset in FILE, and written as FILE.tbi behind the end-of-file block.  A track that failed leaves no index.
bool finish_track(const std::string& file, const std::vector<size_t>& order, size_t count, bool failed, bool bgzf, std::ostream& log,
                  const std::vector<std::shared_ptr<rsi_track_index>>* index, const char* what = "track", const char* flag = "-track") {
  if (file.empty()) return true;
  std::string err;
  std::vector<int64_t> offsets;
  if (index) remove((file + ".tbi").c_str());
  if (failed) {
    rsitrack::remove_parts(file, count);
    remove(file.c_str());
    err = std::string("a chromosome's ") + what + " could not be written (see above)";
  } else if (rsitrack::join_parts(file, order, count, err, bgzf, &offsets)) {
    std::cerr << what << " written to " << file << std::endl; log << what << " written to " << file << std::endl;
    if (!index) return true;
    const std::shared_ptr<rsi_track_index> all = new_track_index();
    bool ok = all != nullptr;
    for (size_t k = 0; ok && k < order.size(); ++k)
      if (offsets[k] >= 0 && (*index)[k]) ok = rsi_track_index_append(all.get(), (*index)[k].get(), offsets[k]) == RSI_OK;
    ok = ok && rsi_track_index_write_tbi(all.get(), (file + ".tbi").c_str()) == RSI_OK;
    if (ok) {
      std::cerr << what << " index written to " << file << ".tbi" << std::endl; log << what << " index written to " << file << ".tbi" << std::endl;
      return true;
    }
    err = std::string("the index: ") + rsi_hot_last_error(nullptr);
  }
  std::cerr << "rsicnv: " << flag << ": " << err << std::endl; log << "rsicnv: " << flag << ": " << err << std::endl;
  return false;
}
// both kinds of track of one output: every part is dealt with, whichever fails
// What the chromosomes of one output leave for its tracks: whose rows were written, in row order, whether a part failed, the parts' indexes
struct TrackParts {
  std::vector<size_t> order;
  bool track_failed = false, bintrack_failed = false;
  std::vector<std::shared_ptr<rsi_track_index>> track_ix, bintrack_ix;   // per entry of `order`
  void add(size_t i, const ChromOutput& co) {
    track_failed = track_failed || co.track_failed;
    bintrack_failed = bintrack_failed || co.bintrack_failed;
    if (!co.populated) return;
    order.push_back(i);
    track_ix.push_back(co.track_ix);
    bintrack_ix.push_back(co.bintrack_ix);
  }
};
bool finish_tracks(const Options& o, const std::string& suffix, const TrackParts& p, size_t count, std::ostream& log) {
  const bool a = finish_track(o.trackfile.empty() ? "" : o.trackfile + suffix, p.order, count, p.track_failed, o.track_bgzf, log,
                              o.trackindex && o.track_bgzf ? &p.track_ix : nullptr);
  const bool b = finish_track(o.bintrackfile.empty() ? "" : o.bintrackfile + suffix, p.order, count, p.bintrack_failed, o.bintrack_bgzf, log,
                              o.trackindex && o.bintrack_bgzf ? &p.bintrack_ix : nullptr, "bin track", "-bintrack");
  return a && b;
}

// `rsicnv stat` and `rsicnv pin`: the lines of -v CNVFILE grouped by chromosome, each chromosome's BAM records
// loaded once with the pair table (and for pin the CIGARs) kept in HBM, the results written back in the file's order.  A line
// this build cannot serve -- a chromosome the BAM header does not name, a chromosome the sample's limits refuse -- is written
// as it stands, and the log says why.
int run_cnvlist(const Options& o) {
  const bool pin = o.function == "pin";
  if (o.bamfile.empty()) { std::cerr << "rsicnv " << o.function << ": need a BAM file (-b BAMFILE)" << std::endl; return 1; }
  if (o.cnvfile.empty()) { std::cerr << "rsicnv " << o.function << ": need a CNV list (-v CNVFILE)" << std::endl; return 1; }
  if (o.gpus > 1) { std::cerr << "rsicnv " << o.function << ": -gpus: a CNV list runs on one device (-gpu INT picks it)" << std::endl; return 1; }
  if (!o.bamread.empty() && o.bamread != "device" && o.bamread != "host") {
    std::cerr << "rsicnv: -bamread " << o.bamread << ": expected device or host" << std::endl;
    return 1;
  }
  std::vector<std::string> names;
  {
    std::vector<char> buf(1 << 20);
    std::vector<int64_t> lens(65536);
    const int nref = rsi_bam_references(o.bamfile.c_str(), buf.data(), (int)buf.size(), lens.data(), (int)lens.size());
    if (nref < 0) { std::cerr << "rsicnv " << o.function << ": " << rsi_hot_last_error(nullptr) << std::endl; return 1; }
    std::istringstream iss(buf.data());
    std::string nm;
    while (std::getline(iss, nm)) names.push_back(nm);
  }
  std::vector<rsipinh::CnvLine> lines;
  if (!rsipinh::read_cnvlist(o.cnvfile, names, lines, std::cerr)) return 0;      // the reference says so and exits with 0
  std::ofstream log((o.outfile + ".log").c_str());
  std::vector<std::string> rows(lines.size());
  std::vector<size_t> known;                    // the lines whose chromosome the header names, in file order
  for (size_t i = 0; i < lines.size(); ++i) {
    rows[i] = lines[i].text;
    if (lines[i].tid >= 0) known.push_back(i);
    else log << "#" << o.function << ": " << lines[i].cell[0] << " is not in the BAM header: line written unchanged\n";
  }
  // cnv_stat's windows: DIS travels through the whole file, so they are fixed before the lines are grouped
  std::vector<rsipinh::CnvLine> known_lines;
  for (size_t i : known) known_lines.push_back(lines[i]);
  const std::vector<rsipairs::Call> windows = rsipinh::stat_windows(known_lines);
  std::vector<int> order;                       // chromosomes by first appearance
  for (size_t i : known) if (std::find(order.begin(), order.end(), lines[i].tid) == order.end()) order.push_back(lines[i].tid);

  int st = 0;
  rsi_ctx* ctx = order.empty() ? nullptr : rsi_hot_create(o.device, &st);
  if (!order.empty() && !ctx) { std::cerr << "rsicnv " << o.function << ": no context on device " << o.device << ": " << rsi_hot_last_error(nullptr) << std::endl; return 1; }
  struct Destroy { rsi_ctx* c; ~Destroy() { if (c) rsi_hot_destroy(c); } } destroy{ctx};
  if (ctx && ((!o.bamread.empty() && rsi_hot_set_bam_read(ctx, o.bamread == "device" ? RSI_BAM_READ_DEVICE : RSI_BAM_READ_HOST, 0) != RSI_OK) ||
              (pin ? rsi_hot_set_bam_pin(ctx, 1) : rsi_hot_set_bam_pairs(ctx, 1)) != RSI_OK)) {
    std::cerr << "rsicnv " << o.function << ": " << rsi_hot_last_error(ctx) << std::endl;
    return 1;
  }
  int32_t isize = -1, isize_sd = -1;
  for (int tid : order) {
    const std::string& chrom = names[(size_t)tid];
    std::vector<size_t> mine, at;               // this chromosome's lines, and where each stands among the known ones
    for (size_t k = 0; k < known.size(); ++k) if (lines[known[k]].tid == tid) { mine.push_back(known[k]); at.push_back(k); }
    std::vector<int32_t> start, end, type;
    bool sampled = !pin;                        // optimize_resolution samples a chromosome at its first line of 800 bases or more
    for (size_t i : mine) {
      start.push_back(lines[i].start); end.push_back(lines[i].end); type.push_back(lines[i].type);
      if (std::abs((long long)lines[i].end - lines[i].start) >= 800) sampled = true;
    }
    auto refuse = [&](const std::string& why) { log << "#" << o.function << ": " << chrom << ": " << why << ": its lines are written unchanged\n"; };
    if (pin && !sampled) {
      for (size_t i : mine) rows[i] = rsipinh::pin_row(lines[i], lines[i].start, lines[i].end, 0, 0);
      continue;
    }
    rsi_bam_stats bs;
    memset(&bs, 0, sizeof(bs));
    const double t0 = now_s();
    if (rsi_hot_load_depth_bam(ctx, o.bamfile.c_str(), chrom.c_str(), o.minq, o.min_baseQ, &bs) != RSI_OK) { refuse(rsi_hot_last_error(ctx)); continue; }
    const double t1 = now_s();
    const size_t nl = mine.size();
    if (!pin) {
      std::vector<int32_t> p1e, p2e, rp(nl);
      std::vector<double> q0(nl);
      for (size_t k : at) { p1e.push_back(windows[k].p1e); p2e.push_back(windows[k].p2e); }
      if (rsi_hot_stat_calls(ctx, (int)nl, start.data(), end.data(), type.data(), p1e.data(), p2e.data(), &isize, &isize_sd, rp.data(), q0.data()) != RSI_OK) {
        refuse(rsi_hot_last_error(ctx));
        continue;
      }
      for (size_t k = 0; k < nl; ++k) rows[mine[k]] = rsipinh::stat_row(lines[mine[k]], rp[k], q0[k]);
      log << "#stat: " << chrom << ": " << nl << " lines, " << bs.on_chrom << " reads, ISIZE " << isize << " +- " << isize_sd << ", load " << (t1 - t0) * 1e3
          << " ms, counts " << (now_s() - t1) * 1e3 << " ms\n";
      continue;
    }
    rsi_pin_stats ps;
    if (rsi_hot_pin_sample(ctx, &ps) != RSI_OK) { refuse(rsi_hot_last_error(ctx)); continue; }
    rsipinh::SampleStats ss;
    ss.l_qseq = ps.l_qseq; ss.rd = ps.rd; ss.rd_sd = ps.rd_sd; ss.drd = ps.drd; ss.drd_sd = ps.drd_sd;
    log << rsipinh::sample_log(chrom, ss);
    std::vector<int32_t> ns(nl), ne(nl), sc1(nl), sc2(nl);
    if (rsi_hot_pin_calls(ctx, o.P.m, (int)nl, start.data(), end.data(), type.data(), ns.data(), ne.data(), sc1.data(), sc2.data()) != RSI_OK) {
      refuse(rsi_hot_last_error(ctx));
      continue;
    }
    for (size_t k = 0; k < nl; ++k) rows[mine[k]] = rsipinh::pin_row(lines[mine[k]], ns[k], ne[k], sc1[k], sc2[k]);
    rsi_hot_last_pin_stats(ctx, &ps);
    log << "#pin: " << chrom << ": " << nl << " lines, " << ps.breakpoints << " breakpoints, window +-" << ps.r_len << ", " << ps.records << " reads, "
        << ps.table_bytes * 1e-6 << " MB of CIGARs, load " << (t1 - t0) * 1e3 << " ms, sample " << ps.t_sample_ms << " ms, windows " << ps.t_windows_ms
        << " ms (device)\n";
  }
  std::ofstream out(o.outfile.c_str());
  for (const std::string& r : rows) out << r << "\n";
  return out.good() ? 0 : 1;
}

// `geno`: what one output (OUT, or a sample's OUT.k) collects from its chromosomes, and the file it becomes: the list's lines in
// the list's order, each with its field; a line nobody served is written as it stands and the log says why.
struct GenoCollect {
  std::vector<std::string> field, cn;
  std::vector<std::string> seen;   // the chromosomes this output's run met
  explicit GenoCollect(size_t n) : field(n), cn(n, "NA") {}
  void take(const std::string& chr, const ChromOutput& co) {
    seen.push_back(chr);
    if (co.geno_done) for (const GenoRow& r : co.geno) { field[r.line] = r.field; cn[r.line] = r.cn; }
  }
  bool write(const std::vector<rsipinh::CnvLine>& lines, const std::string& path, std::ostream& log) const {
    std::ofstream out(path.c_str());
    for (size_t i = 0; i < lines.size(); ++i) {
      if (!field[i].empty()) { out << lines[i].text << "\t" << field[i] << "\n"; continue; }
      out << lines[i].text << "\n";
      bool met = false;
      for (const std::string& c : seen) met = met || same_chrom(lines[i].cell[0], c);
      log << "#geno: " << lines[i].cell[0] << (met ? ": its run failed (see above)" : " is not in the input") << ": line written unchanged\n";
    }
    out.close();
    std::cerr << "output written to " << path << std::endl; log << "output written to " << path << std::endl;
    return out.good();
  }
};

// `rsicnv depth`: every chromosome of the input loaded once as rsi loads it -- the same selection, the same
// readers -- and summed from HBM, no calling run and no FASTA: PREFIX.mosdepth.summary.txt, PREFIX.mosdepth.global.dist.txt,
// PREFIX.per-base.bed.gz (unless -nobase), PREFIX.regions.bed.gz (with -by), PREFIX.log.  One context, one chromosome at a time.
int run_depth(const Options& o, int argc, char** argv) {
  auto refuse = [](const std::string& why) { std::cerr << "rsicnv depth: " << why << std::endl; return 1; };
  // refused where it cannot work, before any output
  if (!o.out_given) return refuse("need an output prefix (-o PREFIX)");
  if (o.gpus > 1) return refuse("-gpus: the coverage files are written by one device (-gpu INT picks it)");
  if (o.samples_given) return refuse("-samples: one sample at a time (a cohort file's columns are not summed)");
  if (!o.trackformat.empty() && o.trackformat != "text" && o.trackformat != "bgzf") return refuse("-trackformat " + o.trackformat + ": expected text or bgzf");
  if (!o.bamread.empty() && o.bamread != "device" && o.bamread != "host") return refuse("-bamread " + o.bamread + ": expected device or host");
  if (!o.dformat.empty() && o.dformat != "depth" && o.dformat != "bedgraph") return refuse("-dformat " + o.dformat + ": expected depth or bedgraph");
  const bool from_bam = !o.bamfile.empty();
  if (!o.bamread.empty() && !from_bam) return refuse("-bamread device|host: there is no BAM file to read (-b BAMFILE)");
  const bool bgzf = o.trackformat != "text";
  if (o.trackindex && (!bgzf || o.nobase)) return refuse("-trackindex: no BGZF per-base track to index (not with -trackformat text or -nobase)");
  int64_t W = 0;
  std::vector<rsidepth::BedLine> bed;
  const bool by_number = !o.by.empty() && o.by.find_first_not_of("0123456789", o.by[0] == '-' ? 1 : 0) == std::string::npos && o.by != "-";
  if (by_number) {
    W = o.by.size() > 18 ? 0 : atoll(o.by.c_str());
    if (W <= 0) return refuse("-by " + o.by + ": a window has at least one base");
  } else if (!o.by.empty()) {
    std::ifstream in(o.by.c_str());
    if (!in) return refuse("-by: cannot open " + o.by);
    std::string err;
    if (!rsidepth::read_bed(in, o.by, bed, err)) return refuse("-by: " + err);
  }
  const bool bedgraph = !from_bam && (o.dformat.empty() ? is_bedgraph_name(o.rdfile) : o.dformat == "bedgraph");
  const bool one = o.chr != "1-22XY" && !o.chr.empty();   // -c RNAME
  const bool genome = !from_bam && (!one || bedgraph);    // the genome reader: RNAME POS DEPTH, or bedGraph (whole, or RNAME's lines)
  std::vector<std::string> fnames;
  std::vector<int64_t> flens;
  if (!from_bam && !read_fai(o.reffile, fnames, flens)) return 1;
  size_t fai_one = 0;
  if (!from_bam && one) {   // read_fasta's rule: the first sequence named RNAME or chrRNAME
    while (fai_one < fnames.size() && fnames[fai_one] != o.chr && fnames[fai_one] != "chr" + o.chr) ++fai_one;
    if (fai_one == fnames.size()) return refuse(o.chr + " not found in fai index");
  }
  std::string dindex_path;   // -dindex: as rsi, for -d FILE.bed.gz -c RNAME
  if (!o.dindex.empty() && o.dindex != "none" && !(bedgraph && one)) return refuse("-dindex: an index serves -d FILE -c RNAME with a bedGraph FILE in BGZF only");
  if (bedgraph && one && o.dindex != "none") {
    unsigned char head[4] = {0, 0, 0, 0};
    FILE* f = fopen(o.rdfile.c_str(), "rb");
    const bool is_bgzf = f && fread(head, 1, 4, f) == 4 && head[0] == 0x1f && head[1] == 0x8b && head[2] == 8 && (head[3] & 4);
    if (f) fclose(f);
    if (!o.dindex.empty()) dindex_path = o.dindex;
    else if (is_bgzf) for (const char* ext : {".tbi", ".csi"}) if (dindex_path.empty() && access((o.rdfile + ext).c_str(), R_OK) == 0) dindex_path = o.rdfile + ext;
  }

  const std::string gz = bgzf ? ".gz" : "";
  const std::string base_path = o.outfile + ".per-base.bed" + gz, region_path = o.outfile + ".regions.bed" + gz;
  std::ofstream log((o.outfile + ".log").c_str());
  std::ostringstream hdr;
  hdr << "#command:   "; for (int i = 0; i < argc; ++i) hdr << argv[i] << " ";
  hdr << "\n#bamfile:   " << o.bamfile << "\n#rdfile:    " << o.rdfile << "\n#chrom:     " << o.chr << "\n#min_mapq:  " << o.minq << "\n#min_baseQ: " << o.min_baseQ
      << "\n#output:    " << o.outfile << "\n";
  std::cerr << hdr.str(); log << hdr.str();
  auto say = [&](const std::string& s) { std::cerr << s; log << s; };

  int st = 0;
  rsi_ctx* ctx = rsi_hot_create(o.device, &st);
  if (!ctx) { say("rsicnv depth: no context on device " + std::to_string(o.device) + ": " + rsi_hot_last_error(nullptr) + "\n"); return 1; }
  struct Destroy { rsi_ctx* c; ~Destroy() { rsi_hot_destroy(c); } } destroy{ctx};
  std::shared_ptr<rsi_track_index> index = o.trackindex ? new_track_index() : nullptr;
  if ((from_bam && !o.bamread.empty() && rsi_hot_set_bam_read(ctx, o.bamread == "device" ? RSI_BAM_READ_DEVICE : RSI_BAM_READ_HOST, 0) != RSI_OK) ||
      rsi_hot_set_track_format(ctx, bgzf ? RSI_TRACK_BGZF : RSI_TRACK_TEXT) != RSI_OK) {
    say(std::string("rsicnv depth: ") + rsi_hot_last_error(ctx) + "\n");
    return 1;
  }

  std::vector<rsidepth::ChromSummary> rows;
  std::vector<int64_t> total(rsidepth::kDistBins, 0), dist(rsidepth::kDistBins);
  std::ostringstream dist_text;
  std::vector<std::string> seen;
  bool wrote_base = false, wrote_regions = false, ok = true, refused = false;
  // one chromosome, its depth in HBM: the summary, then the tracks
  auto chromosome = [&](const std::string& chr, const void* d_depth, int64_t n) {
    const double t0 = now_s();
    rsi_depth_summary sum;
    rsi_depth_stats ds;
    if (rsi_hot_depth_summary(ctx, d_depth, n, &sum, dist.data(), rsidepth::kDistBins) != RSI_OK) {
      say("#depth: " + chr + ": " + rsi_hot_last_error(ctx) + ": nothing written for it\n");
      refused = true;
      return;
    }
    // the chromosome is summed: it enters the two tables here, whatever becomes of its tracks (a track that fails is an exit
    // status of 1, and the log says which file lacks the chromosome or ends in a part of it)
    seen.push_back(chr);
    (void)rsi_hot_last_depth_stats(ctx, &ds);
    int64_t launches = ds.launches;
    rsidepth::ChromSummary row;
    row.name = chr; row.length = n; row.bases = sum.sum; row.min = sum.min; row.max = sum.max;
    rows.push_back(row);
    rsidepth::write_dist(dist_text, chr, dist.data(), n, sum.max);
    for (int k = 0; k < rsidepth::kDistBins; ++k) total[(size_t)k] += dist[(size_t)k];
    rsi_track_stats tk;
    if (!o.nobase) {
      (void)rsi_hot_set_track_index(ctx, index.get());
      const int rc = rsi_hot_write_track_device(ctx, d_depth, n, chr.c_str(), base_path.c_str(), wrote_base ? 1 : 0, &tk);
      (void)rsi_hot_set_track_index(ctx, nullptr);
      if (rc != RSI_OK) {
        say("#depth: " + chr + ": per-base track: " + rsi_hot_last_error(ctx) + ": " + base_path + " is incomplete from " + chr + " on, the tables hold it\n");
        ok = false;
        return;
      }
      wrote_base = true;
    }
    if (W > 0 || !bed.empty() || (!o.by.empty() && !by_number)) {
      int rc;
      if (W > 0) rc = rsi_hot_write_window_track(ctx, d_depth, n, chr.c_str(), W, region_path.c_str(), wrote_regions ? 1 : 0, &tk);
      else {
        std::vector<int64_t> s, e;
        for (const rsidepth::BedLine& l : bed) if (rsidepth::same_chrom(l.chrom, chr)) { s.push_back(l.start); e.push_back(l.end); }
        rc = rsi_hot_write_region_track(ctx, d_depth, n, chr.c_str(), (int)s.size(), s.data(), e.data(), region_path.c_str(), wrote_regions ? 1 : 0, &tk);
      }
      if (rc != RSI_OK) {
        say("#depth: " + chr + ": regions: " + rsi_hot_last_error(ctx) + ": " + region_path + " is incomplete from " + chr + " on, the tables" +
            (o.nobase ? "" : " and " + base_path) + " hold it\n");
        ok = false;
        return;
      }
      wrote_regions = true;
      (void)rsi_hot_last_depth_stats(ctx, &ds);
      launches += ds.launches;
    }
    std::ostringstream line;
    line << "#depth: " << chr << ": length " << n << ", mean " << rsidepth::fixed2(sum.sum, n) << ", " << launches << " launches, " << (now_s() - t0) * 1e3 << " ms\n";
    say(line.str());
  };

  if (from_bam) {
    std::vector<std::string> todo;
    std::vector<int64_t> todo_len;
    if (!select_chromosomes(o, todo, todo_len, log)) return 1;
    const bool many = todo.size() > 1;
    for (const std::string& chr : todo) {
      rsi_bam_stats bs;
      memset(&bs, 0, sizeof(bs));
      if (rsi_hot_load_depth_bam(ctx, o.bamfile.c_str(), chr.c_str(), o.minq, o.min_baseQ, &bs) != RSI_OK) {
        say("#depth: " + chr + ": " + rsi_hot_last_error(ctx) + "\n");
        ok = false;
        continue;
      }
      if (o.bamread == "device") say(bam_read_line(ctx));
      if (many && bs.on_chrom == 0) { say("no reads on " + chr + "\n"); continue; }   // not "populated": rsi does not process it (rsi.cpp:2125)
      const void* d = nullptr;
      int64_t n = 0;
      if (rsi_hot_loaded_depth(ctx, &d, &n) != RSI_OK) { say("#depth: " + chr + ": " + rsi_hot_last_error(ctx) + "\n"); ok = false; continue; }
      chromosome(chr, d, n);
    }
  } else if (!genome) {   // POS DEPTH with -c RNAME
    rsi_text_stats ts;
    const void* d = nullptr;
    int64_t n = 0;
    if (rsi_hot_load_depth_text(ctx, o.rdfile.c_str(), flens[fai_one], &ts) != RSI_OK || rsi_hot_loaded_depth(ctx, &d, &n) != RSI_OK) {
      say("#depth: " + o.chr + ": " + rsi_hot_last_error(ctx) + "\n");
      ok = false;
    } else {
      rsi_inflate_stats is;
      if (rsi_hot_last_inflate_stats(ctx, &is) == RSI_OK) say(inflate_line(is));
      chromosome(o.chr, d, n);
    }
  } else {   // the genome reader, in the file's order
    if (one) { fnames = {fnames[fai_one]}; flens = {flens[fai_one]}; }
    std::vector<const char*> cnames;
    for (const std::string& nm : fnames) cnames.push_back(nm.c_str());
    rsi_genome_text* g = bedgraph && one && !dindex_path.empty()
        ? rsi_genome_bedgraph_open_indexed(o.device, o.rdfile.c_str(), dindex_path.c_str(), (int)cnames.size(), cnames.data(), flens.data(), 2, 0, &st)
        : bedgraph ? rsi_genome_bedgraph_open(o.device, o.rdfile.c_str(), (int)cnames.size(), cnames.data(), flens.data(), 2, 0, &st)
                   : rsi_genome_text_open(o.device, o.rdfile.c_str(), (int)cnames.size(), cnames.data(), flens.data(), 2, 0, &st);
    if (!g) { say(std::string("rsicnv depth: ") + rsi_hot_last_error(nullptr) + "\n"); return 1; }
    for (;;) {
      rsi_genome_chrom c;
      const int rc = rsi_genome_text_next(g, &c);
      if (rc == 0) break;
      if (rc < 0) { say(std::string("rsicnv depth: ") + rsi_genome_text_last_error(g) + "\n"); ok = false; break; }
      if (c.slot < 0) { if (!one) say(std::string(c.name) + " not found in fai index, skipped\n"); continue; }
      chromosome(c.name, c.d_depth, c.n);
      rsi_genome_text_release(g, c.slot);
    }
    rsi_inflate_stats is;
    if (rsi_genome_text_inflate_stats(g, &is) == RSI_OK) say(inflate_line(is));
    rsi_genome_text_close(g);
  }

  // the files end: the BGZF end-of-file blocks, the index, the two tables
  if (bgzf && wrote_base && rsi_bgzf_write_eof(base_path.c_str()) != RSI_OK) { say(std::string("rsicnv depth: ") + rsi_hot_last_error(nullptr) + "\n"); ok = false; }
  if (bgzf && wrote_regions && rsi_bgzf_write_eof(region_path.c_str()) != RSI_OK) { say(std::string("rsicnv depth: ") + rsi_hot_last_error(nullptr) + "\n"); ok = false; }
  if (index && wrote_base && ok) {
    if (rsi_track_index_write_tbi(index.get(), (base_path + ".tbi").c_str()) != RSI_OK) { say(std::string("rsicnv depth: ") + rsi_hot_last_error(nullptr) + "\n"); ok = false; }
    else say("index written to " + base_path + ".tbi" + index_counts(index.get()) + "\n");
  }
  std::vector<std::pair<std::string, int64_t>> unmet;   // -by FILE: names of no chromosome of the input, by first appearance
  for (const rsidepth::BedLine& l : bed) {
    bool met = false;
    for (const std::string& c : seen) met = met || rsidepth::same_chrom(l.chrom, c);
    if (met) continue;
    size_t k = 0;
    while (k < unmet.size() && unmet[k].first != l.chrom) ++k;
    if (k == unmet.size()) unmet.emplace_back(l.chrom, 0);
    ++unmet[k].second;
  }
  for (const auto& u : unmet) say("#depth: -by: " + u.first + " is not in the input" + (refused ? " (or was refused above)" : "") + ": " + std::to_string(u.second) + " lines passed over\n");
  {
    std::ofstream out((o.outfile + ".mosdepth.summary.txt").c_str());
    rsidepth::write_summary(out, rows);
    out.close();
    if (!out.good()) ok = false;
  }
  {
    int64_t n = 0;
    int32_t top = 0;
    for (const rsidepth::ChromSummary& r : rows) { n += r.length; top = std::max(top, r.max); }
    std::ofstream out((o.outfile + ".mosdepth.global.dist.txt").c_str());
    out << dist_text.str();
    rsidepth::write_dist(out, "total", total.data(), n, top);
    out.close();
    if (!out.good()) ok = false;
  }
  say("coverage written to " + o.outfile + ".mosdepth.summary.txt, " + o.outfile + ".mosdepth.global.dist.txt" + (wrote_base ? ", " + base_path : "") +
      (wrote_regions ? ", " + region_path : "") + "\n");
  return ok ? 0 : 1;
}

// `rsicnv view`: the figures of an existing CNV list, what the reference's `plot` does (rsi.cpp:2151-2185) -- raw depth,
// no GC adjustment, no cap, nothing removed.  Every chromosome the list names is loaded once (a depth file's, or a BAM's pileup), its
// lines are planned against its length, filled from HBM (rsi_hot_plot_depth) and written as rsi's plot step writes a call's.
int run_view(const Options& o_in, int argc, char** argv) {
  auto refuse = [](const std::string& why) { std::cerr << "rsicnv view: " << why << std::endl; return 1; };
  // refused where it cannot work, before any output
  if (o_in.cnvfile.empty()) return refuse("need a list of CNVs (-v CNVFILE)");
  if (o_in.gpus > 1) return refuse("-gpus: a CNV list runs on one device (-gpu INT picks it)");
  if (o_in.samples_given) return refuse("-samples: one sample at a time");
  const bool from_bam = !o_in.bamfile.empty();
  if (!from_bam && !o_in.chr_given) return refuse("-d RDFILE needs -c RNAME (a whole-genome depth file is not read)");
  if (!o_in.bamread.empty() && o_in.bamread != "device" && o_in.bamread != "host") return refuse("-bamread " + o_in.bamread + ": expected device or host");
  if (!o_in.bamread.empty() && !from_bam) return refuse("-bamread device|host: there is no BAM file to read (-b BAMFILE)");
  std::vector<rsipinh::CnvLine> lines;
  if (!rsipinh::read_cnvlist(o_in.cnvfile, {}, lines, std::cerr)) return 0;   // as stat / pin: the reference says so and exits with 0
  Options o = o_in;
  o.geno = &lines;   // select_chromosomes: of a BAM's header, the chromosomes the list names
  std::vector<std::string> fnames;
  std::vector<int64_t> flens;
  size_t fai_one = 0;
  if (!from_bam) {   // read_fasta's rule: the first sequence named RNAME or chrRNAME
    if (!read_fai(o.reffile, fnames, flens)) return 1;
    while (fai_one < fnames.size() && fnames[fai_one] != o.chr && fnames[fai_one] != "chr" + o.chr) ++fai_one;
    if (fai_one == fnames.size()) return refuse(o.chr + " not found in fai index");
  }
  const double gv = gnuplot_found();
  if (gv <= 0 && !o.plotfiles) { std::cerr << "gnuplot not found" << std::endl; return 0; }   // plot_cnv returns there, and the reference exits with 0

  (void)!system(("mkdir -p " + o.plotfolder).c_str());
  std::ofstream log((o.plotfolder + "/view.log").c_str());
  if (!log) return refuse("cannot write into " + o.plotfolder);
  log << "#command:   "; for (int i = 0; i < argc; ++i) log << argv[i] << " ";
  log << "\n";
  auto say = [&](const std::string& s) { std::cerr << s; log << s; };
  int st = 0;
  rsi_ctx* ctx = rsi_hot_create(o.device, &st);
  if (!ctx) { say("rsicnv view: no context on device " + std::to_string(o.device) + ": " + rsi_hot_last_error(nullptr) + "\n"); return 1; }
  struct Destroy { rsi_ctx* c; ~Destroy() { rsi_hot_destroy(c); } } destroy{ctx};
  if (from_bam && !o.bamread.empty() && rsi_hot_set_bam_read(ctx, o.bamread == "device" ? RSI_BAM_READ_DEVICE : RSI_BAM_READ_HOST, 0) != RSI_OK) {
    say(std::string("rsicnv view: ") + rsi_hot_last_error(ctx) + "\n");
    return 1;
  }
  if (gv <= 0) say("plot data and scripts are left in " + o.plotfolder + "\n");

  bool ok = true;
  std::vector<std::string> seen, psfiles;
  // one chromosome, its depth in HBM: its lines planned, filled and written
  auto chromosome = [&](const std::string& chr, const void* d_depth, int64_t n) {
    seen.push_back(chr);
    std::shared_ptr<rsi_plot_batch> batch(rsi_plot_batch_new(n, o.P.m, o.P.minmlen, o.P.chklen), rsi_plot_batch_free);
    if (!batch) { say("#view: " + chr + ": an array of " + std::to_string(n) + " values cannot be planned\n"); ok = false; return; }
    std::vector<size_t> mine;
    for (size_t i = 0; i < lines.size(); ++i) {
      if (!same_chrom(lines[i].cell[0], chr)) continue;
      mine.push_back(i);
      (void)rsi_plot_batch_add_span(batch.get(), lines[i].start, lines[i].end, lines[i].type);
    }
    if (rsi_hot_plot_depth(ctx, d_depth, n, batch.get()) != RSI_OK) { say("#view: " + chr + ": " + rsi_hot_last_error(ctx) + ": no figures for it\n"); ok = false; return; }
    rsi_plot_stats ps;
    (void)rsi_hot_last_plot_stats(ctx, &ps);
    int written = 0;
    for (size_t k = 0; k < mine.size(); ++k) {
      const rsipinh::CnvLine& l = lines[mine[k]];
      const std::string what = chr + ":" + l.cell[1] + "-" + l.cell[2] + " " + l.cell[3];
      if (const int r = rsi_plot_batch_refusal(batch.get(), (int)k)) { say("#view: " + what + ": " + rsi_plot_refusal_text(r) + ": no figure\n"); continue; }
      const std::string base = o.plotfolder + "/rsi_" + chr + "_" + l.cell[1] + "_" + l.cell[2] + "_" + l.cell[3];
      const std::string title = chr + ":" + l.cell[1] + "-" + l.cell[2] + " " + std::to_string(abs(l.end - l.start) + 1) + " " + l.cell[3];
      const std::string dat = base + ".dat", gp = base + ".gp", img = base + ".ps";
      say("plotting: " + title + "\n");
      if (rsi_plot_batch_write(batch.get(), (int)k, title.c_str(), "ps", gv > 0 ? gv : 5.0, dat.c_str(), gp.c_str(), img.c_str()) != RSI_OK) {
        say("#view: " + what + ": cannot write " + dat + "\n");
        ok = false;
        continue;
      }
      ++written;
      if (gv > 0) draw_figure(dat, gp, img, psfiles);
    }
    std::ostringstream line;
    line << "#plots: " << chr << ": " << mine.size() << " lines, " << written << " figures, " << ps.queries << " points, " << ps.batches << " batches, "
         << ps.launches << " launches, " << ps.bytes_up << " bytes up, " << ps.bytes_down << " bytes down, " << ps.ms << " ms\n";
    say(line.str());
  };

  if (from_bam) {
    std::vector<std::string> todo;
    std::vector<int64_t> todo_len;
    if (!select_chromosomes(o, todo, todo_len, log)) return 1;
    for (const std::string& chr : todo) {
      if (!geno_names(lines, chr)) continue;   // -c RNAME that the list does not name
      rsi_bam_stats bs;
      memset(&bs, 0, sizeof(bs));
      const void* d = nullptr;
      int64_t n = 0;
      if (rsi_hot_load_depth_bam(ctx, o.bamfile.c_str(), chr.c_str(), o.minq, o.min_baseQ, &bs) != RSI_OK || rsi_hot_loaded_depth(ctx, &d, &n) != RSI_OK) {
        say("#view: " + chr + ": " + rsi_hot_last_error(ctx) + "\n");
        ok = false;
        continue;
      }
      if (o.bamread == "device") say(bam_read_line(ctx));
      chromosome(chr, d, n);
    }
  } else if (geno_names(lines, fnames[fai_one])) {
    rsi_text_stats ts;
    const void* d = nullptr;
    int64_t n = 0;
    if (rsi_hot_load_depth_text(ctx, o.rdfile.c_str(), flens[fai_one], &ts) != RSI_OK || rsi_hot_loaded_depth(ctx, &d, &n) != RSI_OK) {
      say("#view: " + o.chr + ": " + rsi_hot_last_error(ctx) + "\n");
      ok = false;
    } else {
      rsi_inflate_stats is;
      if (rsi_hot_last_inflate_stats(ctx, &is) == RSI_OK) say(inflate_line(is));
      chromosome(fnames[fai_one], d, n);
    }
  }
  convert_figures(psfiles, log);
  for (const rsipinh::CnvLine& l : lines) {
    bool met = false;
    for (const std::string& c : seen) met = met || same_chrom(l.cell[0], c);
    if (!met) say("#view: " + l.cell[0] + " is not in the input: no figure for " + l.cell[0] + ":" + l.cell[1] + "-" + l.cell[2] + "\n");
  }
  return ok ? 0 : 1;
}

}  // namespace

int main(int argc, char** argv) {
  // one hardware queue per stream of a pool (the runtime's default of 4 puts unrelated chromosomes in line behind each other);
  // read when the HIP runtime initialises, so it has to be decided before the first HIP call.  A lower value found in the
  // environment is raised to 32; RSI_HOT_HW_QUEUES=keep or =N is the caller's say (rsi_hot_process_setup, rsi_hot.h)
  rsi_hot_process_setup();
  Options o;
  parse(argc, argv, o);
  if (o.function == "stat" || o.function == "pin") return run_cnvlist(o);
  if (o.function == "depth") return run_depth(o, argc, argv);
  if (o.function == "view") return run_view(o, argc, argv);
  if (o.plots != "host" && o.plots != "device") { std::cerr << "rsicnv: -plots " << o.plots << ": expected device or host" << std::endl; return 1; }
  std::vector<rsipinh::CnvLine> geno_lines;
  if (o.function == "geno") {   // refused where it cannot work, before any output
    if (o.cnvfile.empty()) { std::cerr << "rsicnv geno: need a list of regions (-v CNVFILE)" << std::endl; return 1; }
    if (o.gpus > 1) { std::cerr << "rsicnv geno: -gpus: a CNV list runs on one device (-gpu INT picks it)" << std::endl; return 1; }
    if (!o.trackfile.empty() || !o.bintrackfile.empty()) { std::cerr << "rsicnv geno: -track / -bintrack: geno writes no tracks (run rsi for them)" << std::endl; return 1; }
    if (!(o.ploidy > 0)) { std::cerr << "rsicnv geno: -ploidy: expected a positive number" << std::endl; return 1; }
    if (!rsipinh::read_cnvlist(o.cnvfile, {}, geno_lines, std::cerr)) return 0;   // as stat / pin: the reference says so and exits with 0
    o.geno = &geno_lines;
    o.plot = false;
    o.function = "rsi";
  }
  if (o.function != "rsi") {
    std::cerr << "rsicnv " << o.function << ": not part of the accelerated read-depth path in this build" << std::endl;
    return 0;
  }
  const bool from_bam = !o.bamfile.empty();
  // bedGraph (-dformat, else the file's name): refused where it has no meaning, before any output or device work
  if (!o.dformat.empty() && o.dformat != "depth" && o.dformat != "bedgraph") {
    std::cerr << "rsicnv: -dformat " << o.dformat << ": expected depth or bedgraph" << std::endl;
    return 1;
  }
  const bool bedgraph = !from_bam && !o.rdfile.empty() && (o.dformat.empty() ? is_bedgraph_name(o.rdfile) : o.dformat == "bedgraph");
  const bool bed_one = bedgraph && o.chr != "1-22XY";   // -c RNAME: that chromosome's lines alone
  if (bedgraph) {
    if (o.samples_given) { std::cerr << "rsicnv: -samples: a bedGraph depth file has one depth column (a cohort bedGraph is not read)" << std::endl; return 1; }
    if (o.gpus > 1) { std::cerr << "-gpus: a whole-genome depth file runs on one device (-gpu INT picks it)" << std::endl; return 1; }
    if (bed_one) {
      std::vector<std::string> fnames;
      std::vector<int64_t> flens;
      if (!read_fai(o.reffile, fnames, flens)) return 1;
      size_t k = 0;
      while (k < fnames.size() && fnames[k] != o.chr && fnames[k] != "chr" + o.chr) ++k;
      if (k == fnames.size()) { std::cerr << "rsicnv: " << o.chr << " not found in fai index" << std::endl; return 1; }
      // -dindex: the index that says where RNAME's members are; without one the whole file is inflated
      if (o.dindex != "none") {
        unsigned char head[4] = {0, 0, 0, 0};
        FILE* f = fopen(o.rdfile.c_str(), "rb");
        const bool bgzf = f && fread(head, 1, 4, f) == 4 && head[0] == 0x1f && head[1] == 0x8b && head[2] == 8 && (head[3] & 4);
        if (f) fclose(f);
        if (!o.dindex.empty()) o.dindex_path = o.dindex;   // named: used, or refused by the reader when it cannot be
        else if (bgzf) for (const char* ext : {".tbi", ".csi"}) if (o.dindex_path.empty() && access((o.rdfile + ext).c_str(), R_OK) == 0) o.dindex_path = o.rdfile + ext;
      }
      // a file without lines for RNAME is found by the one pass of the reader (run_genome: exit 1, no output); a host pass
      // in front of it would read the text once more, up to RNAME's first line or through the whole file
    }
  }
  if (!o.dindex.empty() && o.dindex != "none" && !bed_one) {
    std::cerr << "rsicnv: -dindex: an index serves -d FILE -c RNAME with a bedGraph FILE in BGZF only" << std::endl;
    return 1;
  }
  if (!o.bamread.empty() && o.bamread != "device" && o.bamread != "host") {
    std::cerr << "rsicnv: -bamread " << o.bamread << ": expected device or host" << std::endl;
    return 1;
  }
  if (!o.pairs.empty() && o.pairs != "device" && o.pairs != "host") {
    std::cerr << "rsicnv: -pairs " << o.pairs << ": expected device or host" << std::endl;
    return 1;
  }
  if (!o.bamread.empty() && !from_bam) {
    std::cerr << "rsicnv: -bamread device|host: there is no BAM file to read (-b BAMFILE)" << std::endl;
    return 1;
  }
  // -refread, -refindex: the reference's format comes from its first bytes; BGZF goes through the device reader, plain text
  // through read_fasta unless -refread device asks otherwise; plain gzip is refused (rsi_ref_open says how to recompress it)
  if (!o.refread.empty() && o.refread != "device" && o.refread != "host") {
    std::cerr << "rsicnv: -refread " << o.refread << ": expected device or host" << std::endl;
    return 1;
  }
  RefTotals ref_totals;
  std::vector<std::unique_ptr<RefReader>> ref_readers;   // one per device in use; [0] serves -gpu
  {
    unsigned char head[2] = {0, 0};
    FILE* f = fopen(o.reffile.c_str(), "rb");
    const bool compressed = f && fread(head, 1, 2, f) == 2 && head[0] == 0x1f && head[1] == 0x8b;
    if (f) fclose(f);
    if (compressed || o.refread == "device") {
      std::string err;
      ref_readers.emplace_back(new RefReader);
      if (!ref_readers[0]->open(o, o.device, &ref_totals, err)) { std::cerr << "rsicnv: -f " << o.reffile << ": " << err << std::endl; return 1; }
      if (compressed && o.refread == "host") {
        std::cerr << "rsicnv: -refread host: " << o.reffile << " is BGZF, which the host loop cannot read: leave -refread out, or give -refread device" << std::endl;
        return 1;
      }
      o.ref_device = true;
    }
    if (!o.refindex.empty() && !(o.ref_device && rsi_ref_format(ref_readers[0]->ref) == 1)) {
      std::cerr << "rsicnv: -refindex: a .gzi serves a BGZF reference only (" << o.reffile << " is plain text)" << std::endl;
      return 1;
    }
  }
  RefReader* rr = o.ref_device ? ref_readers[0].get() : nullptr;
  // -track: refused where it cannot work, before any output or device work
  if (o.trackdepth != "raw" && o.trackdepth != "gc") {
    std::cerr << "rsicnv: -trackdepth " << o.trackdepth << ": expected raw or gc" << std::endl;
    return 1;
  }
  if (!o.trackformat.empty() && o.trackformat != "text" && o.trackformat != "bgzf") {
    std::cerr << "rsicnv: -trackformat " << o.trackformat << ": expected text or bgzf" << std::endl;
    return 1;
  }
  // BGZF by the name as -d takes it (.gz / .bgz, in any case) -- the FILE given, before -samples adds .k -- unless -trackformat says
  o.track_bgzf = o.trackformat.empty() ? gz_name(o.trackfile) : o.trackformat == "bgzf";
  o.bintrack_bgzf = o.trackformat.empty() ? gz_name(o.bintrackfile) : o.trackformat == "bgzf";
  if (o.trackindex && !((!o.trackfile.empty() && o.track_bgzf) || (!o.bintrackfile.empty() && o.bintrack_bgzf))) {
    std::cerr << "rsicnv: -trackindex: no BGZF track to index (a plain-text track has none: name FILE .gz or .bgz, or give -trackformat bgzf)" << std::endl;
    return 1;
  }
  if (o.trackindex) {   // the format ends at 2^29: a longer sequence among those this run can write (the .fai's, or -c's alone) is refused here
    const bool one_named = !o.chr.empty() && o.chr != "1-22XY";   // -c RNAME was given: that sequence alone can be written
    std::ifstream fai((o.reffile + ".fai").c_str());
    std::string line, name;
    while (std::getline(fai, line)) {
      std::istringstream iss(line);
      long long len = 0;
      if ((iss >> name >> len) && len > (1ll << 29) && (!one_named || name == o.chr || name == "chr" + o.chr || "chr" + name == o.chr)) {
        std::cerr << "rsicnv: -trackindex: " << name << " has " << len << " bases, more than 2^29 = 536870912, the limit of a tabix index" << std::endl;
        return 1;
      }
    }
  }
  if (!o.trackfile.empty()) {
    if (o.gpus > 1) { std::cerr << "rsicnv: -track: not with -gpus above 1 (the track is written by one device: -gpu INT picks it)" << std::endl; return 1; }
    if (o.trackdepth == "gc" && !o.P.gcadjust) { std::cerr << "rsicnv: -trackdepth gc: -NOGC leaves no GC-adjusted depth to save" << std::endl; return 1; }
    if (o.trackfile == o.outfile || o.trackfile == o.rdfile || o.trackfile == o.bamfile) { std::cerr << "rsicnv: -track: the track file is an input or the output file" << std::endl; return 1; }
  }
  if (o.bintrackvalue != "ratio" && o.bintrackvalue != "median") {
    std::cerr << "rsicnv: -bintrackvalue " << o.bintrackvalue << ": expected ratio or median" << std::endl;
    return 1;
  }
  if (!o.bintrackfile.empty()) {
    if (o.gpus > 1) { std::cerr << "rsicnv: -bintrack: not with -gpus above 1 (the track is written by one device: -gpu INT picks it)" << std::endl; return 1; }
    if (o.bintrackfile == o.outfile || o.bintrackfile == o.rdfile || o.bintrackfile == o.bamfile || o.bintrackfile == o.trackfile) {
      std::cerr << "rsicnv: -bintrack: the bin track file is an input, the output file or -track's file" << std::endl;
      return 1;
    }
  }
  // -x: a BED file with a bad line is refused as a whole, whichever chromosome the line names, before any output exists
  if (!o.excludefile.empty() && rsi_exclude_read_bed(o.excludefile.c_str(), "", 0, nullptr, nullptr, 0) < 0) {
    std::cerr << "rsicnv: -x: " << rsi_hot_last_error(nullptr) << std::endl;
    return 1;
  }
  std::vector<int32_t> cols;            // -samples: the cohort file's depth columns, and the header's names for them
  std::vector<std::string> sample_names;
  if (o.samples_given) {
    std::string err;
    if (!select_samples(o, cols, sample_names, err)) { std::cerr << "rsicnv: " << err << std::endl; return 1; }
  }
  // -d without -c (-c defaults to 1-22XY): a whole-genome depth file, RNAME POS DEPTH
  const bool genome = !from_bam && !o.rdfile.empty() && (o.chr == "1-22XY" || bedgraph);
  if (genome && !bedgraph) {
    const int cols = first_line_columns(o.rdfile);
    if (cols >= 0 && cols < 3) { std::cerr << "readdepth file and chromosome must be specified together" << std::endl; return usage(); }
    if (o.gpus > 1) { std::cerr << "-gpus: a whole-genome depth file runs on one device (-gpu INT picks it)" << std::endl; return 1; }
  }
  std::ofstream log((o.outfile + ".log").c_str());
  std::ostringstream hdr;
  hdr << "#command:   "; for (int i = 0; i < argc; ++i) hdr << argv[i] << " ";
  hdr << "\n#bamfile:   " << o.bamfile << "\n#rdfile:    " << o.rdfile << "\n#reffile:   " << o.reffile << "\n#chrom:     " << o.chr
      << "\n#min_mapq:  " << o.minq << "\n#min_baseQ: " << o.min_baseQ << "\n#binsize:   " << o.P.m << "\n#adjustGC:  " << o.P.gcadjust
      << "\n#output:    " << o.outfile << "\n";
  std::cerr << hdr.str(); log << hdr.str();

  // chromosomes to process: -c RNAME, or (BAM input, rsi.cpp:2114-2131) every reference of the header that is not
  // a mitochondrial / decoy name and has reads
  std::vector<std::string> todo;
  std::vector<int64_t> todo_len;
  if (!select_chromosomes(o, todo, todo_len, log)) return 0;
  const bool many = todo.size() > 1;

  // write_cnv_to_file, rsi.cpp:1592-1616: the first processed chromosome opens the file and writes the header, the others
  // append.  Rows always leave in the order of `todo` (the BAM header's), whatever ran where.
  bool wrote_header = false;
  GenoCollect geno_out(geno_lines.size());
  auto emit = [&](const std::string& chr, const ChromOutput& co) {
    std::cerr << co.log; log << co.log;
    if (o.geno) { geno_out.take(chr, co); return; }
    if (!co.populated) return;
    std::ofstream out(o.outfile.c_str(), wrote_header ? std::ios::app : std::ios::trunc);
    if (!wrote_header) {
      if (!o.rdfile.empty()) out << "#input " << o.rdfile << (genome && !bed_one ? "" : " " + chr) << std::endl;
      if (from_bam) out << "#input " << o.bamfile << std::endl;
      if (o.P.gcadjust) out << "#GC adjusted\n";
      out << kHeader << std::endl;
      wrote_header = true;
    }
    for (const std::string& r : co.rows) out << r << std::endl;
    out.close();
    std::cerr << "output written to " << o.outfile << std::endl; log << "output written to " << o.outfile << std::endl;
  };

  if (genome && !cols.empty()) {   // a cohort file: OUT.k and OUT.k.log per selected column k, OUT.log for the whole run
    auto out_k = [&](size_t j) { return o.outfile + "." + std::to_string(cols[j]); };
    for (size_t j = 0; j < cols.size(); ++j) {
      std::ostringstream l;
      l << "#sample " << cols[j] << (sample_names[j].empty() ? "" : ": " + sample_names[j]) << "\n";
      std::cerr << l.str(); log << l.str();
    }
    std::vector<std::string> chroms;
    std::vector<std::vector<ChromOutput>> outs;
    std::string err, summary;
    const bool ok = run_genome(o, cols, chroms, outs, err, summary, false, nullptr, rr);
    if (!ok) {   // no sample's output: the rows of a file that cannot be read through are not an answer
      std::cerr << "rsicnv: " << err << std::endl; log << "rsicnv: " << err << std::endl;
      for (size_t j = 0; j < cols.size(); ++j) { remove(out_k(j).c_str()); remove((out_k(j) + ".log").c_str()); }
      if (!o.trackfile.empty()) for (size_t j = 0; j < cols.size(); ++j) rsitrack::remove_parts(o.trackfile + "." + std::to_string(cols[j]), chroms.size());
      if (!o.bintrackfile.empty()) for (size_t j = 0; j < cols.size(); ++j) rsitrack::remove_parts(o.bintrackfile + "." + std::to_string(cols[j]), chroms.size());
      return 1;
    }
    bool tracks_ok = true;
    std::vector<std::vector<std::string>> geno_cn;   // `geno`: per sample, the lines' CN
    // each sample as its own genome run would write it: header, then its chromosomes until the first fatal one
    for (size_t j = 0; j < cols.size(); ++j) {
      const std::string path = out_k(j);
      std::ofstream slog((path + ".log").c_str());
      std::string h = hdr.str();
      h.replace(h.find("#output:    " + o.outfile + "\n"), 12 + o.outfile.size() + 1, "#output:    " + path + "\n");
      slog << h << "#sample " << cols[j] << (sample_names[j].empty() ? "" : ": " + sample_names[j]) << "\n";
      bool header_done = false;
      TrackParts parts;
      GenoCollect sample_out(geno_lines.size());
      for (size_t i = 0; i < chroms.size(); ++i) {
        const ChromOutput& co = outs[i][j];
        std::cerr << co.log; slog << co.log;
        parts.add(i, co);
        if (o.geno) sample_out.take(chroms[i], co);
        if (co.populated && !o.geno) {
          std::ofstream out(path.c_str(), header_done ? std::ios::app : std::ios::trunc);
          if (!header_done) {
            out << "#input " << o.rdfile << " sample " << cols[j] << (sample_names[j].empty() ? "" : " " + sample_names[j]) << std::endl;
            if (o.P.gcadjust) out << "#GC adjusted\n";
            out << kHeader << std::endl;
            header_done = true;
          }
          for (const std::string& r : co.rows) out << r << std::endl;
          out.close();
          std::cerr << "output written to " << path << std::endl; slog << "output written to " << path << std::endl;
        }
        if (co.fatal && !o.geno) break;   // (geno: a chromosome that fails leaves its lines unchanged, the others go on)
      }
      if (!finish_tracks(o, "." + std::to_string(cols[j]), parts, chroms.size(), slog)) tracks_ok = false;
      if (o.geno) {
        if (!sample_out.write(geno_lines, path, slog)) tracks_ok = false;
        geno_cn.push_back(sample_out.cn);
      }
    }
    if (o.geno) {   // OUT.matrix: one CN (or NA) per line and sample
      std::ofstream mx((o.outfile + ".matrix").c_str());
      mx << "#RNAME\tSTART\tEND\tTYPE";
      for (int32_t k : cols) mx << "\t" << k;
      mx << "\n";
      for (size_t i = 0; i < geno_lines.size(); ++i) {
        const rsipinh::CnvLine& l = geno_lines[i];
        mx << l.cell[0] << "\t" << l.cell[1] << "\t" << l.cell[2] << "\t" << l.cell[3];
        for (size_t j = 0; j < cols.size(); ++j) mx << "\t" << geno_cn[j][i];
        mx << "\n";
      }
      mx.close();
      if (!mx.good()) tracks_ok = false;
      std::cerr << "matrix written to " << o.outfile << ".matrix" << std::endl; log << "matrix written to " << o.outfile << ".matrix" << std::endl;
    }
    if (rr) summary += rr->line();
    std::cerr << summary; log << summary;
    return tracks_ok ? 0 : 1;
  }

  if (genome) {
    std::vector<std::string> chroms;
    std::vector<std::vector<ChromOutput>> outs;
    std::string err, summary;
    const bool ok = run_genome(o, cols, chroms, outs, err, summary, bedgraph, bed_one ? &o.chr : nullptr, rr);
    if (!ok) {   // nothing is written under OUT: the rows of a file that cannot be read through are not an answer
      for (const auto& co : outs) { std::cerr << co[0].log; log << co[0].log; }
      std::cerr << "rsicnv: " << err << std::endl; log << "rsicnv: " << err << std::endl;
      remove(o.outfile.c_str());
      rsitrack::remove_parts(o.trackfile, chroms.size());
      rsitrack::remove_parts(o.bintrackfile, chroms.size());
      return 1;
    }
    TrackParts parts;
    for (size_t i = 0; i < chroms.size(); ++i) {
      emit(chroms[i], outs[i][0]);
      parts.add(i, outs[i][0]);
      if (outs[i][0].fatal && !o.geno) break;
    }
    if (rr) summary += rr->line();
    std::cerr << summary; log << summary;
    if (o.geno && !geno_out.write(geno_lines, o.outfile, log)) return 1;
    return finish_tracks(o, "", parts, chroms.size(), log) ? 0 : 1;
  }

  if (o.gpus <= 0 || !many) {   // the reference's own shape: one chromosome after the other on one context
    int st = 0;
    rsi_ctx* ctx = rsi_hot_create(o.device, &st);
    if (!ctx) { std::cerr << "rsicnv: " << rsi_hot_last_error(nullptr) << std::endl; return 1; }
    TrackParts parts;
    for (size_t i = 0; i < todo.size(); ++i) {
      const std::string& chr = todo[i];
      ChromOutput co;
      co.track_index = i;
      process_chromosome(ctx, o, chr, many, co, rr);
      if (co.bad_input) {   // as the genome mode: a depth file that cannot be read through gives no output
        std::cerr << co.log; log << co.log;
        remove(o.outfile.c_str());
        rsitrack::remove_parts(o.trackfile, todo.size());
        rsitrack::remove_parts(o.bintrackfile, todo.size());
        rsi_hot_destroy(ctx);
        return 1;
      }
      emit(chr, co);
      parts.add(i, co);
      if (co.fatal && !o.geno) break;
    }
    rsi_hot_destroy(ctx);
    if (rr) { std::cerr << rr->line(); log << rr->line(); }
    if (o.geno && !geno_out.write(geno_lines, o.outfile, log)) return 1;
    return finish_tracks(o, "", parts, todo.size(), log) ? 0 : 1;
  }

  // ---- -gpus N: the iterations of the loop are independent.  Chromosomes go to devices longest first
  // (each to the least loaded one), every device gets a pool whose workers take that device's chromosomes longest first;
  // nothing is exchanged between devices but the finished rows, which the main thread writes in header order. ----
  const int ndev = std::max(1, o.gpus), nwork = std::max(1, std::min(o.workers, 32));
  // RSI_HOT_DEVICE_MAP=a,b,...: the HIP device behind logical device 0, 1, ... (default: -gpu, -gpu + 1, ...).  "0,0" runs the
  // two-device code path on a box with one GPU: the partition, the per-device pools and the ordered writer are what is tested.
  std::vector<int> devmap;
  if (const char* dm = getenv("RSI_HOT_DEVICE_MAP")) {
    std::stringstream ss(dm);
    std::string tok;
    while (std::getline(ss, tok, ',')) if (!tok.empty()) devmap.push_back(atoi(tok.c_str()));
  }
  auto physical = [&](int d) { return d < (int)devmap.size() ? devmap[(size_t)d] : o.device + d; };
  std::vector<rsi_pool*> pools;
  for (int d = 0; d < ndev; ++d) {
    int st = 0;
    rsi_pool* pl = rsi_pool_create(physical(d), nwork, &st);
    if (!pl) {
      if (d == 0) { std::cerr << "rsicnv: " << rsi_hot_last_error(nullptr) << std::endl; return 1; }
      std::cerr << "rsicnv: device " << physical(d) << " not available, using " << d << " device(s)" << std::endl;
      break;
    }
    pools.push_back(pl);
  }
  std::cerr << "rsicnv: " << todo.size() << " chromosomes over " << pools.size() << " device(s), " << nwork << " in flight each" << std::endl;
  // the device reader: a handle of its own per device (a handle belongs to the device it first loads on), shared by that device's workers
  std::vector<RefReader*> dev_reader(pools.size(), nullptr);
  for (size_t d = 0; rr && d < pools.size(); ++d) {
    if (d == 0 && physical(0) == o.device) { dev_reader[0] = rr; continue; }
    std::string err;
    ref_readers.emplace_back(new RefReader);
    if (!ref_readers.back()->open(o, physical((int)d), &ref_totals, err)) {
      std::cerr << "rsicnv: -f " << o.reffile << ": " << err << std::endl;
      for (rsi_pool* pl : pools) rsi_pool_destroy(pl);
      return 1;
    }
    dev_reader[d] = ref_readers.back().get();
  }
  std::vector<std::vector<int>> per_dev(pools.size());
  {
    std::vector<int> order(todo.size());
    for (size_t i = 0; i < todo.size(); ++i) order[i] = (int)i;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return todo_len[(size_t)a] > todo_len[(size_t)b]; });
    std::vector<int64_t> load(pools.size(), 0);
    for (int i : order) {
      size_t best = 0;
      for (size_t d = 1; d < pools.size(); ++d) if (load[d] < load[best]) best = d;
      per_dev[best].push_back(i);
      load[best] += todo_len[(size_t)i];
    }
  }
  std::vector<ChromOutput> outs(todo.size());
  for (size_t i = 0; i < todo.size(); ++i) outs[i].track_index = i;
  std::vector<std::thread> threads;
  std::vector<std::atomic<int>> next(pools.size());
  for (auto& a : next) a = 0;
  for (size_t d = 0; d < pools.size(); ++d)
    for (int w = 0; w < nwork; ++w)
      threads.emplace_back([&, d, w]() {
        rsi_ctx* ctx = rsi_pool_worker(pools[d], w);
        for (;;) {
          const int k = next[d].fetch_add(1);
          if (k >= (int)per_dev[d].size()) break;
          const int i = per_dev[d][(size_t)k];
          process_chromosome(ctx, o, todo[(size_t)i], true, outs[(size_t)i], dev_reader[d]);
        }
      });
  for (auto& t : threads) t.join();
  TrackParts parts;
  for (size_t i = 0; i < todo.size(); ++i) {
    emit(todo[i], outs[i]);
    parts.add(i, outs[i]);
  }
  for (rsi_pool* pl : pools) rsi_pool_destroy(pl);
  if (rr) { std::cerr << rr->line(); log << rr->line(); }
  if (o.geno && !geno_out.write(geno_lines, o.outfile, log)) return 1;
  return finish_tracks(o, "", parts, todo.size(), log) ? 0 : 1;   // (-track, -bintrack: one device only, -gpus 1)
}
