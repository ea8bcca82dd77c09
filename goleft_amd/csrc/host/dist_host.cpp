// dist_host.cpp -- `goleft-depth dist`: the depth distribution, the summary and the threshold counts of a BAM (DESIGN.md
// section 3.22).
//
//   goleft-depth dist [-Q Q] [-c CHROM] [-b regions.bed] [--thresholds T1,T2,...] [--max-depth N] --prefix PREFIX in.bam
//
// PREFIX.dist.txt (`scope depth fraction`: the share of the scope's positions at that depth or above, from the scope's
// highest depth down to 0), PREFIX.summary.txt (`chrom length bases mean min max`), with -b PREFIX.region.dist.txt and the
// `_region` rows of the summary over the BED's lines, with --thresholds PREFIX.thresholds.bed (per BED line, its positions
// at or above each threshold).  The BAM is read as `perbase` reads it (host/bam_records.hpp), the wanted contigs are
// computed with the per-base vector kept, and gd_depth_hist and gd_region_bins count on the device: a histogram and a few
// numbers a contig cross the link, a row of counts a BED line.  The layouts follow mosdepth's files of the same names; the
// definitions are this project's.  Nothing is written before everything is computed.
#include <algorithm>
#include <cerrno>
#include <chrono>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include <unistd.h>

#include "../../../include/goleft_depth.h"
#include "../../../include/goleft_depth_host.h"
#include "bam_reader.hpp"
#include "bam_records.hpp"
#include "cli.hpp"
#include "regions.hpp"

namespace {

using gdh::cli::now_s;
using gdh::regions::Region;

struct DArgs {
    int q = 1;                          // -Q, as depth's
    int max_depth = 65535;              // --max-depth: depths above it fall into the last bin
    std::string chrom, bed, prefix, bam;
    std::vector<int32_t> thresholds;    // --thresholds
    bool have_thresholds = false;
};

void usage(FILE* f)
{
    fputs("usage: dist [-Q Q] [-c CHROM] [-b REGIONS.bed] [--thresholds T1,T2,...] [--max-depth N] --prefix PREFIX BAM\n"
          "  -Q, --q         mapping quality cutoff (default 1)\n"
          "  -c, --chrom     only this chromosome\n"
          "  -b, --bed       also over the lines of this BED file, each on its own, clipped to its chromosome\n"
          "  --thresholds    per BED line, the positions at or above each of these depths; at most 32, increasing, from 1; needs -b\n"
          "  --max-depth     depths above N count as N (1 .. 65535, default 65535)\n"
          "  --prefix        writes PREFIX.dist.txt and PREFIX.summary.txt; with -b PREFIX.region.dist.txt; with --thresholds PREFIX.thresholds.bed\n"
          "  BAM             coordinate sorted; its .bai or .csi is used when there is one\n", f);
}

// 0 ok, 1 help shown, -1 error (message printed)
int parse_args(int argc, const char* const* argv, DArgs* a)
{
    using gdh::cli::Args;
    Args c(argc, argv, usage);
    std::vector<std::string> pos;
    for (;;) {
        const Args::Kind kind = c.next();
        if (kind == Args::End) break;
        if (kind == Args::Help) return 1;
        if (kind == Args::Positional) { pos.push_back(c.arg); continue; }
        const std::string k = c.key;
        if (k != "-Q" && k != "--q" && k != "-c" && k != "--chrom" && k != "-b" && k != "--bed" && k != "--thresholds" && k != "--max-depth" && k != "--prefix")
            return c.fail("unknown argument %s", c.arg.c_str());
        if (!c.value()) return -1;
        if (k == "-Q" || k == "--q") {
            if (!gdh::regions::parse_int(c.val, &a->q)) return c.fail("%s %s: not an integer", k.c_str(), c.val.c_str());
        } else if (k == "-c" || k == "--chrom") a->chrom = c.val;
        else if (k == "-b" || k == "--bed") a->bed = c.val;
        else if (k == "--prefix") a->prefix = c.val;
        else if (k == "--max-depth") {
            if (!gdh::regions::parse_int(c.val, &a->max_depth)) return c.fail("--max-depth %s: not an integer", c.val.c_str());
            if (a->max_depth < 1 || a->max_depth > GD_DEPTH_HIST_MAX_BINS - 1)
                return c.fail("--max-depth %s: 1 .. %d", c.val.c_str(), GD_DEPTH_HIST_MAX_BINS - 1);
        } else {
            std::string why;
            if (!gdh::regions::parse_cuts(c.val, &a->thresholds, &why)) return c.fail("--thresholds %s: %s", c.val.c_str(), why.c_str());
            a->have_thresholds = true;
        }
    }
    if (pos.empty()) return c.fail("bam is required");
    if (pos.size() > 1) return c.fail("too many positional arguments at '%s'", pos[1].c_str());
    if (a->prefix.empty()) return c.fail("--prefix is required");
    if (a->have_thresholds && a->bed.empty()) return c.fail("--thresholds needs -b");
    a->bam = pos[0];
    return 0;
}

// What is known of a scope: the clamped histogram and the unclamped scalars of its positions.
struct Scope {
    std::string name;
    int64_t length = 0;                 // the contig's length, or the sum of the clipped line lengths
    int64_t bases = 0;
    int32_t min = 0, max = 0;
    bool any = false;                   // it holds a position
    std::vector<uint64_t> bins;         // [n_bins] once it holds one

    void add(const Scope& o)
    {
        length += o.length;
        if (!o.any) return;
        bases += o.bases;
        min = any ? std::min(min, o.min) : o.min;
        max = any ? std::max(max, o.max) : o.max;
        any = true;
        if (bins.size() < o.bins.size()) bins.resize(o.bins.size(), 0);
        for (size_t k = 0; k < o.bins.size(); ++k) bins[k] += o.bins[k];
    }
};

// `name depth fraction` from the scope's highest clamped depth down to 0; nothing for a scope without positions
void dist_lines(std::string* out, const Scope& s)
{
    if (!s.any) return;
    const int64_t top = std::min<int64_t>((int64_t)s.bins.size() - 1, s.max);
    uint64_t n = 0, at_or_above = 0;
    for (uint64_t b : s.bins) n += b;
    char buf[64];
    for (int64_t d = top; d >= 0; --d) {
        at_or_above += s.bins[(size_t)d];
        snprintf(buf, sizeof buf, "\t%lld\t%.6f\n", (long long)d, (double)at_or_above / (double)n);
        out->append(s.name);
        out->append(buf);
    }
}

void summary_line(std::string* out, const Scope& s)
{
    char buf[160];
    snprintf(buf, sizeof buf, "\t%lld\t%lld\t%.2f\t%d\t%d\n", (long long)s.length, (long long)s.bases,
             s.length > 0 ? (double)s.bases / (double)s.length : 0.0, s.min, s.max);
    out->append(s.name);
    out->append(buf);
}

bool write_file(const std::string& path, const std::string& text)
{
    FILE* f = fopen(path.c_str(), "w");
    if (!f) { fprintf(stderr, "dist: cannot create %s\n", path.c_str()); return false; }
    const bool ok = fwrite(text.data(), 1, text.size(), f) == text.size();
    if ((fclose(f) != 0) || !ok) { fprintf(stderr, "dist: write error on %s\n", path.c_str()); return false; }
    return true;
}

// Chunk-table entries a device call may hold (64 MB of table): a batch of BED lines ends before it would pass this.  A
// region alone is always below it.
constexpr uint64_t kBatchChunks = 1ull << 24;
// ... and the counters a gd_region_bins call may return (32 MB of rows): a batch of short lines ends there first.
constexpr uint64_t kBatchCounts = 1ull << 22;
inline uint64_t chunks_of(const Region& r) { return (uint64_t)(r.end - r.start) / 4096 + 2; }

struct Timing { double upload = 0, kernel = 0, readback = 0; uint64_t calls = 0; };

void add_timing(gd_ctx* ctx, Timing* t)
{
    double s[3] = {0, 0, 0};
    (void)gd_dist_timing(ctx, s, 3);
    t->upload += s[0]; t->kernel += s[1]; t->readback += s[2];
    ++t->calls;
}

// The histogram of regions [k0, k1) of one list into *s, a device call per batch.
int hist_scope(gd_ctx* ctx, const std::vector<Region>& regions, int n_bins, Scope* s, Timing* tm)
{
    std::vector<int32_t> tid;
    std::vector<int64_t> st, en;
    std::vector<uint64_t> bins((size_t)n_bins);
    for (size_t k0 = 0; k0 < regions.size();) {
        tid.clear(); st.clear(); en.clear();
        uint64_t chunks = 0;
        size_t k1 = k0;
        int64_t positions = 0;
        for (; k1 < regions.size() && (k1 == k0 || chunks + chunks_of(regions[k1]) <= kBatchChunks); ++k1) {
            chunks += chunks_of(regions[k1]);
            tid.push_back(regions[k1].tid); st.push_back(regions[k1].start); en.push_back(regions[k1].end);
            positions += regions[k1].end - regions[k1].start;
        }
        Scope part;
        part.length = positions;
        part.any = positions > 0;
        if (part.any) {
            int64_t sum = 0;
            const int rc = gd_depth_hist(ctx, tid.size(), tid.data(), st.data(), en.data(), n_bins, bins.data(), &sum, &part.min, &part.max);
            if (rc != GD_OK) { fprintf(stderr, "dist: gd_depth_hist failed: %s (%s)\n", gd_strerror(rc), gd_last_error(ctx)); return 1; }
            add_timing(ctx, tm);
            part.bases = sum;
            part.bins = bins;
        }
        s->add(part);
        k0 = k1;
    }
    return 0;
}

int run(const DArgs& a)
{
    const double t_begin = now_s();
    std::string err;
    gdh::BamReader bam;
    if (!bam.open(a.bam, 0, &err)) { fprintf(stderr, "dist: %s\n", err.empty() ? ("cannot open " + a.bam).c_str() : err.c_str()); return 1; }
    const auto& contigs = bam.contigs();
    std::map<std::string, int> tid_of;
    std::vector<int64_t> lens(contigs.size());
    for (size_t i = 0; i < contigs.size(); ++i) { tid_of.emplace(contigs[i].name, (int)i); lens[i] = contigs[i].length; }

    // ---- the contigs and the BED's lines -------------------------------------------------------------------------------
    if (!a.chrom.empty() && !tid_of.count(a.chrom)) { fprintf(stderr, "dist: chromosome %s is not in the BAM header\n", a.chrom.c_str()); return 1; }
    std::vector<Region> lines;
    std::vector<std::string> names;
    if (!a.bed.empty()) {
        if (int rc = gdh::regions::read_bed("dist", a.bed, tid_of, lens, &lines, &names)) return rc;
        if (!a.chrom.empty()) {
            const int32_t only = tid_of[a.chrom];
            size_t n = 0;
            for (size_t k = 0; k < lines.size(); ++k)
                if (lines[k].tid == only) { lines[n] = lines[k]; names[n] = names[k]; ++n; }
            lines.resize(n); names.resize(n);
        }
    }
    std::vector<int32_t> wanted;
    for (size_t t = 0; t < contigs.size(); ++t)
        if (a.chrom.empty() || contigs[t].name == a.chrom) wanted.push_back((int32_t)t);

    // ---- one device: records into HBM as depth reads them, then the per-base vector ------------------------------------
    gdh::rec::Shards S;
    S.v.resize(1);
    gdh::rec::Shard& sh = S.v[0];
    if (const char* e = getenv("GOLEFT_DEVICE")) sh.device = atoi(e);
    sh.wanted = wanted;
    {
        const int rc = gd_create(sh.device, &sh.ctx);
        if (rc != GD_OK) {
            sh.ctx = nullptr;
            fprintf(stderr, "dist: no usable MI355X device (%s); this build has no CPU path\n", gd_strerror(rc));
            return 1;
        }
    }
    gd_ctx* const ctx = sh.ctx;
    uint64_t n_gpu_records = 0;
    if (!wanted.empty()) {
        gd_params P;
        gd_default_params(&P);
        P.min_mapq = a.q;
        if (int rc = gdh::rec::configure_context("dist", ctx, P, lens, true, wanted)) return rc;
        const std::vector<int> shard_of(contigs.size(), 0);
        const auto t0 = std::chrono::steady_clock::now();
        gdh::rec::ReadTimes T{t0, t0, t0};
        if (int rc = gdh::rec::read_records("dist", a.bam, bam, wanted, S, shard_of, &n_gpu_records, &T)) return rc;
        const int rc = gd_compute(ctx);
        if (rc != GD_OK) { fprintf(stderr, "dist: gd_compute failed: %s (%s)\n", gd_strerror(rc), gd_last_error(ctx)); return 1; }
    }
    const double t_computed = now_s();

    // ---- the scopes: every wanted contig, and with -b the lines of every contig that has some --------------------------
    const int n_bins = a.max_depth + 1;
    Timing tm;
    std::string dist, region_dist, summary = "chrom\tlength\tbases\tmean\tmin\tmax\n", thresholds;
    Scope total, total_region;
    total.name = "total"; total_region.name = "total_region";
    std::vector<std::vector<Region>> lines_of(contigs.size());
    for (const Region& r : lines) lines_of[(size_t)r.tid].push_back(r);
    for (int32_t t : wanted) {
        Scope s;
        s.name = contigs[(size_t)t].name;
        if (int rc = hist_scope(ctx, {Region{t, 0, lens[(size_t)t]}}, n_bins, &s, &tm)) return rc;
        dist_lines(&dist, s);
        summary_line(&summary, s);
        total.add(s);
        if (lines_of[(size_t)t].empty()) continue;
        Scope rs;
        rs.name = contigs[(size_t)t].name;
        if (int rc = hist_scope(ctx, lines_of[(size_t)t], n_bins, &rs, &tm)) return rc;
        dist_lines(&region_dist, rs);
        rs.name += "_region";
        summary_line(&summary, rs);
        total_region.add(rs);
    }
    dist_lines(&dist, total);
    summary_line(&summary, total);
    if (!a.bed.empty()) {
        Scope tr = total_region;
        tr.name = "total";
        dist_lines(&region_dist, tr);
        summary_line(&summary, total_region);
    }

    // ---- --thresholds: a row per BED line, a device call per batch of lines --------------------------------------------
    if (a.have_thresholds) {
        thresholds = "#chrom\tstart\tend\tregion";
        for (int32_t t : a.thresholds) thresholds += "\t" + std::to_string(t) + "X";
        thresholds += "\n";
        const size_t nc = a.thresholds.size(), row = nc + 1;
        std::vector<int32_t> tid;
        std::vector<int64_t> st, en;
        std::vector<uint64_t> counts;
        for (size_t k0 = 0; k0 < lines.size();) {
            tid.clear(); st.clear(); en.clear();
            uint64_t chunks = 0;
            size_t k1 = k0;
            for (; k1 < lines.size() && (k1 == k0 || (chunks + chunks_of(lines[k1]) <= kBatchChunks && (k1 - k0 + 1) * row <= kBatchCounts)); ++k1) {
                chunks += chunks_of(lines[k1]);
                tid.push_back(lines[k1].tid); st.push_back(lines[k1].start); en.push_back(lines[k1].end);
            }
            counts.assign((k1 - k0) * row, 0);
            const int rc = gd_region_bins(ctx, k1 - k0, tid.data(), st.data(), en.data(), (int)nc, a.thresholds.data(), counts.data());
            if (rc != GD_OK) { fprintf(stderr, "dist: gd_region_bins failed: %s (%s)\n", gd_strerror(rc), gd_last_error(ctx)); return 1; }
            add_timing(ctx, &tm);
            std::vector<uint64_t> ge(nc);
            for (size_t k = k0; k < k1; ++k) {
                const uint64_t* c = counts.data() + (k - k0) * row;
                uint64_t above = 0;                               // the positions at or above threshold i: columns i + 1 .. nc
                for (size_t i = nc; i-- > 0;) { above += c[i + 1]; ge[i] = above; }
                thresholds += contigs[(size_t)lines[k].tid].name + "\t" + std::to_string(lines[k].start) + "\t" + std::to_string(lines[k].end) + "\t" + names[k];
                for (size_t i = 0; i < nc; ++i) thresholds += "\t" + std::to_string(ge[i]);
                thresholds += "\n";
            }
            k0 = k1;
        }
    }
    const double t_counted = now_s();

    // ---- the files -----------------------------------------------------------------------------------------------------
    if (!write_file(a.prefix + ".dist.txt", dist) || !write_file(a.prefix + ".summary.txt", summary)) return 1;
    if (!a.bed.empty() && !write_file(a.prefix + ".region.dist.txt", region_dist)) return 1;
    if (a.have_thresholds && !write_file(a.prefix + ".thresholds.bed", thresholds)) return 1;
    if (const char* e = getenv("GOLEFT_DIST_TIMING"); e && *e == '1')
        fprintf(stderr, "dist: %.4f s in all: reading + compute %.4f, counting %.4f (upload %.4f, kernels %.4f, read-back %.4f in %llu device calls), text %.4f; %s decoder\n",
                now_s() - t_begin, t_computed - t_begin, t_counted - t_computed, tm.upload, tm.kernel, tm.readback, (unsigned long long)tm.calls,
                now_s() - t_counted, n_gpu_records ? "device" : "host");
    return 0;
}

}  // namespace

extern "C" int gdh_dist_run(int argc, const char* const* argv)
{
    DArgs a;
    const int p = parse_args(argc, argv, &a);
    if (p > 0) return 0;
    if (p < 0) return 1;
    if (a.bam.size() >= 5 && a.bam.compare(a.bam.size() - 5, 5, ".cram") == 0) {
        fprintf(stderr, "dist: %s: a CRAM is not served, only a BAM\n", a.bam.c_str());
        return 1;
    }
    if (access(a.bam.c_str(), R_OK) != 0) { fprintf(stderr, "dist: cannot open %s: %s\n", a.bam.c_str(), strerror(errno)); return 1; }
    // the directory the files go to, before anything is read or a device is opened
    const size_t slash = a.prefix.rfind('/');
    const std::string dir = slash == std::string::npos ? "." : slash == 0 ? "/" : a.prefix.substr(0, slash);
    if (access(dir.c_str(), W_OK | X_OK) != 0) { fprintf(stderr, "dist: cannot write to %s: %s\n", dir.c_str(), strerror(errno)); return 1; }
    return run(a);
}

extern "C" int gdh_dist_main(int argc, const char* const* argv) { return gdh_dist_run(argc, argv); }
