// covstats_host.cpp -- host twin of `goleft covstats` (goleft's covstats/covstats.go).
//
//   goleft-depth covstats [-n N] [-r BED] [-f FASTA] BAM...
//
// One row per BAM: coverage, insert-size and template-length figures and the duplicate / unmapped / proper-pair shares
// of a sample of records read in file order after the first 100 000.  The records are inflated, walked and extracted on
// the device range by range (gd_ingest_begin / _feed_fd, gd_covstats_decode), where the reference's sampling loop
// (:137-172) runs as a scan and the sampled values land in histograms; the host reads the header, the .bai (n_mapped of
// every reference's pseudo-bin, and the anchors of the walk), and turns the counts and histograms into the row
// (gdh_covstats_finish), replaying the reference's floating-point sums over its sorted arrays in order.
#include <unistd.h>
#include <zlib.h>

#include <algorithm>
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../../include/goleft_depth.h"
#include "../../../include/goleft_depth_host.h"
#include "bam_head.hpp"
#include "bam_reader.hpp"
#include "cli.hpp"
#include "gpu_ingest.hpp"
#include "sample_names.hpp"

namespace {

const char* const kHeader = "coverage\tinsert_mean\tinsert_sd\tinsert_5th\tinsert_95th\ttemplate_mean\ttemplate_sd\tpct_unmapped\t"
                            "pct_bad_reads\tpct_duplicate\tpct_proper_pair\tread_length\tbam\tsample\n";

// ---- covstats.go:21-26 ------------------------------------------------------------------------------------------
struct CArgs {
    int64_t n = 1000000;        // -n / --n
    std::string regions;        // -r / --regions
    std::string fasta;          // -f / --fasta (CRAM only: accepted and ignored)
    std::vector<std::string> bams;
};

void usage(FILE* f) { fputs("usage: covstats [--n N] [--regions REGIONS] [--fasta FASTA] BAMS [BAMS ...]\n", f); }

// strconv.Atoi: an optional sign and decimal digits, nothing else, in int64 range.
bool go_atoi(const std::string& s, int64_t* out)
{
    size_t i = 0;
    bool neg = false;
    if (i < s.size() && (s[i] == '+' || s[i] == '-')) neg = s[i++] == '-';
    if (i == s.size()) return false;
    unsigned __int128 v = 0;
    for (; i < s.size(); ++i) {
        if (s[i] < '0' || s[i] > '9') return false;
        v = v * 10 + (unsigned)(s[i] - '0');
        if (v > (unsigned __int128)INT64_MAX + 1) return false;
    }
    if (!neg && v > (unsigned __int128)INT64_MAX) return false;
    *out = neg ? (int64_t)(0 - (uint64_t)v) : (int64_t)v;
    return true;
}

// 1: help printed, 0: parsed, -1: usage error
int parse_args(int argc, const char* const* argv, CArgs* a)
{
    using gdh::cli::Args;
    Args c(argc, argv, usage);
    for (;;) {
        const Args::Kind kind = c.next();
        if (kind == Args::End) break;
        if (kind == Args::Help) return 1;
        if (kind == Args::Positional) { a->bams.push_back(c.arg); continue; }
        std::string* const text = c.key == "-r" || c.key == "--regions" ? &a->regions : c.key == "-f" || c.key == "--fasta" ? &a->fasta : nullptr;
        if (!text && c.key != "-n" && c.key != "--n") return c.fail("unknown argument %s", c.arg.c_str());
        if (!c.value()) return -1;
        if (text) *text = c.val;
        else if (!go_atoi(c.val, &a->n)) return c.fail("error processing %s: invalid integer %s", c.key.c_str(), c.val.c_str());
    }
    if (a->bams.empty()) return c.fail("bams is required");
    return 0;
}

bool ends_with(const std::string& s, const char* suf)
{
    const size_t n = strlen(suf);
    return s.size() >= n && s.compare(s.size() - n, n, suf) == 0;
}

using Header = gdh::BamHead;
using gdh::read_bam_head;

// samplename.Names (sample_names.hpp), joined as covstats prints them
std::string sample_names(const std::string& text)
{
    const std::vector<std::string> out = gdh::sample_name_list(text);
    std::string j;
    for (size_t i = 0; i < out.size(); ++i) j += (i ? "," : "") + out[i];
    return j.empty() ? "<no-read-groups>" : j;
}

// readCoverage (:36-55): the sum of end - start over the lines of a BED file (plain or gzip); a last line without a
// newline is not counted; a line without an integer 2nd and 3rd field is fatal.
bool read_coverage(const std::string& path, int64_t* out, std::string* err)
{
    gzFile f = gzopen(path.c_str(), "rb");
    if (!f) { *err = "open " + path + ": " + strerror(errno); return false; }
    std::string buf;
    char tmp[1 << 16];
    int got;
    while ((got = gzread(f, tmp, sizeof tmp)) > 0) buf.append(tmp, (size_t)got);
    const bool bad = got < 0;
    gzclose(f);
    if (bad) { *err = "read " + path + ": not a readable (gzip) file"; return false; }
    int64_t cov = 0;
    size_t p = 0;
    for (;;) {
        const size_t e = buf.find('\n', p);
        if (e == std::string::npos) break;
        const std::string line = buf.substr(p, e - p);
        p = e + 1;
        std::vector<std::string> toks;
        size_t q = 0;
        while (toks.size() < 4) {
            const size_t t = line.find('\t', q);
            if (t == std::string::npos) break;
            toks.push_back(line.substr(q, t - q));
            q = t + 1;
        }
        toks.push_back(line.substr(std::min(q, line.size())));
        int64_t s = 0, en = 0;
        if (toks.size() < 3) { *err = path + ": a line with fewer than 3 fields: " + line; return false; }
        if (!go_atoi(toks[1], &s)) { *err = "strconv.Atoi: parsing \"" + toks[1] + "\": invalid syntax"; return false; }
        if (!go_atoi(toks[2], &en)) { *err = "strconv.Atoi: parsing \"" + toks[2] + "\": invalid syntax"; return false; }
        cov += en - s;
    }
    *out = cov;
    return true;
}

// Go's %.Nf: NaN and the infinities as fmt writes them.
void put_f(std::string* o, const char* fmt, double v)
{
    char b[64];
    if (std::isnan(v)) snprintf(b, sizeof b, "NaN");
    else if (std::isinf(v)) snprintf(b, sizeof b, v > 0 ? "+Inf" : "-Inf");
    else snprintf(b, sizeof b, fmt, v);
    *o += b;
}

// A sampled array in ascending order, as runs of (value, count).
struct Sorted {
    std::vector<std::pair<int64_t, uint64_t>> runs;
    uint64_t n = 0;
    explicit Sorted(const gdh_covstats_values* v)
    {
        std::vector<int64_t> ov(v->overflow, v->overflow + v->n_overflow);
        std::sort(ov.begin(), ov.end());
        auto add = [&](int64_t x, uint64_t c) {
            if (!c) return;
            if (!runs.empty() && runs.back().first == x) runs.back().second += c;
            else runs.emplace_back(x, c);
            n += c;
        };
        size_t i = 0;
        for (; i < ov.size() && ov[i] < v->lo; ++i) add(ov[i], 1);
        for (uint64_t b = 0; b < v->n_bins; ++b) add(v->lo + (int64_t)b, v->bins[b]);
        for (; i < ov.size(); ++i) add(ov[i], 1);
    }
    int64_t at(uint64_t k) const                // the k-th element
    {
        for (const auto& r : runs) {
            if (k < r.second) return r.first;
            k -= r.second;
        }
        return 0;
    }
    // meanStd (:78-90) over the first len elements, additions in the reference's order
    void mean_std(uint64_t len, double* mean, double* sd) const
    {
        const double l = (double)len;
        double m = 0, s = 0;
        uint64_t left = len;
        for (const auto& r : runs) {
            if (!left) break;
            const uint64_t c = std::min(left, r.second);
            const double x = (double)r.first;
            for (uint64_t k = 0; k < c; ++k) m += x / l;
            left -= c;
        }
        left = len;
        for (const auto& r : runs) {
            if (!left) break;
            const uint64_t c = std::min(left, r.second);
            const double d = (double)r.first - m;
            for (uint64_t k = 0; k < c; ++k) s += d * d / l;      // math.Pow(d, 2) is d * d rounded once
            left -= c;
        }
        *mean = m;
        *sd = std::sqrt(s);
    }
    // madFilter (:57-76): the length of the kept prefix (n >= 3)
    uint64_t mad_filter(int64_t nmads) const
    {
        const uint64_t half = n / 2;
        const int64_t med = at(half);
        const uint64_t n_up = n - half - 1;
        const int64_t umad = at(half + 1 + n_up / 2) - med;
        const int64_t upper = med + nmads * umad;
        uint64_t kept = 0;                                   // elements <= upper
        for (const auto& r : runs) {
            if (r.first > upper) break;
            kept += r.second;
        }
        return kept == n ? n - 1 : kept;                     // no element above: the loop's i is the last index
    }
};

}  // namespace

extern "C" int gdh_covstats_finish(const int64_t* counts, const gdh_covstats_values* sizes, const gdh_covstats_values* inserts,
                                   const gdh_covstats_values* tlens, uint64_t mapped, int64_t genome_bases, const char* bam,
                                   const char* names, char* row, size_t cap)
{
    if (!counts || !sizes || !inserts || !tlens || !bam || !names || !row) return -1;
    const int64_t nU = counts[0], k = counts[1], nBad = counts[2], nDup = counts[3], nProper = counts[4];
    const Sorted sz(sizes), ins(inserts), tl(tlens);
    if (ins.n == 1 || ins.n == 2 || (ins.n && tl.n != ins.n)) return -2;   // madFilter panics on 1 or 2 elements
    double p_bad = 0, p_dup = (double)nDup, p_proper = (double)nProper, p_unmapped = 0, rl_mean = 0;
    int64_t max_rl = 0;
    if (sz.n > 0) {
        const double denom = (double)(k + nU);
        p_bad = (double)nBad / denom;
        p_dup = p_dup / denom;
        p_proper = p_proper / denom;
        p_unmapped = (double)nU / denom;
        double sd;
        sz.mean_std(sz.n, &rl_mean, &sd);
        max_rl = sz.runs.back().first;
    }
    double i_mean = 0, i_sd = 0, t_mean = 0, t_sd = 0;
    int64_t p5 = 0, p95 = 0;
    if (ins.n > 0) {
        volatile double l = (double)(ins.n - 1);             // (no fused multiply-add: Go on amd64 rounds twice)
        volatile double a5 = 0.05 * l, a95 = 0.95 * l;
        p5 = ins.at((uint64_t)(int64_t)(a5 + 0.5));
        p95 = ins.at((uint64_t)(int64_t)(a95 + 0.5));
        ins.mean_std(ins.mad_filter(10), &i_mean, &i_sd);
        tl.mean_std(tl.mad_filter(10), &t_mean, &t_sd);
    }
    const double coverage = (1 - p_bad) * (double)mapped * rl_mean / (double)genome_bases;
    std::string o;
    put_f(&o, "%.2f", coverage); o += '\t';
    put_f(&o, "%.2f", i_mean); o += '\t';
    put_f(&o, "%.2f", i_sd); o += '\t';
    o += std::to_string(p5) + "\t" + std::to_string(p95) + "\t";
    put_f(&o, "%.2f", t_mean); o += '\t';
    put_f(&o, "%.2f", t_sd); o += '\t';
    put_f(&o, "%.2f", 100 * p_unmapped); o += '\t';
    put_f(&o, "%.1f", 100 * p_bad); o += '\t';
    put_f(&o, "%.1f", 100 * p_dup); o += '\t';
    put_f(&o, "%.1f", 100 * p_proper); o += '\t';
    o += std::to_string(max_rl) + "\t" + bam + "\t" + names + "\n";
    if (o.size() + 1 > cap) return -3;
    memcpy(row, o.c_str(), o.size() + 1);
    return (int)o.size();
}

extern "C" int gdh_bai_mapped(const char* bam_path, int64_t* mapped, size_t cap, size_t* n_ref)
{
    if (!bam_path) return -1;
    std::vector<std::vector<uint64_t>> lin;
    std::vector<int64_t> nm;
    std::string err;
    if (!gdh::BamReader::linear_index(bam_path, &lin, &err, nullptr, nullptr, &nm)) return -1;
    if (n_ref) *n_ref = nm.size();
    for (size_t r = 0; r < nm.size() && r < cap && mapped; ++r) mapped[r] = nm[r];
    return 0;
}

namespace {

int env_int(const char* name, int64_t dflt)
{
    const char* e = getenv(name);
    return e && *e ? atoi(e) : (int)dflt;
}

using gdh::cli::now_s;

struct Timing { double list = 0, feed = 0, decode = 0, hist = 0, finish = 0; };

#define CS_CHECK(call)                                                                                     \
    do {                                                                                                   \
        const int rc_ = (call);                                                                            \
        if (rc_ != GD_OK) {                                                                                \
            fprintf(stderr, "covstats: %s: %s (%s)\n", bam.c_str(), gd_strerror(rc_), gd_last_error(ctx)); \
            (void)gd_ingest_abort(ctx);                                                                    \
            return 1;                                                                                      \
        }                                                                                                  \
    } while (0)

// One BAM -> its row on `out`.  0, or the exit code.
int one_bam(gd_ctx* ctx, const CArgs& a, const std::string& bam, int64_t skip, uint64_t range_bytes, FILE* out, Timing* tm)
{
    if (ends_with(bam, ".cram")) {
        fprintf(stderr, "covstats: %s: CRAM input is not supported (only BAM)\n", bam.c_str());
        return 1;
    }
    Header h;
    std::string err;
    if (!read_bam_head(bam, &h, &err)) { fprintf(stderr, "covstats: %s\n", err.c_str()); return 1; }
    const std::string names = sample_names(h.text);
    // the index: only for a path ending in .bam (x.bam.bai, else x.bai); a missing one is fatal
    std::vector<std::vector<uint64_t>> lin;
    std::vector<int64_t> n_mapped;
    const bool indexed = ends_with(bam, ".bam");
    if (indexed && !gdh::BamReader::linear_index(bam, &lin, &err, nullptr, nullptr, &n_mapped)) {
        fprintf(stderr, "covstats: %s: no usable index (%s.bai or %.*s.bai)%s%s\n", bam.c_str(), bam.c_str(),
                (int)(bam.size() - 4), bam.c_str(), err.empty() ? "" : ": ", err.c_str());
        return 1;
    }
    std::vector<uint64_t> anchors;
    for (const auto& v : lin) anchors.insert(anchors.end(), v.begin(), v.end());
    std::sort(anchors.begin(), anchors.end());
    anchors.erase(std::unique(anchors.begin(), anchors.end()), anchors.end());

    gdh::FileMap fm;
    if (!fm.open(bam)) { fprintf(stderr, "covstats: cannot open %s\n", bam.c_str()); return 1; }
    // the member that holds the first record
    double t0 = now_s();
    uint64_t first_voff = 0;
    bool have_first = false;
    if (!gdh::first_record_voffset(fm.fd, fm.size, h.length, &first_voff, &have_first)) { fprintf(stderr, "covstats: %s: not a BGZF file\n", bam.c_str()); return 1; }
    tm->list += now_s() - t0;
    CS_CHECK(gd_covstats_begin(ctx, a.n, skip));
    gd_covstats_counts cnt{};
    cnt.skip_left = skip;
    if (have_first && !(a.n <= 0 && skip == 0)) {
        (void)gd_set_option(ctx, GD_OPT_INGEST_RANGE_HINT, (int64_t)std::min<uint64_t>(range_bytes, fm.size));
        uint64_t voff = first_voff, want = range_bytes;
        for (;;) {
            const uint64_t beg = voff >> 16;
            const double ta = now_s();
            gdh::MemberTable mt;
            if (!gdh::list_members_serial_fd(fm.fd, beg, (size_t)std::min<uint64_t>(want, fm.size - beg), &mt) || mt.n == 0) {
                fprintf(stderr, "covstats: %s: truncated or damaged BGZF data at file offset %" PRIu64 "\n", bam.c_str(), beg);
                return 1;
            }
            const uint64_t used = mt.off[mt.n - 1] + mt.size[mt.n - 1];
            const bool last = beg + used >= fm.size;
            const double tb = now_s();
            CS_CHECK(gd_ingest_begin(ctx, used, beg, mt.n, mt.off.data(), mt.size.data(), mt.hdr.data(), mt.isize.data(), mt.crc.data()));
            CS_CHECK(gd_ingest_feed_fd(ctx, fm.fd, beg, (size_t)used));
            const double tc = now_s();
            CS_CHECK(gd_covstats_decode(ctx, voff, anchors.data(), anchors.size(), last ? 1 : 0, &cnt));
            const double td = now_s();
            tm->list += tb - ta; tm->feed += tc - tb; tm->decode += td - tc;
            if (cnt.done || last) break;
            if (cnt.resume == voff) { want *= 2; continue; }     // not one whole record in the range: a larger one
            voff = cnt.resume;
            want = range_bytes;
        }
    }
    if (cnt.skip_left > 0) fprintf(stderr, "covmed: not enough reads to sample for bam stats\n");
    // the sampled values
    const double te = now_s();
    std::vector<uint64_t> bins[3];
    std::vector<int64_t> ovf[3];
    gdh_covstats_values vals[3];
    for (int w = 0; w < 3; ++w) {
        int64_t lo = 0;
        size_t nb = 0, no = 0;
        CS_CHECK(gd_covstats_histogram(ctx, w, &lo, &nb, nullptr, nullptr, 0, &no));
        bins[w].resize(nb);
        ovf[w].resize(no);
        CS_CHECK(gd_covstats_histogram(ctx, w, &lo, &nb, bins[w].data(), ovf[w].data(), no, &no));
        vals[w] = gdh_covstats_values{lo, (uint64_t)nb, bins[w].data(), (uint64_t)no, ovf[w].data()};
    }
    const double tf = now_s();
    tm->hist += tf - te;
    // mapped (the .bai pseudo-bins) and the genome's size
    int64_t genome = 0;
    uint64_t mapped = 0;
    std::string not_found;
    for (size_t r = 0; r < h.names.size(); ++r) {
        genome += h.lengths[r];
        if (!indexed) continue;
        if (r >= n_mapped.size() || n_mapped[r] < 0) {
            if (h.names[r].find("random") == std::string::npos && h.lengths[r] > 10000)
                not_found += (not_found.empty() ? "" : ",") + h.names[r];
            continue;
        }
        mapped += (uint64_t)n_mapped[r];
    }
    if (!not_found.empty()) fprintf(stderr, "chromosomes: %s not found in %s\n", not_found.c_str(), bam.c_str());
    if (!a.regions.empty() && !read_coverage(a.regions, &genome, &err)) { fprintf(stderr, "covstats: %s\n", err.c_str()); return 1; }
    const int64_t counts[5] = {cnt.unmapped, cnt.counted, cnt.bad, cnt.dup, cnt.proper};
    std::vector<char> row(bam.size() + names.size() + 512);
    const int n = gdh_covstats_finish(counts, &vals[0], &vals[1], &vals[2], mapped, genome, bam.c_str(), names.c_str(), row.data(), row.size());
    if (n == -2) {
        fprintf(stderr, "covstats: %s: %" PRId64 " insert sizes sampled: too few for the median filter (the reference panics)\n",
                bam.c_str(), cnt.inserts);
        return 1;
    }
    if (n < 0) { fprintf(stderr, "covstats: %s: cannot format the row\n", bam.c_str()); return 1; }
    fwrite(row.data(), 1, (size_t)n, out);
    fflush(out);
    tm->finish += now_s() - tf;
    return 0;
}

int run(const CArgs& a, FILE* out)
{
    int64_t skip = 100000;                                   // skipReads (:119)
    if (const char* e = getenv("GOLEFT_COVSTATS_SKIP")) if (*e) skip = std::max<int64_t>(0, strtoll(e, nullptr, 10));
    const uint64_t range_bytes = (uint64_t)std::max(64, env_int("GOLEFT_COVSTATS_RANGE_KB", 128 << 10)) << 10;
    if (ends_with(a.bams.front(), ".cram")) {                // (refused before the device is touched)
        fprintf(stderr, "covstats: %s: CRAM input is not supported (only BAM)\n", a.bams.front().c_str());
        return 1;
    }
    gdh::cli::Device ctx;
    if (!ctx.open("covstats")) return 1;
    Timing tm;
    const double t0 = now_s();
    int r = 0;
    for (const std::string& bam : a.bams) {
        const double tb = now_s();
        r = one_bam(ctx, a, bam, skip, range_bytes, out, &tm);
        if (getenv("GOLEFT_COVSTATS_TIMING"))
            fprintf(stderr, "{\"bam\": \"%s\", \"wall_s\": %.4f}\n", bam.c_str(), now_s() - tb);
        if (r) break;
    }
    if (getenv("GOLEFT_COVSTATS_TIMING")) {
        double lib[7] = {0, 0, 0, 0, 0, 0, 0};
        (void)gd_ingest_timing(ctx, lib, 7);
        fprintf(stderr, "{\"total_s\": %.4f, \"list_members_s\": %.4f, \"begin_feed_s\": %.4f, \"decode_s\": %.4f, "
                        "\"histograms_s\": %.4f, \"finish_s\": %.4f, \"lib_read_s\": %.4f, \"lib_wait_inflate_s\": %.4f, "
                        "\"lib_walk_scan_hist_s\": %.4f}\n",
                now_s() - t0, tm.list, tm.feed, tm.decode, tm.hist, tm.finish, lib[0], lib[3], lib[4]);
    }
    return r;
}

}  // namespace

extern "C" int gdh_covstats_run(int argc, const char* const* argv, const char* out_path)
{
    return gdh::cli::run_to_output("covstats", out_path, [&](FILE* out) {
        fputs(kHeader, out);                                 // before the arguments are parsed (:224-226)
        fflush(out);
        CArgs a;
        const int p = parse_args(argc, argv, &a);
        return p > 0 ? 0 : p < 0 ? 255 : run(a, out);
    });
}

extern "C" int gdh_covstats_main(int argc, const char* const* argv) { return gdh_covstats_run(argc, argv, nullptr); }
