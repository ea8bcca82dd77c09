// emdepth_host.cpp -- copy numbers per site of a depthwed matrix: goleft's emdepth.EMDepth (emdepth/emdepth.go; DESIGN.md
// section 3.10) run on the device, row by row.
//
//   goleft-depth emdepth [--scales FILE | --normalize [--level L]] [--cnvs FILE] matrix.bed[.gz]
//   goleft-depth scales [--level L] matrix.bed[.gz]
//
// The matrix is what `depthwed` writes and dcnv reads (dcnv/dcnv.go:153-186): a `#chrom start end samples...` header and
// rows of chrom, start, end and one depth per sample.  Cells are parsed with strtod and narrowed to float32; with
// --scales (one factor per line, in column order) a cell is multiplied by its sample's factor in float32.  Nothing else is
// normalised: the reference package "does no normalization and expects incoming data to be normalized".  The whole file is
// read and checked first, then the rows go through gd_emdepth in blocks (GOLEFT_EMDEPTH_ROWS, default 65536; the output
// does not depend on it).  Output: the header, and per row chrom, start, end and one copy number per sample.
//
// With --cnvs the rows go through gd_emcnv_add instead (the same kernel, the same copy numbers, the same blocks), which
// also joins every sample's aberrant sites into CNV calls as emdepth.Cache does; FILE gets one
// line per call.  Cache knows positions, not chromosomes, so start and end must be decimal uint32 values, and a call may
// run across a chromosome boundary when the arithmetic says so: every site is written with its chromosome.
//
// `scales` reads the same matrix with the same reader and writes the factors `--scales` takes, one per line in column order:
// every sample's 0.65 quantile of its non-zero depths (dcnv's SampleMedians, dcnv/dcnv.go:108-125; gd_sample_medians on
// the device) carried to one level, scale[s] = (float)(T / med[s]) with T = sorted(med)[N / 2] or
// --level.  `emdepth --normalize` computes the same factors in-process and goes on as with --scales: the matrix is
// uploaded once for the medians and again, scaled, in its blocks.
//
//   goleft-depth debias (--gc-values FILE | --fasta ref.fa) [--window W | --moving ROWS] matrix.bed[.gz]
//   goleft-depth emdepth (--gc-values FILE | --gc-fasta ref.fa) [--gc-window W | --gc-moving ROWS] [--level L] [--cnvs FILE] matrix.bed[.gz]
//
// `debias` reads the same matrix with the same reader and writes it back with every cell divided by the "median" of its
// sample over the rows of similar covariate: dcnv's ChunkDebiaser (dcnv/debiaser/debiaser.go:125-171; gd_chunk_debias on
// the device).  The covariate is one float64 per row -- from a file, one per line in row order, or
// the GC fraction of [max(start, 250) - 250, end) of a FASTA (dcnv/dcnv.go:82-86; counted by gd_seq_stats_ex under the
// active GDH_STATS_* contract).  --window (the reference's ScoreWindow) defaults to 0.01: this project's choice, the
// reference gives none.  With --moving ROWS the divisor is instead the moving median over ROWS rows in covariate order of
// dcnv's GeneralDebiaser (debiaser.go:98-123, what dcnv's main runs with 9; gd_moving_debias, section 3.15).  Cells go out as %.9g of the float32, which the reader takes back bit for bit.  `emdepth` with a GC
// flag debiases in-process and then normalises, in the reference's order (dcnv.go:331-337): the quotients are near 1 and
// EMDepth stops on absolute thresholds, so they go back to depth scale -- the level is --level or the middle sample median
// of the matrix AS READ, the factors T / med'[s] over the medians of the debiased matrix (this project's definition).
//
//   goleft-depth debias --svd PCT [--zscore] matrix.bed[.gz]
//   goleft-depth emdepth --svd PCT [GC flags] [--level L] [--cnvs FILE] matrix.bed[.gz]
//
// `debias --svd` removes the bias nobody has a covariate for: dcnv's SVD debiaser (debiaser.go:173-200; gd_svd_debias,
// DESIGN.md section 3.16) zeroes the leading singular values of the matrix whose share of the spectrum exceeds PCT (the
// reference's MinVariancePct), at most 15; --zscore flanks it with the reference's z-score scaler (scalers.go:24-56) --
// without it the first component is the mean depth and cells may come out negative.  One stderr line carries the removed
// shares as the reference logs them.  Not with a covariate or its windows: chain the debiasers by a pipe.  `emdepth --svd`
// runs it in-process, always z-scored (emdepth refuses negative cells), after the GC debias when there is one and before
// --normalize, which it implies: the output is what `debias --svd PCT --zscore | emdepth --normalize` writes.  The spectrum
// needs every row, so this step is never tiled by GOLEFT_EMDEPTH_ROWS.
//
//   goleft-depth debias --svd PCT --log2 matrix.bed[.gz]
//   goleft-depth emdepth --svd PCT --log2 [GC flags] [--level L] [--cnvs FILE] matrix.bed[.gz]
//
// --log2 flanks the SVD debiaser with the reference's Log2 scaler instead (scalers.go:134-164):
// log2(1 + depth), every sample centred on its median over the rows, and back by max(0, 2^x - 1) -- the "- 1" and the clamp
// are this project's, the reference's UnScale returns depth + 1.  In log space a multiplicative bias is additive, and a site
// where a few samples carry a CNV is not flattened before the cut sees it, as the z-score flattens it.  Not with --zscore.
// `emdepth --svd PCT --log2` is `debias --svd PCT --log2 | emdepth --normalize`.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <string_view>
#include <vector>

#include "../../../include/goleft_depth.h"
#include "../../../include/goleft_depth_host.h"
#include "cli.hpp"
#include "depth_matrix.hpp"
#include "fasta_stats.hpp"

namespace {

using gdh::Matrix;
using gdh::cli::now_s;

struct EArgs {
    std::string scales, cnvs, input, gc_values, gc_fasta;
    bool normalize = false, has_level = false, has_window = false, has_moving = false;
    double level = 0, window = 0.01;
    int moving = 0;                              // --moving / --gc-moving: the GeneralDebiaser's window, in rows
    bool has_svd = false, zscore = false;        // --svd PCT [--zscore]: the SVD debiaser's MinVariancePct, its scaler
    bool log2 = false;                           // --log2: the Log2 scaler in the z-score's place
    double svd = 0;
    bool gc() const { return !gc_values.empty() || !gc_fasta.empty(); }
};

void usage_scales(FILE* f)
{
    fputs("usage: scales [--level L] MATRIX\n"
          "  MATRIX  a depthwed matrix (#chrom start end samples... and its rows), plain or gzipped\n"
          "  writes one factor per sample and line, in column order, for emdepth --scales: T / q[s], where q[s] is the 0.65\n"
          "  quantile of the sample's non-zero depths and T the middle one of them (sorted q, index N / 2)\n"
          "  --level  a finite number > 0 that replaces T (1: the factors 1 / q[s])\n", f);
}

void usage_debias(FILE* f)
{
    fputs("usage: debias (--gc-values FILE | --fasta REF.fa) [--window W | --moving ROWS] MATRIX\n"
          "       debias --svd PCT [--zscore | --log2] MATRIX\n"
          "  MATRIX  a depthwed matrix (#chrom start end samples... and its rows), plain or gzipped\n"
          "  writes the matrix with every cell divided by its sample's median over the rows of similar covariate (dcnv's\n"
          "  ChunkDebiaser): the rows in covariate order are cut where a value exceeds the chunk's first by more than W\n"
          "  --gc-values  the covariate: one number per line, one line per row, in row order (GC content or any other)\n"
          "  --fasta  take the GC fraction of [max(start, 250) - 250, end) of REF.fa (needs REF.fa.fai) instead\n"
          "  --window  W, a finite number > 0 (default 0.01)\n"
          "  --moving  divide by a moving median over ROWS rows in covariate order instead (dcnv's GeneralDebiaser; dcnv runs\n"
          "            it with 9): an odd number, 1 .. 255.  Not with --window\n"
          "  --svd  instead of a covariate: zero the leading singular values of the matrix whose share of the spectrum exceeds\n"
          "         PCT per cent (a finite number >= 0), at most 15 (dcnv's SVD debiaser); 2 .. 1024 samples.  The removed shares\n"
          "         go to stderr.  Not with the flags above: chain the debiasers by a pipe\n"
          "  --zscore  with --svd: z-score every row first and carry it back after (max(0, z sd + mean)); without it the first\n"
          "            component is the mean depth and cells may come out negative\n"
          "  --log2  with --svd, not with --zscore: take log2(1 + depth) and centre every sample on its median over the rows\n"
          "          first (dcnv's Log2 scaler), and carry the result back after (max(0, 2^x - 1))\n", f);
}

void usage(FILE* f)
{
    fputs("usage: emdepth [--scales FILE | --normalize [--level L] | (--gc-values FILE | --gc-fasta REF.fa) [--gc-window W | --gc-moving ROWS] [--level L]]\n"
          "               [--svd PCT [--log2]] [--cnvs FILE] MATRIX\n"
          "  MATRIX  a depthwed matrix (#chrom start end samples... and its rows), plain or gzipped, already normalised\n"
          "  --scales  a file of one factor per line, in column order: every depth is multiplied by its sample's factor\n"
          "  --normalize  compute those factors here, as `scales` does: each sample's 0.65 quantile of its non-zero depths\n"
          "               carried to the middle one of them (--level L: to L)\n"
          "  --gc-values, --gc-fasta, --gc-window, --gc-moving  first remove the bias of a per-row covariate as `debias` does (its\n"
          "               --gc-values, --fasta, --window, --moving), then --normalize: to --level, or to the middle one of the\n"
          "               sample quantiles of the matrix as read\n"
          "  --svd  after the GC debias, if any: `debias --svd PCT --zscore`, then --normalize (to --level or the middle sample quantile)\n"
          "  --log2  with --svd: `debias --svd PCT --log2` in place of --zscore\n"
          "  --cnvs  write the CNV calls of every sample (emdepth.Cache) to FILE: sample, index, psize, sites, positions, cn, depth, log2fc\n", f);
}

// a finite number > 0 that is all of val
bool parse_positive(const std::string& val, double* out)
{
    char* end = nullptr;
    *out = strtod(val.c_str(), &end);
    return end == val.c_str() + val.size() && std::isfinite(*out) && *out > 0;
}

// What a command takes: each flag by the name the command gives it, null where the flag is not its own.
struct Command {
    const char* prog;
    void (*usage)(FILE*);
    const char *normalize, *zscore, *log2;                                       // flags without a value
    const char *scales, *cnvs, *level, *svd, *gc_values, *fasta, *window, *moving;
    bool debiaser_required;                      // debias: a debiaser has to be named, and --svd stands without a covariate
};

const Command kEmdepth = {"emdepth", usage, "--normalize", nullptr, "--log2",
                          "--scales", "--cnvs", "--level", "--svd", "--gc-values", "--gc-fasta", "--gc-window", "--gc-moving", false};
const Command kScales = {"scales", usage_scales, nullptr, nullptr, nullptr,
                         nullptr, nullptr, "--level", nullptr, nullptr, nullptr, nullptr, nullptr, false};
const Command kDebias = {"debias", usage_debias, nullptr, "--zscore", "--log2",
                         nullptr, nullptr, nullptr, "--svd", "--gc-values", "--fasta", "--window", "--moving", true};

// 0, 1 after the help, -1 for a usage error, -2 for two valid flags that do not go together (exit code 1)
int parse_args(const Command& k, int argc, const char* const* argv, EArgs* a)
{
    using gdh::cli::Args;
    Args c(argc, argv, k.usage);
    const auto is = [&c](const char* name) { return name && c.key == name; };
    std::vector<std::string> pos;
    for (;;) {
        const Args::Kind kind = c.next();
        if (kind == Args::End) break;
        if (kind == Args::Help) return 1;
        if (kind == Args::Positional) { pos.push_back(c.arg); continue; }
        if (!c.has_val && (is(k.normalize) || is(k.zscore) || is(k.log2))) {
            (is(k.normalize) ? a->normalize : is(k.zscore) ? a->zscore : a->log2) = true;
            continue;
        }
        std::string* const text = is(k.scales) ? &a->scales : is(k.cnvs) ? &a->cnvs : is(k.gc_values) ? &a->gc_values : is(k.fasta) ? &a->gc_fasta : nullptr;
        if (!text && !is(k.level) && !is(k.svd) && !is(k.window) && !is(k.moving)) return c.fail("unknown argument %s", c.arg.c_str());
        if (!c.value()) return -1;
        const std::string& val = c.val;
        if (val.empty()) return c.fail("empty value for %s", c.key.c_str());
        if (text) {
            *text = val;
        } else if (is(k.moving)) {
            char* end = nullptr;
            const long v = strtol(val.c_str(), &end, 10);
            if (end != val.c_str() + val.size() || v < 1 || v > 255 || v % 2 == 0)
                return c.fail("%s must be an odd number of rows, 1 .. 255, not '%s'", c.key.c_str(), val.c_str());
            a->moving = (int)v;
            a->has_moving = true;
        } else if (is(k.svd)) {
            char* end = nullptr;
            a->svd = strtod(val.c_str(), &end);
            if (end != val.c_str() + val.size() || !std::isfinite(a->svd) || !(a->svd >= 0))
                return c.fail("--svd must be a finite share in per cent >= 0, not '%s'", val.c_str());
            a->has_svd = true;
        } else {
            const bool level = is(k.level);
            if (!parse_positive(val, level ? &a->level : &a->window))
                return c.fail("%s must be a finite number > 0, not '%s'", c.key.c_str(), val.c_str());
            (level ? a->has_level : a->has_window) = true;
        }
    }
    // (in this order: an argv that trips two of them names the first)
    if (a->normalize && !a->scales.empty()) return c.fail("--normalize computes the factors that --scales reads: give one of them");
    if (!a->gc_values.empty() && !a->gc_fasta.empty()) return c.fail("--gc-values and %s both name the covariate: give one of them", k.fasta);
    if (k.debiaser_required && a->has_svd && (a->gc() || a->has_window || a->has_moving)) {
        c.fail("--svd takes no covariate and no window: run the two debiasers one after the other, by a pipe");
        return -2;                               // (the flags are each valid)
    }
    if (a->zscore && !a->has_svd) return c.fail("--zscore is the scaler of --svd: it needs --svd PCT");
    if (a->log2 && !a->has_svd) return c.fail("--log2 is a scaler of --svd: it needs --svd PCT");
    if (a->log2 && a->zscore) return c.fail("--log2 and --zscore both name the scaler of --svd: give one of them");
    if (a->has_svd && !a->scales.empty())
        return c.fail("--svd normalises after the debiasing, as --normalize does: --scales cannot be given with it");
    if (k.debiaser_required && !a->gc() && !a->has_svd) return c.fail("the covariate is required: --gc-values FILE or --fasta REF.fa");
    if (a->gc() && !a->scales.empty())
        return c.fail("the GC flags normalise after the debiasing, as --normalize does: --scales cannot be given with them");
    if (a->has_window && !a->gc()) return c.fail("%s is the window of the debiasing: it needs --gc-values or %s", k.window, k.fasta);
    if (a->has_moving && !a->gc()) return c.fail("%s is the window of the debiasing: it needs --gc-values or %s", k.moving, k.fasta);
    if (a->has_moving && a->has_window) {
        c.fail("%s and %s choose the debiaser: give one of them", k.window, k.moving);
        return -2;                               // (the two flags are each valid)
    }
    if ((a->gc() || a->has_svd) && k.normalize) a->normalize = true;          // emdepth: a debiaser implies --normalize
    if (a->has_level && !a->normalize && k.normalize) return c.fail("--level sets the level --normalize carries the samples to: it needs --normalize");
    if (pos.size() != 1) return c.fail("one matrix is required");
    a->input = pos[0];
    return 0;
}

int read_scales(const std::string& path, size_t n, std::vector<float>* out)
{
    gdh::cli::Lines in;
    if (!in.open(path)) { fprintf(stderr, "emdepth: cannot open %s\n", path.c_str()); return 1; }
    std::string line;
    while (in.next(&line)) {
        size_t a = 0, b = line.size();
        while (a < b && (line[a] == ' ' || line[a] == '\t')) ++a;
        while (b > a && (line[b - 1] == ' ' || line[b - 1] == '\t')) --b;
        if (a == b) continue;
        float v;
        if (!gdh::parse_factor(line.c_str() + a, line.c_str() + b, &v)) {
            fprintf(stderr, "emdepth: %s: line %lld is not a finite factor >= 0\n", path.c_str(), in.lineno);
            return 1;
        }
        out->push_back(v);
    }
    if (out->size() != n) {
        fprintf(stderr, "emdepth: %s has %zu factors, the matrix has %zu samples\n", path.c_str(), out->size(), n);
        return 1;
    }
    return 0;
}

// all of t as a decimal uint32
bool parse_u32(std::string_view t, uint32_t* out)
{
    if (t.empty()) return false;
    uint64_t v = 0;
    for (const char ch : t) {
        if (ch < '0' || ch > '9') return false;
        v = v * 10 + (uint64_t)(ch - '0');
        if (v > 0xffffffffull) return false;
    }
    *out = (uint32_t)v;
    return true;
}

// start and end of every row (emdepth.Position holds uint32 values)
int parse_positions(const std::string& path, const Matrix& m, std::vector<uint32_t>* starts, std::vector<uint32_t>* ends)
{
    const size_t rows = m.rows();
    starts->resize(rows);
    ends->resize(rows);
    for (size_t r = 0; r < rows; ++r) {
        if (!parse_u32(m.start(r), &(*starts)[r]) || !parse_u32(m.end(r), &(*ends)[r])) {
            fprintf(stderr, "emdepth: %s: line %lld: --cnvs needs start and end as decimal numbers below 2^32\n", path.c_str(),
                    m.lineno[r]);
            return 1;
        }
    }
    return 0;
}

// %.2f as Go prints it: the infinities are +Inf and -Inf
void append_fc(std::string* o, float v)
{
    if (std::isinf(v)) { *o += v > 0 ? "+Inf" : "-Inf"; return; }
    char buf[64];
    snprintf(buf, sizeof buf, "%.2f", (double)v);
    *o += buf;
}

// the calls gd_emcnv_finish left as the text of the --cnvs file, one line each, in (emit row, sample) order
int format_cnvs(gd_ctx* ctx, const Matrix& m, uint64_t n_cnvs, uint64_t n_members, std::string* text)
{
    std::vector<uint32_t> sample(n_cnvs), psize(n_cnvs), row(n_members);
    std::vector<uint64_t> off(n_cnvs + 1);
    std::vector<float> depth(n_members), fc(n_members);
    std::vector<uint8_t> cn(n_members);
    const int rc = gd_emcnv_read(ctx, sample.data(), psize.data(), nullptr, off.data(), row.data(), depth.data(), cn.data(), fc.data());
    if (rc != GD_OK) { fprintf(stderr, "emdepth: gd_emcnv_read: %s (%s)\n", gd_strerror(rc), gd_last_error(ctx)); return 1; }
    const std::vector<std::string> names = sample_names(m);
    std::string& o = *text;
    o = "#sample\tindex\tpsize\tsites\tpositions\tcn\tdepth\tlog2fc\n";
    char buf[64];
    for (uint64_t k = 0; k < n_cnvs; ++k) {
        const uint64_t a = off[k], b = off[k + 1];
        o += names[sample[k]];
        snprintf(buf, sizeof buf, "\t%u\t%u\t%llu\t", sample[k], psize[k], (unsigned long long)(b - a));
        o += buf;
        for (uint64_t i = a; i < b; ++i) {
            if (i > a) o += ',';
            o.append(m.chrom(row[i]));
            o += ':';
            o.append(m.start(row[i]));
            o += '-';
            o.append(m.end(row[i]));
        }
        o += '\t';
        for (uint64_t i = a; i < b; ++i) { if (i > a) o += ','; o += (char)('0' + cn[i]); }
        o += '\t';
        for (uint64_t i = a; i < b; ++i) { if (i > a) o += ','; snprintf(buf, sizeof buf, "%.9g", (double)depth[i]); o += buf; }
        o += '\t';
        for (uint64_t i = a; i < b; ++i) { if (i > a) o += ','; append_fc(&o, fc[i]); }
        o += '\n';
    }
    return 0;
}

int write_text(const std::string& path, const std::string& o)
{
    FILE* f = fopen(path.c_str(), "w");
    if (!f) { fprintf(stderr, "emdepth: cannot create %s\n", path.c_str()); return 1; }
    const bool ok = fwrite(o.data(), 1, o.size(), f) == o.size();
    if (fclose(f) != 0 || !ok) { fprintf(stderr, "emdepth: error writing %s\n", path.c_str()); return 1; }
    return 0;
}

// Every sample's factor: gd_sample_medians over the whole matrix, then N values of host work in float64.  The level T is
// the middle median, sorted(med)[N / 2] -- the centre the reference's own scalers use (gmean, dcnv/scalers/scalers.go:
// 126-130) -- or --level.  med and nonzero are left for the caller; secs: upload, kernels, read-back, passes.  level_out
// (or null) gets T; scale may be null when T is all that is wanted.
int sample_scales(const char* prog, gd_ctx* ctx, const EArgs& a, const Matrix& m, std::vector<float>* scale,
                  std::vector<float>* med, std::vector<uint64_t>* nonzero, double* secs, double* level_out = nullptr)
{
    const size_t N = m.n, rows = m.rows();
    if (rows == 0) { fprintf(stderr, "%s: %s has no rows\n", prog, a.input.c_str()); return 1; }
    med->assign(N, 0.0f);
    nonzero->assign(N, 0);
    const int rc = gd_sample_medians(ctx, m.depths.data(), rows, (int)N, med->data(), nonzero->data());
    if (rc != GD_OK) {
        fprintf(stderr, "%s: gd_sample_medians: %s (%s)\n", prog, gd_strerror(rc), gd_last_error(ctx));
        return 1;
    }
    (void)gd_sample_medians_timing(ctx, secs, 4);
    const std::vector<std::string> names = sample_names(m);
    for (size_t s = 0; s < N; ++s)
        if ((*nonzero)[s] == 0) {
            fprintf(stderr, "%s: sample %s (column %zu) has no depth above 0: it has no factor\n", prog, names[s].c_str(), s + 4);
            return 1;
        }
    double T = a.level;
    if (!a.has_level) {
        std::vector<float> sorted(*med);
        std::sort(sorted.begin(), sorted.end());
        T = (double)sorted[N / 2];
    }
    if (level_out) *level_out = T;
    if (!scale) return 0;
    scale->resize(N);
    for (size_t s = 0; s < N; ++s) {
        const float f = (float)(T / (double)(*med)[s]);
        if (!std::isfinite(f)) {
            fprintf(stderr, "%s: sample %s (column %zu): the factor %g / %g is not finite as a float32\n", prog, names[s].c_str(),
                    s + 4, T, (double)(*med)[s]);
            return 1;
        }
        (*scale)[s] = f;
    }
    return 0;
}

void print_medians_timing(size_t rows, size_t N, const double* secs)
{
    fprintf(stderr, "{\"rows\": %zu, \"samples\": %zu, \"medians_upload_s\": %.4f, \"medians_kernels_s\": %.4f, "
                    "\"medians_readback_s\": %.4f, \"medians_passes\": %d}\n",
            rows, N, secs[0], secs[1], secs[2], (int)secs[3]);
}

int run_scales(const EArgs& a, FILE* out)
{
    Matrix m;
    if (int rc = read_matrix(a.input, &m)) return rc;
    gdh::cli::Device ctx;
    if (!ctx.open("scales")) return 1;
    std::vector<float> scale, med;
    std::vector<uint64_t> nonzero;
    double secs[4] = {0, 0, 0, 0};
    if (int rc = sample_scales("scales", ctx, a, m, &scale, &med, &nonzero, secs)) return rc;
    ctx.reset();
    const std::vector<std::string> names = sample_names(m);
    std::string o;
    char buf[64];
    for (size_t s = 0; s < m.n; ++s) {
        fprintf(stderr, "%s\t%.9g\t%llu\n", names[s].c_str(), (double)med[s], (unsigned long long)nonzero[s]);
        snprintf(buf, sizeof buf, "%.9g\n", (double)scale[s]);
        o += buf;
    }
    if (fwrite(o.data(), 1, o.size(), out) != o.size() || fflush(out) != 0) { fprintf(stderr, "scales: error writing the factors\n"); return 1; }
    if (getenv("GOLEFT_EMDEPTH_TIMING")) print_medians_timing(m.rows(), m.n, secs);
    return 0;
}

// --gc-values: one float64 per line, one line per row, in row order
int read_vals(const char* prog, const std::string& path, size_t rows, std::vector<double>* out)
{
    gdh::cli::Lines in;
    if (!in.open(path)) { fprintf(stderr, "%s: cannot open %s\n", prog, path.c_str()); return 1; }
    std::string line;
    const long long& lineno = in.lineno;
    while (in.next(&line)) {
        size_t a = 0, b = line.size();
        while (a < b && (line[a] == ' ' || line[a] == '\t')) ++a;
        while (b > a && (line[b - 1] == ' ' || line[b - 1] == '\t')) --b;
        const std::string t = line.substr(a, b - a);
        char* end = nullptr;
        const double v = t.empty() ? 0 : strtod(t.c_str(), &end);
        if (t.empty() || end != t.c_str() + t.size() || !std::isfinite(v)) {
            fprintf(stderr, "%s: %s: line %lld is not a finite number\n", prog, path.c_str(), lineno);
            return 1;
        }
        if (out->size() == rows) {
            fprintf(stderr, "%s: %s: line %lld: the matrix has only %zu rows\n", prog, path.c_str(), lineno, rows);
            return 1;
        }
        out->push_back(v);
    }
    if (out->size() != rows) {
        fprintf(stderr, "%s: %s ends after line %lld: the matrix has %zu rows\n", prog, path.c_str(), lineno, rows);
        return 1;
    }
    return 0;
}

// all of t as a decimal int64 below 2^62
bool parse_i64(std::string_view t, int64_t* out)
{
    if (t.empty()) return false;
    int64_t v = 0;
    for (const char ch : t) {
        if (ch < '0' || ch > '9' || v > ((int64_t)1 << 58)) return false;
        v = v * 10 + (int64_t)(ch - '0');
    }
    *out = v;
    return true;
}

// --fasta: the GC fraction of [max(start, 250) - 250, end) of every row (dcnv/dcnv.go:82-86), as a float64: n_gc over the
// denominator of the active GDH_STATS_* contract, 0 for an empty one.  Each chromosome goes to the device once
// (gd_seq_load), in order of first appearance; the counts are gd_seq_stats_ex's.
int fasta_vals(const char* prog, gd_ctx* ctx, const std::string& fasta, const std::string& path, const Matrix& m,
               std::vector<double>* out)
{
    gdh::FastaStats fa;
    std::string err;
    if (!fa.open(fasta, &err)) { fprintf(stderr, "%s: %s\n", prog, err.c_str()); return 1; }
    const size_t rows = m.rows();
    std::vector<std::string> chroms;             // in order of first appearance
    std::vector<std::vector<size_t>> rows_of;
    std::vector<int64_t> start(rows), end(rows);
    for (size_t r = 0; r < rows; ++r) {
        if (!parse_i64(m.start(r), &start[r]) || !parse_i64(m.end(r), &end[r])) {
            fprintf(stderr, "%s: %s: line %lld: --fasta needs start and end as decimal numbers\n", prog, path.c_str(), m.lineno[r]);
            return 1;
        }
        start[r] = std::max<int64_t>(start[r], 250) - 250;                     // dcnv.go:83-86
        const std::string_view chrom = m.chrom(r);
        size_t k = 0;
        while (k < chroms.size() && chroms[k] != chrom) ++k;
        if (k == chroms.size()) { chroms.emplace_back(chrom); rows_of.emplace_back(); }
        rows_of[k].push_back(r);
    }
    const int contract = gdh_get_stats_contract();
    out->assign(rows, 0.0);
    std::string bases;
    for (size_t k = 0; k < chroms.size(); ++k) {
        int64_t line_bases = 0;
        if (!fa.contig_bases(chroms[k], &bases, &line_bases)) {
            fprintf(stderr, "%s: chromosome %s is not in %s.fai\n", prog, chroms[k].c_str(), fasta.c_str());
            return 1;
        }
        int rc = gd_seq_load(ctx, reinterpret_cast<const uint8_t*>(bases.data()), (int64_t)bases.size());
        const size_t n = rows_of[k].size();
        std::vector<int64_t> s(n), e(n);
        for (size_t i = 0; i < n; ++i) { s[i] = start[rows_of[k][i]]; e[i] = end[rows_of[k][i]]; }
        std::vector<uint32_t> gc(n, 0), cpg(n, 0), low(n, 0), acgt(n, 0), lacgt(n, 0);
        const bool raw = (contract & GDH_STATS_CPG_RAW_LINES) && line_bases > 0 && line_bases < 0x7fffffff;
        if (rc == GD_OK)
            rc = gd_seq_stats_ex(ctx, n, s.data(), e.data(), raw ? (int32_t)line_bases : 0, gc.data(), cpg.data(), low.data(),
                                 acgt.data(), lacgt.data());
        if (rc != GD_OK) { fprintf(stderr, "%s: gd_seq_stats: %s (%s)\n", prog, gd_strerror(rc), gd_last_error(ctx)); return 1; }
        for (size_t i = 0; i < n; ++i) {
            const double tot = (contract & GDH_STATS_DENOM_ACGT) ? (double)acgt[i] : (double)(e[i] - s[i]);
            (*out)[rows_of[k][i]] = tot > 0 ? (double)gc[i] / tot : 0.0;
        }
    }
    return 0;
}

// The covariate of --gc-values or the FASTA, then gd_chunk_debias over the whole matrix: m's depths become the quotients.
// A quotient that is not finite as a float32 has no text the reader takes back: refused with its row and sample.
// secs: gd_chunk_debias_timing's seven values.
int debias_matrix(const char* prog, gd_ctx* ctx, const EArgs& a, Matrix* m, std::vector<double>* vals, double* secs)
{
    const size_t N = m->n, rows = m->rows();
    if (rows == 0) { fprintf(stderr, "%s: %s has no rows\n", prog, a.input.c_str()); return 1; }
    if (!a.gc_values.empty()) {
        if (int rc = read_vals(prog, a.gc_values, rows, vals)) return rc;
    } else if (int rc = fasta_vals(prog, ctx, a.gc_fasta, a.input, *m, vals)) {
        return rc;
    }
    std::vector<float> out(rows * N);
    if (a.has_moving) {                          // dcnv's GeneralDebiaser; secs: its four values
        const int rc = gd_moving_debias(ctx, m->depths.data(), rows, (int)N, vals->data(), a.moving, out.data(), nullptr);
        if (rc != GD_OK) { fprintf(stderr, "%s: gd_moving_debias: %s (%s)\n", prog, gd_strerror(rc), gd_last_error(ctx)); return 1; }
        (void)gd_moving_debias_timing(ctx, secs, 4);
    } else {
        const int rc = gd_chunk_debias(ctx, m->depths.data(), rows, (int)N, vals->data(), a.window, out.data(), nullptr, nullptr,
                                       nullptr, nullptr, 0);
        if (rc != GD_OK) { fprintf(stderr, "%s: gd_chunk_debias: %s (%s)\n", prog, gd_strerror(rc), gd_last_error(ctx)); return 1; }
        (void)gd_chunk_debias_timing(ctx, secs, 7);
    }
    for (size_t i = 0; i < rows * N; ++i)
        if (!std::isfinite(out[i])) {
            fprintf(stderr, "%s: row %zu, sample %zu: the debiased depth is not finite as a float32\n", prog, i / N + 1, i % N + 1);
            return 1;
        }
    m->depths.swap(out);
    return 0;
}

// the scaler the flags name; `none` where they name none
int svd_scaler(const EArgs& a, int none) { return a.log2 ? GD_SVD_SCALER_LOG2 : a.zscore ? GD_SVD_SCALER_ZSCORE : none; }

// gd_svd_debias_scaled over the whole matrix (scaler: a GD_SVD_SCALER_*): m's depths become the result.  The stderr line is the reference's log line
// (debiaser.go:186-192: the shares of the removed singular values, %.2f), then their number.  secs: gd_svd_debias_timing's
// five values, then n.
int svd_matrix(const char* prog, gd_ctx* ctx, const EArgs& a, int scaler, Matrix* m, double* secs)
{
    const size_t N = m->n, rows = m->rows();
    if (rows == 0) { fprintf(stderr, "%s: %s has no rows\n", prog, a.input.c_str()); return 1; }
    std::vector<float> out(rows * N);
    std::vector<double> s(std::min(rows, N));
    int n = 0;
    const int rc = gd_svd_debias_scaled(ctx, m->depths.data(), rows, (int)N, a.svd, scaler, out.data(), s.data(), &n, nullptr);
    if (rc != GD_OK) { fprintf(stderr, "%s: gd_svd_debias_scaled: %s (%s)\n", prog, gd_strerror(rc), gd_last_error(ctx)); return 1; }
    (void)gd_svd_debias_timing(ctx, secs, 5);
    secs[5] = (double)n;
    double sum = 0;
    for (double v : s) sum += v;
    std::string line = "variance:";
    char buf[64];
    for (int k = 0; k < n; ++k) { snprintf(buf, sizeof buf, " %.2f", 100.0 * s[(size_t)k] / sum); line += buf; }
    fprintf(stderr, "%s; n = %d\n", line.c_str(), n);
    m->depths.swap(out);
    return 0;
}

void print_svd_timing(size_t rows, size_t N, const double* secs)
{
    fprintf(stderr, "{\"rows\": %zu, \"samples\": %zu, \"svd_upload_s\": %.4f, \"svd_gram_s\": %.4f, \"svd_eigen_s\": %.4f, "
                    "\"svd_project_s\": %.4f, \"svd_readback_s\": %.4f, \"svd_removed\": %d}\n",
            rows, N, secs[0], secs[1], secs[2], secs[3], secs[4], (int)secs[5]);
}

void print_debias_timing(size_t rows, size_t N, const double* secs)
{
    fprintf(stderr, "{\"rows\": %zu, \"samples\": %zu, \"debias_sort_s\": %.4f, \"debias_upload_s\": %.4f, \"debias_kernels_s\": %.4f, "
                    "\"debias_readback_s\": %.4f, \"debias_chunks\": %llu, \"debias_largest_chunk\": %llu}\n",
            rows, N, secs[0], secs[1], secs[2], secs[3], (unsigned long long)secs[4], (unsigned long long)secs[5]);
}

int run_debias(const EArgs& a, FILE* out)
{
    Matrix m;
    if (int rc = read_matrix(a.input, &m)) return rc;
    gdh::cli::Device ctx;
    if (!ctx.open("debias")) return 1;
    std::vector<double> vals;
    double secs[7] = {0, 0, 0, 0, 0, 0, 0};
    if (int rc = a.has_svd ? svd_matrix("debias", ctx, a, svd_scaler(a, GD_SVD_SCALER_NONE), &m, secs) : debias_matrix("debias", ctx, a, &m, &vals, secs))
        return rc;
    ctx.reset();                                 // before the rows are formatted and written
    const size_t N = m.n, rows = m.rows();
    if (!a.gc_fasta.empty())                     // the covariate the FASTA gave, for the record: --gc-values takes it back
        for (size_t r = 0; r < rows; ++r) fprintf(stderr, "%s\t%.17g\n", m.where[r].c_str(), vals[r]);
    const std::string o = gdh::matrix_text(m);
    if (fwrite(o.data(), 1, o.size(), out) != o.size() || fflush(out) != 0) { fprintf(stderr, "debias: error writing the rows\n"); return 1; }
    if (getenv("GOLEFT_EMDEPTH_TIMING")) a.has_svd ? print_svd_timing(rows, N, secs) : print_debias_timing(rows, N, secs);
    return 0;
}

int apply_scales(Matrix* m, const std::vector<float>& scale)
{
    const size_t N = m->n, rows = m->rows();
    for (size_t r = 0; r < rows; ++r)
        for (size_t s = 0; s < N; ++s) {
            const float d = m->depths[r * N + s] * scale[s];            // float32, one rounding
            if (!std::isfinite(d)) {
                fprintf(stderr, "emdepth: row %zu, sample %zu: the scaled depth is not finite\n", r + 1, s + 1);
                return 1;
            }
            m->depths[r * N + s] = d;
        }
    return 0;
}

int run(const EArgs& a, FILE* out)
{
    const bool timing = getenv("GOLEFT_EMDEPTH_TIMING") != nullptr;
    const double t_start = now_s();
    Matrix m;
    if (int rc = read_matrix(a.input, &m)) return rc;
    const size_t N = m.n, rows = m.rows();
    if (!a.scales.empty()) {
        std::vector<float> scale;
        if (int rc = read_scales(a.scales, N, &scale)) return rc;
        if (int rc = apply_scales(&m, scale)) return rc;
    }
    const bool cnvs = !a.cnvs.empty();
    std::vector<uint32_t> starts, ends;
    if (cnvs)
        if (int rc = parse_positions(a.input, m, &starts, &ends)) return rc;
    const double t_read = now_s() - t_start;
    size_t block = 65536;
    if (const char* e = getenv("GOLEFT_EMDEPTH_ROWS")) {
        const long long v = atoll(e);
        if (v < 1) { fprintf(stderr, "emdepth: GOLEFT_EMDEPTH_ROWS must be at least 1\n"); return 1; }
        block = (size_t)v;
    }
    gdh::cli::Device ctx;
    if (!ctx.open("emdepth")) return 1;
    double med_secs[4] = {0, 0, 0, 0}, gc_secs[7] = {0, 0, 0, 0, 0, 0, 0}, svd_secs[6] = {0, 0, 0, 0, 0, 0};
    EArgs norm = a;                              // what the normalisation after a debiasing is asked for
    if (a.gc()) {
        // debias, then normalise (dcnv.go:331-337).  The quotients are near 1; the level that carries them back to depth
        // scale is --level, or the T --normalize would have chosen on the matrix as read
        int rc = 0;
        if (!a.has_level) {
            std::vector<float> med;
            std::vector<uint64_t> nonzero;
            rc = sample_scales("emdepth", ctx, a, m, nullptr, &med, &nonzero, med_secs, &norm.level);
            norm.has_level = true;
        }
        std::vector<double> vals;
        if (rc == 0) rc = debias_matrix("emdepth", ctx, a, &m, &vals, gc_secs);
        if (rc) return rc;
    }
    if (a.has_svd)                               // always scaled: the rows below take no negative cell
        if (int rc = svd_matrix("emdepth", ctx, a, svd_scaler(a, GD_SVD_SCALER_ZSCORE), &m, svd_secs)) return rc;
    if (a.normalize) {
        // the matrix goes up once for the medians and again, scaled, in its blocks
        std::vector<float> scale, med;
        std::vector<uint64_t> nonzero;
        int rc = sample_scales("emdepth", ctx, norm, m, &scale, &med, &nonzero, med_secs);
        if (rc == 0) rc = apply_scales(&m, scale);
        if (rc) return rc;
    }
    std::vector<uint8_t> cn(rows * N);
    double lib[3] = {0, 0, 0};
    double cnv_lib[4] = {0, 0, 0, 0}, t_cnv_write = 0;
    std::string cnv_text;
    uint64_t n_cnvs = 0, n_members = 0;
    if (cnvs) {
        int rc = gd_emcnv_begin(ctx, (int)N);
        for (size_t r0 = 0; rc == GD_OK && r0 < rows; r0 += block) {
            const size_t nb = std::min(block, rows - r0);
            rc = gd_emcnv_add(ctx, m.depths.data() + r0 * N, nb, starts.data() + r0, ends.data() + r0, cn.data() + r0 * N);
        }
        if (rc == GD_OK) rc = gd_emcnv_finish(ctx, &n_cnvs, &n_members);
        if (rc != GD_OK) {
            fprintf(stderr, "emdepth: gd_emcnv: %s (%s)\n", gd_strerror(rc), gd_last_error(ctx));
            return 1;
        }
        if (format_cnvs(ctx, m, n_cnvs, n_members, &cnv_text) != 0) return 1;
        (void)gd_emcnv_timing(ctx, cnv_lib, 4);
    }
    for (size_t r0 = 0; !cnvs && r0 < rows; r0 += block) {
        const size_t nb = std::min(block, rows - r0);
        const int rc = gd_emdepth(ctx, m.depths.data() + r0 * N, nb, (int)N, nullptr, nullptr, cn.data() + r0 * N, nullptr);
        if (rc != GD_OK) {
            fprintf(stderr, "emdepth: gd_emdepth: %s (%s)\n", gd_strerror(rc), gd_last_error(ctx));
            return 1;
        }
        double t[3] = {0, 0, 0};
        (void)gd_emdepth_timing(ctx, t, 3);
        for (int k = 0; k < 3; ++k) lib[k] += t[k];
    }
    ctx.reset();                                 // before the rows are formatted and written
    const double t_write0 = now_s();
    const std::string o = gdh::copy_number_text(m, cn);
    if (fwrite(o.data(), 1, o.size(), out) != o.size() || fflush(out) != 0) { fprintf(stderr, "emdepth: error writing the rows\n"); return 1; }
    if (cnvs) {                                  // after the rows: a run that fails leaves no calls file behind
        const double t0 = now_s();
        if (int rc = write_text(a.cnvs, cnv_text)) return rc;
        t_cnv_write = now_s() - t0;
    }
    if (timing && a.gc()) print_debias_timing(rows, N, gc_secs);
    if (timing && a.has_svd) print_svd_timing(rows, N, svd_secs);
    if (timing && a.normalize) print_medians_timing(rows, N, med_secs);
    if (timing && cnvs)
        fprintf(stderr, "{\"rows\": %zu, \"samples\": %zu, \"block_rows\": %zu, \"total_s\": %.4f, \"read_s\": %.4f, \"upload_s\": %.4f, "
                        "\"kernel_s\": %.4f, \"cnv_kernels_s\": %.4f, \"readback_s\": %.4f, \"write_s\": %.4f, \"cnvs\": %llu, "
                        "\"members\": %llu, \"cnvs_write_s\": %.4f}\n",
                rows, N, block, now_s() - t_start, t_read, cnv_lib[0], cnv_lib[1], cnv_lib[2], cnv_lib[3], now_s() - t_write0,
                (unsigned long long)n_cnvs, (unsigned long long)n_members, t_cnv_write);
    else if (timing)
        fprintf(stderr, "{\"rows\": %zu, \"samples\": %zu, \"block_rows\": %zu, \"total_s\": %.4f, \"read_s\": %.4f, \"upload_s\": %.4f, "
                        "\"kernel_s\": %.4f, \"readback_s\": %.4f, \"write_s\": %.4f}\n",
                rows, N, block, now_s() - t_start, t_read, lib[0], lib[1], lib[2], now_s() - t_write0);
    return 0;
}

int run_command(const Command& k, int (*run_it)(const EArgs&, FILE*), int argc, const char* const* argv, const char* out_path)
{
    EArgs a;
    const int p = parse_args(k, argc, argv, &a);
    if (p > 0) return 0;
    if (p < 0) return p == -2 ? 1 : 255;
    return gdh::cli::run_to_output(k.prog, out_path, [&](FILE* out) { return run_it(a, out); });
}

}  // namespace

extern "C" int gdh_emdepth_run(int argc, const char* const* argv, const char* out_path) { return run_command(kEmdepth, run, argc, argv, out_path); }
extern "C" int gdh_emdepth_main(int argc, const char* const* argv) { return gdh_emdepth_run(argc, argv, nullptr); }

extern "C" int gdh_scales_run(int argc, const char* const* argv, const char* out_path) { return run_command(kScales, run_scales, argc, argv, out_path); }
extern "C" int gdh_scales_main(int argc, const char* const* argv) { return gdh_scales_run(argc, argv, nullptr); }

extern "C" int gdh_debias_run(int argc, const char* const* argv, const char* out_path) { return run_command(kDebias, run_debias, argc, argv, out_path); }
extern "C" int gdh_debias_main(int argc, const char* const* argv) { return gdh_debias_run(argc, argv, nullptr); }
