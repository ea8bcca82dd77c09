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
#include <zlib.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../../include/goleft_depth.h"
#include "../../../include/goleft_depth_host.h"

namespace {

struct EArgs {
    std::string scales, cnvs, input;
    bool normalize = false, has_level = false;
    double level = 0;
};

void usage_scales(FILE* f)
{
    fputs("usage: scales [--level L] MATRIX\n"
          "  MATRIX  a depthwed matrix (#chrom start end samples... and its rows), plain or gzipped\n"
          "  writes one factor per sample and line, in column order, for emdepth --scales: T / q[s], where q[s] is the 0.65\n"
          "  quantile of the sample's non-zero depths and T the middle one of them (sorted q, index N / 2)\n"
          "  --level  a finite number > 0 that replaces T (1: the factors 1 / q[s])\n", f);
}

void usage(FILE* f)
{
    fputs("usage: emdepth [--scales FILE | --normalize [--level L]] [--cnvs FILE] MATRIX\n"
          "  MATRIX  a depthwed matrix (#chrom start end samples... and its rows), plain or gzipped, already normalised\n"
          "  --scales  a file of one factor per line, in column order: every depth is multiplied by its sample's factor\n"
          "  --normalize  compute those factors here, as `scales` does: each sample's 0.65 quantile of its non-zero depths\n"
          "               carried to the middle one of them (--level L: to L)\n"
          "  --cnvs  write the CNV calls of every sample (emdepth.Cache) to FILE: sample, index, psize, sites, positions, cn, depth, log2fc\n", f);
}

// scales_cmd: the `scales` entry, which takes --level alone
int parse_args(int argc, const char* const* argv, EArgs* a, bool scales_cmd)
{
    const auto usage = [scales_cmd](FILE* f) { scales_cmd ? usage_scales(f) : ::usage(f); };
    std::vector<std::string> pos;
    for (int i = 1; i < argc; ++i) {
        std::string arg = argv[i];
        if (arg == "-h" || arg == "--help") { usage(stdout); return 1; }
        if (arg == "--") { for (++i; i < argc; ++i) pos.push_back(argv[i]); break; }
        if (arg == "--normalize" && !scales_cmd) { a->normalize = true; continue; }
        if (arg.size() > 1 && arg[0] == '-') {
            std::string key = arg, val;
            bool has_val = false;
            const size_t eq = arg.find('=');
            if (eq != std::string::npos) { key = arg.substr(0, eq); val = arg.substr(eq + 1); has_val = true; }
            if (key != "--level" && (scales_cmd || (key != "--scales" && key != "--cnvs"))) {
                fprintf(stderr, "error: unknown argument %s\n", arg.c_str());
                usage(stderr);
                return -1;
            }
            if (!has_val) {
                if (i + 1 >= argc) { fprintf(stderr, "error: missing value for %s\n", key.c_str()); usage(stderr); return -1; }
                val = argv[++i];
            }
            if (val.empty()) { fprintf(stderr, "error: empty value for %s\n", key.c_str()); usage(stderr); return -1; }
            if (key == "--level") {
                char* end = nullptr;
                a->level = strtod(val.c_str(), &end);
                if (end != val.c_str() + val.size() || !std::isfinite(a->level) || !(a->level > 0)) {
                    fprintf(stderr, "error: --level must be a finite number > 0, not '%s'\n", val.c_str());
                    usage(stderr);
                    return -1;
                }
                a->has_level = true;
                continue;
            }
            (key == "--scales" ? a->scales : a->cnvs) = val;
            continue;
        }
        pos.push_back(arg);
    }
    if (a->normalize && !a->scales.empty()) {
        fprintf(stderr, "error: --normalize computes the factors that --scales reads: give one of them\n");
        usage(stderr);
        return -1;
    }
    if (a->has_level && !a->normalize && !scales_cmd) {
        fprintf(stderr, "error: --level sets the level --normalize carries the samples to: it needs --normalize\n");
        usage(stderr);
        return -1;
    }
    if (pos.size() != 1) { fprintf(stderr, "error: one matrix is required\n"); usage(stderr); return -1; }
    a->input = pos[0];
    return 0;
}

double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// one line without its newline (and without a carriage return before it); false at the end of the file
bool read_line(gzFile f, std::string* line)
{
    line->clear();
    char buf[1 << 16];
    bool any = false;
    while (gzgets(f, buf, sizeof buf)) {
        any = true;
        const size_t n = strlen(buf);
        line->append(buf, n);
        if (n && buf[n - 1] == '\n') break;
    }
    while (!line->empty() && (line->back() == '\n' || line->back() == '\r')) line->pop_back();
    return any;
}

// a finite number >= 0 that is all of [s, e) and still finite as a float32
bool parse_factor(const char* s, const char* e, float* out)
{
    if (s == e) return false;
    const std::string t(s, e);
    char* end = nullptr;
    const double v = strtod(t.c_str(), &end);
    if (end != t.c_str() + t.size() || !std::isfinite(v) || !(v >= 0)) return false;
    const float f = (float)v;
    if (!std::isfinite(f)) return false;
    *out = f;
    return true;
}

struct Matrix {
    std::string header;
    size_t n = 0;                                // samples
    std::vector<std::string> where;              // chrom \t start \t end of each row, as read
    std::vector<long long> lineno;               // ... and the line it was read from
    std::vector<float> depths;                   // [rows][n]
};

int read_matrix(const std::string& path, Matrix* m)
{
    gzFile f = gzopen(path.c_str(), "rb");       // (reads a plain file as it is)
    if (!f) { fprintf(stderr, "emdepth: cannot open %s\n", path.c_str()); return 1; }
    struct Close { gzFile f; ~Close() { gzclose(f); } } closer{f};
    std::string line;
    long long lineno = 0;
    bool have_header = false;
    while (read_line(f, &line)) {
        ++lineno;
        if (!have_header) {
            // dcnv.go:173-175: the first line, '#...' or 'chrom...'; the samples are its fields from the fourth on
            if (line.empty() || (line[0] != '#' && line.compare(0, 5, "chrom") != 0)) {
                fprintf(stderr, "emdepth: %s: line 1 is not a '#chrom start end samples...' header\n", path.c_str());
                return 1;
            }
            size_t tabs = 0;
            for (char ch : line) tabs += ch == '\t';
            if (tabs < 3) { fprintf(stderr, "emdepth: %s: the header names no samples\n", path.c_str()); return 1; }
            m->n = tabs - 2;
            m->header = line;
            have_header = true;
            if (m->n == 2) {
                fprintf(stderr, "emdepth: %s has 2 samples: the reference's median of an even row reads b[N/2 + 1], which two values do not have (1 or 3 .. 4096 samples)\n", path.c_str());
                return 1;
            }
            if (m->n > 4096) { fprintf(stderr, "emdepth: %s has %zu samples: 1 or 3 .. 4096\n", path.c_str(), m->n); return 1; }
            continue;
        }
        if (line.empty()) continue;
        const char* p = line.c_str();
        const char* const end = p + line.size();
        size_t field = 0;
        const char* cells_at = nullptr;
        const size_t at = m->depths.size();
        m->depths.resize(at + m->n);
        for (;;) {
            const char* q = static_cast<const char*>(memchr(p, '\t', (size_t)(end - p)));
            const char* fe = q ? q : end;
            if (field == 3) cells_at = p;
            if (field >= 3 && field < 3 + m->n && !parse_factor(p, fe, &m->depths[at + field - 3])) {
                fprintf(stderr, "emdepth: %s: line %lld: column %zu is not a finite depth >= 0: '%.*s'\n", path.c_str(), lineno,
                        field + 1, (int)(fe - p), p);
                return 1;
            }
            ++field;
            if (!q) break;
            p = q + 1;
        }
        if (field != 3 + m->n) {
            fprintf(stderr, "emdepth: %s: line %lld has %zu columns, the header has %zu\n", path.c_str(), lineno, field, 3 + m->n);
            return 1;
        }
        m->where.emplace_back(line.c_str(), (size_t)(cells_at - 1 - line.c_str()));
        m->lineno.push_back(lineno);
    }
    if (!have_header) { fprintf(stderr, "emdepth: %s is empty\n", path.c_str()); return 1; }
    return 0;
}

int read_scales(const std::string& path, size_t n, std::vector<float>* out)
{
    gzFile f = gzopen(path.c_str(), "rb");
    if (!f) { fprintf(stderr, "emdepth: cannot open %s\n", path.c_str()); return 1; }
    struct Close { gzFile f; ~Close() { gzclose(f); } } closer{f};
    std::string line;
    long long lineno = 0;
    while (read_line(f, &line)) {
        ++lineno;
        size_t a = 0, b = line.size();
        while (a < b && (line[a] == ' ' || line[a] == '\t')) ++a;
        while (b > a && (line[b - 1] == ' ' || line[b - 1] == '\t')) --b;
        if (a == b) continue;
        float v;
        if (!parse_factor(line.c_str() + a, line.c_str() + b, &v)) {
            fprintf(stderr, "emdepth: %s: line %lld is not a finite factor >= 0\n", path.c_str(), lineno);
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

// all of [s, e) as a decimal uint32
bool parse_u32(const char* s, const char* e, uint32_t* out)
{
    if (s == e) return false;
    uint64_t v = 0;
    for (; s < e; ++s) {
        if (*s < '0' || *s > '9') return false;
        v = v * 10 + (uint64_t)(*s - '0');
        if (v > 0xffffffffull) return false;
    }
    *out = (uint32_t)v;
    return true;
}

// start and end of every row (emdepth.Position holds uint32 values)
int parse_positions(const std::string& path, const Matrix& m, std::vector<uint32_t>* starts, std::vector<uint32_t>* ends)
{
    const size_t rows = m.where.size();
    starts->resize(rows);
    ends->resize(rows);
    for (size_t r = 0; r < rows; ++r) {
        const std::string& w = m.where[r];
        const size_t t1 = w.find('\t'), t2 = t1 == std::string::npos ? t1 : w.find('\t', t1 + 1);
        if (t2 == std::string::npos || !parse_u32(w.c_str() + t1 + 1, w.c_str() + t2, &(*starts)[r]) ||
            !parse_u32(w.c_str() + t2 + 1, w.c_str() + w.size(), &(*ends)[r])) {
            fprintf(stderr, "emdepth: %s: line %lld: --cnvs needs start and end as decimal numbers below 2^32\n", path.c_str(),
                    m.lineno[r]);
            return 1;
        }
    }
    return 0;
}

// the header's fields from the fourth on
std::vector<std::string> sample_names(const Matrix& m)
{
    std::vector<std::string> names;
    size_t at = 0;
    for (int k = 0; k < 3; ++k) at = m.header.find('\t', at) + 1;
    for (;;) {
        const size_t q = m.header.find('\t', at);
        names.push_back(m.header.substr(at, q == std::string::npos ? q : q - at));
        if (q == std::string::npos) break;
        at = q + 1;
    }
    return names;
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
            const std::string& w = m.where[row[i]];
            const size_t t1 = w.find('\t'), t2 = w.find('\t', t1 + 1);
            if (i > a) o += ',';
            o.append(w, 0, t1);
            o += ':';
            o.append(w, t1 + 1, t2 - t1 - 1);
            o += '-';
            o.append(w, t2 + 1, std::string::npos);
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

int open_device(const char* prog, gd_ctx** ctx)
{
    int device = 0;
    if (const char* e = getenv("GOLEFT_DEVICE")) device = atoi(e);
    const int rc = gd_create(device, ctx);
    if (rc != GD_OK) {
        fprintf(stderr, "%s: no usable MI355X device (%s); this build has no CPU path\n", prog, gd_strerror(rc));
        return 1;
    }
    return 0;
}

// Every sample's factor: gd_sample_medians over the whole matrix, then N values of host work in float64.  The level T is
// the middle median, sorted(med)[N / 2] -- the centre the reference's own scalers use (gmean, dcnv/scalers/scalers.go:
// 126-130) -- or --level.  med and nonzero are left for the caller; secs: upload, kernels, read-back, passes.
int sample_scales(const char* prog, gd_ctx* ctx, const EArgs& a, const Matrix& m, std::vector<float>* scale,
                  std::vector<float>* med, std::vector<uint64_t>* nonzero, double* secs)
{
    const size_t N = m.n, rows = m.where.size();
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

int run_scales(const EArgs& a, FILE* out)
{
    Matrix m;
    if (int rc = read_matrix(a.input, &m)) return rc;
    gd_ctx* ctx = nullptr;
    if (int rc = open_device("scales", &ctx)) return rc;
    std::vector<float> scale, med;
    std::vector<uint64_t> nonzero;
    double secs[4] = {0, 0, 0, 0};
    const int rc = sample_scales("scales", ctx, a, m, &scale, &med, &nonzero, secs);
    gd_destroy(ctx);
    if (rc) return rc;
    const std::vector<std::string> names = sample_names(m);
    std::string o;
    char buf[64];
    for (size_t s = 0; s < m.n; ++s) {
        fprintf(stderr, "%s\t%.9g\t%llu\n", names[s].c_str(), (double)med[s], (unsigned long long)nonzero[s]);
        snprintf(buf, sizeof buf, "%.9g\n", (double)scale[s]);
        o += buf;
    }
    if (fwrite(o.data(), 1, o.size(), out) != o.size() || fflush(out) != 0) { fprintf(stderr, "scales: error writing the factors\n"); return 1; }
    if (getenv("GOLEFT_EMDEPTH_TIMING"))
        fprintf(stderr, "{\"rows\": %zu, \"samples\": %zu, \"medians_upload_s\": %.4f, \"medians_kernels_s\": %.4f, "
                        "\"medians_readback_s\": %.4f, \"medians_passes\": %d}\n",
                m.where.size(), m.n, secs[0], secs[1], secs[2], (int)secs[3]);
    return 0;
}

int apply_scales(Matrix* m, const std::vector<float>& scale)
{
    const size_t N = m->n, rows = m->where.size();
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
    const size_t N = m.n, rows = m.where.size();
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
    gd_ctx* ctx = nullptr;
    if (int rc = open_device("emdepth", &ctx)) return rc;
    double med_secs[4] = {0, 0, 0, 0};
    if (a.normalize) {
        // the matrix goes up once for the medians and again, scaled, in its blocks
        std::vector<float> scale, med;
        std::vector<uint64_t> nonzero;
        int rc = sample_scales("emdepth", ctx, a, m, &scale, &med, &nonzero, med_secs);
        if (rc == 0) rc = apply_scales(&m, scale);
        if (rc) { gd_destroy(ctx); return rc; }
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
            gd_destroy(ctx);
            return 1;
        }
        if (format_cnvs(ctx, m, n_cnvs, n_members, &cnv_text) != 0) { gd_destroy(ctx); return 1; }
        (void)gd_emcnv_timing(ctx, cnv_lib, 4);
    }
    for (size_t r0 = 0; !cnvs && r0 < rows; r0 += block) {
        const size_t nb = std::min(block, rows - r0);
        const int rc = gd_emdepth(ctx, m.depths.data() + r0 * N, nb, (int)N, nullptr, nullptr, cn.data() + r0 * N, nullptr);
        if (rc != GD_OK) {
            fprintf(stderr, "emdepth: gd_emdepth: %s (%s)\n", gd_strerror(rc), gd_last_error(ctx));
            gd_destroy(ctx);
            return 1;
        }
        double t[3] = {0, 0, 0};
        (void)gd_emdepth_timing(ctx, t, 3);
        for (int k = 0; k < 3; ++k) lib[k] += t[k];
    }
    gd_destroy(ctx);
    const double t_write0 = now_s();
    std::string o = m.header;
    o += '\n';
    for (size_t r = 0; r < rows; ++r) {
        o += m.where[r];
        for (size_t s = 0; s < N; ++s) { o += '\t'; o += (char)('0' + cn[r * N + s]); }     // 0 .. 9
        o += '\n';
    }
    if (fwrite(o.data(), 1, o.size(), out) != o.size() || fflush(out) != 0) { fprintf(stderr, "emdepth: error writing the rows\n"); return 1; }
    if (cnvs) {                                  // after the rows: a run that fails leaves no calls file behind
        const double t0 = now_s();
        if (int rc = write_text(a.cnvs, cnv_text)) return rc;
        t_cnv_write = now_s() - t0;
    }
    if (timing && a.normalize)
        fprintf(stderr, "{\"rows\": %zu, \"samples\": %zu, \"medians_upload_s\": %.4f, \"medians_kernels_s\": %.4f, "
                        "\"medians_readback_s\": %.4f, \"medians_passes\": %d}\n",
                rows, N, med_secs[0], med_secs[1], med_secs[2], (int)med_secs[3]);
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

}  // namespace

extern "C" int gdh_emdepth_run(int argc, const char* const* argv, const char* out_path)
{
    EArgs a;
    const int p = parse_args(argc, argv, &a, false);
    if (p > 0) return 0;
    if (p < 0) return 255;
    FILE* out = stdout;
    if (out_path) {
        out = fopen(out_path, "w");
        if (!out) { fprintf(stderr, "emdepth: cannot create %s\n", out_path); return 1; }
    }
    int r = run(a, out);
    if (out_path) { if (fclose(out) != 0 && r == 0) r = 1; }
    return r;
}

extern "C" int gdh_emdepth_main(int argc, const char* const* argv) { return gdh_emdepth_run(argc, argv, nullptr); }

extern "C" int gdh_scales_run(int argc, const char* const* argv, const char* out_path)
{
    EArgs a;
    const int p = parse_args(argc, argv, &a, true);
    if (p > 0) return 0;
    if (p < 0) return 255;
    FILE* out = stdout;
    if (out_path) {
        out = fopen(out_path, "w");
        if (!out) { fprintf(stderr, "scales: cannot create %s\n", out_path); return 1; }
    }
    int r = run_scales(a, out);
    if (out_path) { if (fclose(out) != 0 && r == 0) r = 1; }
    return r;
}

extern "C" int gdh_scales_main(int argc, const char* const* argv) { return gdh_scales_run(argc, argv, nullptr); }
