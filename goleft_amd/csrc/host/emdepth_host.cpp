// emdepth_host.cpp -- copy numbers per site of a depthwed matrix: goleft's emdepth.EMDepth (emdepth/emdepth.go; DESIGN.md
// section 3.10) run on the device, row by row.
//
//   goleft-depth emdepth [--scales FILE] matrix.bed[.gz]
//
// The matrix is what `depthwed` writes and dcnv reads (dcnv/dcnv.go:153-186): a `#chrom start end samples...` header and
// rows of chrom, start, end and one depth per sample.  Cells are parsed with strtod and narrowed to float32; with
// --scales (one factor per line, in column order) a cell is multiplied by its sample's factor in float32.  Nothing else is
// normalised: the reference package "does no normalization and expects incoming data to be normalized".  The whole file is
// read and checked first, then the rows go through gd_emdepth in blocks (GOLEFT_EMDEPTH_ROWS, default 65536; the output
// does not depend on it).  Output: the header, and per row chrom, start, end and one copy number per sample.
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
    std::string scales, input;
};

void usage(FILE* f)
{
    fputs("usage: emdepth [--scales FILE] MATRIX\n"
          "  MATRIX  a depthwed matrix (#chrom start end samples... and its rows), plain or gzipped, already normalised\n"
          "  --scales  a file of one factor per line, in column order: every depth is multiplied by its sample's factor\n", f);
}

int parse_args(int argc, const char* const* argv, EArgs* a)
{
    std::vector<std::string> pos;
    for (int i = 1; i < argc; ++i) {
        std::string arg = argv[i];
        if (arg == "-h" || arg == "--help") { usage(stdout); return 1; }
        if (arg == "--") { for (++i; i < argc; ++i) pos.push_back(argv[i]); break; }
        if (arg.size() > 1 && arg[0] == '-') {
            std::string key = arg, val;
            bool has_val = false;
            const size_t eq = arg.find('=');
            if (eq != std::string::npos) { key = arg.substr(0, eq); val = arg.substr(eq + 1); has_val = true; }
            if (key != "--scales") { fprintf(stderr, "error: unknown argument %s\n", arg.c_str()); usage(stderr); return -1; }
            if (!has_val) {
                if (i + 1 >= argc) { fprintf(stderr, "error: missing value for %s\n", key.c_str()); usage(stderr); return -1; }
                val = argv[++i];
            }
            a->scales = val;
            continue;
        }
        pos.push_back(arg);
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
        for (size_t r = 0; r < rows; ++r)
            for (size_t s = 0; s < N; ++s) {
                const float d = m.depths[r * N + s] * scale[s];         // float32, one rounding
                if (!std::isfinite(d)) {
                    fprintf(stderr, "emdepth: row %zu, sample %zu: the scaled depth is not finite\n", r + 1, s + 1);
                    return 1;
                }
                m.depths[r * N + s] = d;
            }
    }
    const double t_read = now_s() - t_start;
    size_t block = 65536;
    if (const char* e = getenv("GOLEFT_EMDEPTH_ROWS")) {
        const long long v = atoll(e);
        if (v < 1) { fprintf(stderr, "emdepth: GOLEFT_EMDEPTH_ROWS must be at least 1\n"); return 1; }
        block = (size_t)v;
    }
    int device = 0;
    if (const char* e = getenv("GOLEFT_DEVICE")) device = atoi(e);
    gd_ctx* ctx = nullptr;
    {
        const int rc = gd_create(device, &ctx);
        if (rc != GD_OK) {
            fprintf(stderr, "emdepth: no usable MI355X device (%s); this build has no CPU path\n", gd_strerror(rc));
            return 1;
        }
    }
    std::vector<uint8_t> cn(rows * N);
    double lib[3] = {0, 0, 0};
    for (size_t r0 = 0; r0 < rows; r0 += block) {
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
    if (timing)
        fprintf(stderr, "{\"rows\": %zu, \"samples\": %zu, \"block_rows\": %zu, \"total_s\": %.4f, \"read_s\": %.4f, \"upload_s\": %.4f, "
                        "\"kernel_s\": %.4f, \"readback_s\": %.4f, \"write_s\": %.4f}\n",
                rows, N, block, now_s() - t_start, t_read, lib[0], lib[1], lib[2], now_s() - t_write0);
    return 0;
}

}  // namespace

extern "C" int gdh_emdepth_run(int argc, const char* const* argv, const char* out_path)
{
    EArgs a;
    const int p = parse_args(argc, argv, &a);
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
