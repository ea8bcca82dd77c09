// depth_matrix.hpp -- the text of a depthwed matrix, as `depthwed` writes it and dcnv reads it (dcnv/dcnv.go:153-186): a
// `#chrom start end samples...` header and rows of chrom, start, end and one depth per sample.  The reader every matrix
// command uses (emdepth, scales, debias) and the two writers of their rows.  Cells are parsed with strtod and narrowed to
// float32; the whole file is read and checked.  The reader's messages carry the `emdepth:` prefix in every command.
#pragma once
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <string_view>
#include <vector>

#include "cli.hpp"

namespace gdh {

// a finite number >= 0 that is all of [s, e) and still finite as a float32
inline bool parse_factor(const char* s, const char* e, float* out)
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
    std::vector<uint32_t> tab1, tab2;            // ... where its two tabs are
    std::vector<long long> lineno;               // ... and the line it was read from
    std::vector<float> depths;                   // [rows][n]

    size_t rows() const { return where.size(); }
    std::string_view chrom(size_t r) const { return std::string_view(where[r]).substr(0, tab1[r]); }
    std::string_view start(size_t r) const { return std::string_view(where[r]).substr(tab1[r] + 1, tab2[r] - tab1[r] - 1); }
    std::string_view end(size_t r) const { return std::string_view(where[r]).substr(tab2[r] + 1); }
};

inline int read_matrix(const std::string& path, Matrix* m)
{
    cli::Lines in;
    if (!in.open(path)) { fprintf(stderr, "emdepth: cannot open %s\n", path.c_str()); return 1; }
    std::string line;
    bool have_header = false;
    while (in.next(&line)) {
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
        const char* at_field[4] = {p, p, p, p};  // where fields 0 .. 3 begin
        const size_t at = m->depths.size();
        m->depths.resize(at + m->n);
        for (;;) {
            const char* q = static_cast<const char*>(memchr(p, '\t', (size_t)(end - p)));
            const char* fe = q ? q : end;
            if (field <= 3) at_field[field] = p;
            if (field >= 3 && field < 3 + m->n && !parse_factor(p, fe, &m->depths[at + field - 3])) {
                fprintf(stderr, "emdepth: %s: line %lld: column %zu is not a finite depth >= 0: '%.*s'\n", path.c_str(), in.lineno,
                        field + 1, (int)(fe - p), p);
                return 1;
            }
            ++field;
            if (!q) break;
            p = q + 1;
        }
        if (field != 3 + m->n) {
            fprintf(stderr, "emdepth: %s: line %lld has %zu columns, the header has %zu\n", path.c_str(), in.lineno, field, 3 + m->n);
            return 1;
        }
        m->where.emplace_back(line.c_str(), (size_t)(at_field[3] - 1 - line.c_str()));
        m->tab1.push_back((uint32_t)(at_field[1] - 1 - line.c_str()));
        m->tab2.push_back((uint32_t)(at_field[2] - 1 - line.c_str()));
        m->lineno.push_back(in.lineno);
    }
    if (!have_header) { fprintf(stderr, "emdepth: %s is empty\n", path.c_str()); return 1; }
    return 0;
}

// the header's fields from the fourth on
inline std::vector<std::string> sample_names(const Matrix& m)
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

// the matrix as text: every cell as %.9g of the float32, which read_matrix takes back bit for bit
inline std::string matrix_text(const Matrix& m)
{
    std::string o = m.header;
    o += '\n';
    char buf[64];
    for (size_t r = 0; r < m.rows(); ++r) {
        o += m.where[r];
        for (size_t s = 0; s < m.n; ++s) { snprintf(buf, sizeof buf, "\t%.9g", (double)m.depths[r * m.n + s]); o += buf; }
        o += '\n';
    }
    return o;
}

// the matrix's header and row prefixes with cn[rows][n], one digit (0 .. 9) per cell
inline std::string copy_number_text(const Matrix& m, const std::vector<uint8_t>& cn)
{
    std::string o = m.header;
    o += '\n';
    for (size_t r = 0; r < m.rows(); ++r) {
        o += m.where[r];
        for (size_t s = 0; s < m.n; ++s) { o += '\t'; o += (char)('0' + cn[r * m.n + s]); }
        o += '\n';
    }
    return o;
}

}  // namespace gdh
