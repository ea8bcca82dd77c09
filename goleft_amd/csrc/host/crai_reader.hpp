// crai_reader.hpp -- the slices of a .crai (ReadIndex, indexcov/crai/crai.go:129-192 of the reference): gzip-compressed
// text, one slice per line, six tab-separated integers (seqID, alnStart, alnSpan, containerStart, sliceStart, sliceLen).
// What `indexcov` and `indexsplit` take from it are alnStart, alnSpan and sliceLen of every reference's slices in file
// order; the device turns them into tile sizes (gd_crai_sizes).  zlib, member after member: a .crai may be several
// concatenated gzip members (the libdeflate path of the BAM reader takes one member at a time).
//
// As the reference: the line is trimmed of white space first; a seqID of -1 (unmapped) is skipped without a look at the
// other fields; a negative alnSpan ends the reading and keeps what was read; a last line without its newline is not seen.
// Refused here, with the line: a field count other than 6 or an unparsable number (the reference's
// errors), a seqID below -1 or above 2^20 - 1, |alnStart| or alnSpan above 2^31 - 1, a sliceLen outside int32, and a
// gzip stream that is damaged after its first header.
#pragma once

#include <zlib.h>

#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

namespace gdh {

struct CraiSlices {
    std::vector<int64_t> ref_off;                // [n_ref + 1] into the three arrays
    std::vector<int64_t> start, span;
    std::vector<int32_t> len;
};

namespace crai_detail {

// every member of a gzip file
inline bool gunzip(const std::string& path, std::string* text, std::string* why)
{
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) { *why = "cannot open the file"; return false; }
    std::vector<unsigned char> raw;
    unsigned char buf[1 << 16];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) raw.insert(raw.end(), buf, buf + n);
    const bool rd_ok = !ferror(f);
    fclose(f);
    if (!rd_ok) { *why = "cannot read the file"; return false; }
    if (raw.size() < 18 || raw[0] != 0x1f || raw[1] != 0x8b) { *why = "not a gzip file"; return false; }
    if (raw.size() > 0x7fffffffu) { *why = "the file is too large for a .crai"; return false; }
    z_stream zs{};
    if (inflateInit2(&zs, 15 + 16) != Z_OK) { *why = "zlib cannot start"; return false; }
    zs.next_in = raw.data();
    zs.avail_in = (uInt)raw.size();
    std::vector<unsigned char> out(1 << 18);
    bool ok = true;
    for (;;) {
        zs.next_out = out.data();
        zs.avail_out = (uInt)out.size();
        const int rc = inflate(&zs, Z_NO_FLUSH);
        text->append(reinterpret_cast<const char*>(out.data()), out.size() - zs.avail_out);
        if (rc == Z_STREAM_END) {
            if (zs.avail_in == 0) break;                     // the last member ended with the file
            if (inflateReset(&zs) != Z_OK) { ok = false; break; }
        } else if (rc != Z_OK || (zs.avail_in == 0 && zs.avail_out != 0)) {
            ok = false;                                      // damaged, or the file ends inside a member
            break;
        }
    }
    inflateEnd(&zs);
    if (!ok) *why = "the gzip stream is damaged or ends early";
    return ok;
}

// strconv.Atoi: an optional sign and decimal digits that fit an int64
inline bool atoi64(const char* p, const char* e, int64_t* v)
{
    bool neg = false;
    if (p < e && (*p == '+' || *p == '-')) neg = *p++ == '-';
    if (p == e) return false;
    uint64_t x = 0;
    const uint64_t lim = neg ? (uint64_t)1 << 63 : ((uint64_t)1 << 63) - 1;
    for (; p < e; ++p) {
        if (*p < '0' || *p > '9') return false;
        const uint64_t d = (uint64_t)(*p - '0');
        if (x > (lim - d) / 10) return false;
        x = x * 10 + d;
    }
    *v = neg ? (int64_t)(0 - x) : (int64_t)x;
    return true;
}

inline bool is_space(char c) { return c == ' ' || c == '\t' || c == '\n' || c == '\v' || c == '\f' || c == '\r'; }

}  // namespace crai_detail

// ReadIndex on the inflated text.  false: *line (1-based) and *why say where and what.
inline bool parse_crai_text(const std::string& text, CraiSlices* out, int64_t* line, std::string* why)
{
    using namespace crai_detail;
    struct Slice { int64_t start, span; int32_t len; };
    std::vector<std::vector<Slice>> refs;
    constexpr int64_t kMaxSeq = (1 << 20) - 1, kMaxPos = 0x7fffffffLL;
    static const char* const kField[6] = {"seqID", "alignment start", "alignment span", "container start", "slice start", "slice length"};
    size_t at = 0;
    *line = 0;
    for (;;) {
        const size_t nl = text.find('\n', at);
        if (nl == std::string::npos) break;      // a last line without its newline is not seen (:135)
        const char *p = text.data() + at, *e = text.data() + nl;
        at = nl + 1;
        ++*line;
        while (p < e && is_space(*p)) ++p;
        while (e > p && is_space(e[-1])) --e;
        const char* fb[6];
        const char* fe[6];
        int nf = 0;
        const char* q = p;
        for (const char* c = p;; ++c)
            if (c == e || *c == '\t') {
                if (nf < 6) { fb[nf] = q; fe[nf] = c; }
                ++nf;
                q = c + 1;
                if (c == e) break;
            }
        if (nf != 6) { *why = "expected 6 fields in index, got " + std::to_string(nf); return false; }
        int64_t v[6] = {0, 0, 0, 0, 0, 0};
        bool stop = false;
        for (int k = 0; k < 6; ++k) {
            if (!atoi64(fb[k], fe[k], &v[k])) {
                *why = std::string("unable to parse ") + kField[k] + " (" + std::string(fb[k], fe[k]) + ")";
                return false;
            }
            if (k == 0) {
                if (v[0] == -1) break;           // unmapped (:145-148): the other fields are not looked at
                if (v[0] < -1 || v[0] > kMaxSeq) { *why = "seqID " + std::to_string(v[0]) + " is outside 0 .. 2^20 - 1"; return false; }
                if (refs.size() <= (size_t)v[0]) refs.resize((size_t)v[0] + 1);
            } else if (k == 1) {
                if (v[1] < -kMaxPos || v[1] > kMaxPos) { *why = "alignment start " + std::to_string(v[1]) + " is outside +-(2^31 - 1)"; return false; }
            } else if (k == 2) {
                if (v[2] < 0) { stop = true; break; }        // (:163-166) what was read so far is kept
                if (v[2] > kMaxPos) { *why = "alignment span " + std::to_string(v[2]) + " is above 2^31 - 1"; return false; }
            } else if (k == 5) {
                if (v[5] < INT32_MIN || v[5] > INT32_MAX) { *why = "slice length " + std::to_string(v[5]) + " is outside int32"; return false; }
            }
        }
        if (stop) break;
        if (v[0] == -1) continue;
        refs[(size_t)v[0]].push_back(Slice{v[1], v[2], (int32_t)v[5]});
    }
    out->ref_off.assign(1, 0);
    for (const auto& r : refs) {
        for (const Slice& s : r) { out->start.push_back(s.start); out->span.push_back(s.span); out->len.push_back(s.len); }
        out->ref_off.push_back((int64_t)out->start.size());
    }
    return true;
}

// *line: 0 when the file cannot be opened or is not gzip
inline bool read_crai(const std::string& path, CraiSlices* out, int64_t* line, std::string* why)
{
    std::string text;
    *line = 0;
    if (!crai_detail::gunzip(path, &text, why)) return false;
    return parse_crai_text(text, out, line, why);
}

}  // namespace gdh
