// index_sizes.hpp -- what `indexcov` and `indexsplit` both take from an index and a reference list: the tile sizes of a
// .bai linear index (indexcov's readIndex :471-525 + getSizes, types.go:45-82) or of a .crai (the slices read by
// crai_reader.hpp on the reader threads, then tiled on the device for the whole cohort at once: tile_crai_indexes), and
// the references of a .fai in the order ReadFai (:278-318) gives them.
#pragma once

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../../include/goleft_depth.h"
#include "bam_reader.hpp"
#include "crai_reader.hpp"

namespace gdh {

inline bool ends_with(const std::string& s, const char* suf)
{
    const size_t n = strlen(suf);
    return s.size() >= n && s.compare(s.size() - n, n, suf) == 0;
}

struct FaiRef { std::string name; int64_t length; };

inline bool read_fai(const std::string& path, std::vector<FaiRef>* refs)
{
    FILE* f = fopen(path.c_str(), "r");
    if (!f) return false;
    std::vector<std::pair<int64_t, FaiRef>> recs;
    char* line = nullptr;
    size_t cap = 0;
    while (getline(&line, &cap, f) > 0) {
        std::vector<std::string> t;
        std::string cur;
        for (const char* p = line; *p && *p != '\n'; ++p) { if (*p == '\t') { t.push_back(cur); cur.clear(); } else cur.push_back(*p); }
        t.push_back(cur);
        if (t.size() < 3) continue;
        recs.push_back({strtoll(t[2].c_str(), nullptr, 10), FaiRef{t[0], strtoll(t[1].c_str(), nullptr, 10)}});
    }
    free(line);
    fclose(f);
    std::stable_sort(recs.begin(), recs.end(), [](const auto& x, const auto& y) { return x.first < y.first; });   // ReadFai :293
    for (auto& r : recs) refs->push_back(r.second);
    return !refs->empty();
}

// The tile sizes of one index: the differences of consecutive entries of every reference's interval array as stored.
// b: x.bam (index x.bam.bai, else x.bai) or a bare .bai.
struct IndexSizes {
    std::vector<std::vector<uint64_t>> raw;      // the interval arrays as stored
    std::vector<int64_t> ref_off;                // [n_ref + 1] into sizes
    std::vector<int64_t> sizes;
    uint64_t mapped = 0, unmapped = 0;           // of the pseudo-bins (a .crai has none: 0)
    bool is_crai = false;
    CraiSlices crai;                             // a .crai: its slices, until tile_crai_indexes has made sizes of them
    double crai_read_s = 0;                      // ... and the seconds its inflate + parse took
};

inline bool read_index_sizes(const std::string& b, IndexSizes* s, std::string* why)
{
    if (ends_with(b, ".cram")) {
        *why = b + ": CRAM alignment files are not read: pass the .crai index instead";
        return false;
    }
    if (ends_with(b, ".crai")) {
        const auto t0 = std::chrono::steady_clock::now();
        int64_t line = 0;
        std::string err;
        s->is_crai = true;
        if (!read_crai(b, &s->crai, &line, &err)) {
            *why = "error from index: " + b + ": " + (line > 0 ? "line " + std::to_string(line) + ": " : std::string()) + err;
            return false;
        }
        if (s->crai.start.empty()) { *why = "bad index: " + b + " has no slice on any reference"; return false; }
        s->crai_read_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        return true;
    }
    std::vector<std::vector<uint64_t>> lin;
    std::vector<int64_t> nm, nu;
    std::string err;
    if (!BamReader::linear_index(b, &lin, &err, nullptr, nullptr, &nm, &s->raw, &nu)) {
        if (err == kCsiHasNoTiles) *why = b + ": " + err;
        else *why = "no usable index for " + b + (err.empty() ? "" : ": " + err);
        return false;
    }
    for (size_t r = 0; r < nm.size(); ++r)
        if (nm[r] >= 0) { s->mapped += (uint64_t)nm[r]; s->unmapped += (uint64_t)nu[r]; }
    s->ref_off.assign(1, 0);
    for (const auto& iv : s->raw) {
        for (size_t k = 1; k < iv.size(); ++k) {
            const int64_t d = (int64_t)iv[k] - (int64_t)iv[k - 1];
            if (d < 0) { *why = "expected positive change in vOffset: the linear index of " + b + " decreases"; return false; }
            s->sizes.push_back(d);
        }
        s->ref_off.push_back((int64_t)s->sizes.size());
    }
    if (s->sizes.empty()) { *why = "indexcov: no usable chromsomes in bam: " + b; return false; }   // Index.init :100-102
    return true;
}

// The .crai indexes among smp (paths[i] names smp[i]) get their sizes / ref_off: every reference of every one of them is a
// sequence of ONE gd_crai_sizes call (crai.go:56-127 makeSizes on the device).  *seconds: the wall clock of that.
inline bool tile_crai_indexes(gd_ctx* ctx, const std::vector<IndexSizes*>& smp, const std::vector<std::string>& paths, std::string* why,
                              double* seconds)
{
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<int64_t> seq_off(1, 0), start, span;
    std::vector<int32_t> len;
    int64_t guess = 0;
    for (IndexSizes* s : smp) {
        if (!s->is_crai) continue;
        const CraiSlices& c = s->crai;
        const int64_t base = (int64_t)start.size();
        for (size_t r = 0; r + 1 < c.ref_off.size(); ++r) {
            seq_off.push_back(base + c.ref_off[r + 1]);
            int64_t end = 0;
            for (int64_t i = c.ref_off[r]; i < c.ref_off[r + 1]; ++i) end = std::max(end, c.start[(size_t)i] + c.span[(size_t)i]);
            guess += end / 16384 + 2;
        }
        start.insert(start.end(), c.start.begin(), c.start.end());
        span.insert(span.end(), c.span.begin(), c.span.end());
        len.insert(len.end(), c.len.begin(), c.len.end());
    }
    const size_t n_seq = seq_off.size() - 1;
    if (n_seq == 0) return true;
    if (n_seq > (size_t)INT32_MAX) { *why = "too many .crai references in one cohort"; return false; }
    std::vector<int64_t> tile_off(n_seq + 1), sizes((size_t)guess);
    std::vector<int32_t> status(n_seq);
    // sorted slices fit the guess; if not, the call has left the counts and runs once more
    for (int pass = 0;; ++pass) {
        const int rc = gd_crai_sizes(ctx, (int32_t)n_seq, seq_off.data(), start.data(), span.data(), len.data(), tile_off.data(),
                                     status.data(), sizes.data(), sizes.size());
        if (rc == GD_E_CAPACITY && pass == 0) { sizes.assign((size_t)tile_off[n_seq], 0); continue; }
        if (rc != GD_OK) { *why = std::string("gd_crai_sizes: ") + gd_strerror(rc) + " (" + gd_last_error(ctx) + ")"; return false; }
        break;
    }
    size_t q = 0;
    for (size_t i = 0; i < smp.size(); ++i) {
        IndexSizes* s = smp[i];
        if (!s->is_crai) continue;
        const size_t nr = s->crai.ref_off.size() - 1;
        const int64_t a = tile_off[q];
        s->ref_off.assign(1, 0);
        for (size_t r = 0; r < nr; ++r, ++q) {
            if (status[q] != 0) {
                *why = "error from index: " + paths[i] + ": reference " + std::to_string(r) + ": the slices do not tile (" +
                       (status[q] == 1 ? "tilewidth logic error" : "logic error") + ")";
                return false;
            }
            s->ref_off.push_back(tile_off[q + 1] - a);
        }
        s->sizes.assign(sizes.begin() + a, sizes.begin() + tile_off[q]);
        for (int64_t v : s->sizes)
            if (v < 0) { *why = "error from index: " + paths[i] + ": a negative slice length"; return false; }
        if (s->sizes.empty()) { *why = "indexcov: no usable chromsomes in bam: " + paths[i]; return false; }   // Index.init :100-102
        s->crai = CraiSlices();
    }
    *seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return true;
}

}  // namespace gdh
