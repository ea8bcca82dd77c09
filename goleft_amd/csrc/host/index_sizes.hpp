// index_sizes.hpp -- what `indexcov` and `indexsplit` both take from an index and a reference list: the tile sizes of a
// .bai linear index (indexcov's readIndex :471-525 + getSizes, types.go:45-82) and the references of a .fai in the
// order ReadFai (:278-318) gives them.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "bam_reader.hpp"

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
    uint64_t mapped = 0, unmapped = 0;           // of the pseudo-bins
};

inline bool read_index_sizes(const std::string& b, IndexSizes* s, std::string* why)
{
    std::vector<std::vector<uint64_t>> lin;
    std::vector<int64_t> nm, nu;
    std::string err;
    if (!BamReader::linear_index(b, &lin, &err, nullptr, nullptr, &nm, &s->raw, &nu)) {
        *why = "no usable index for " + b + (err.empty() ? "" : ": " + err);
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

}  // namespace gdh
