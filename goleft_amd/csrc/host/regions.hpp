// regions.hpp -- what the commands over the per-base vector (perbase, dist) share besides cli.hpp: an integer, a list of
// cut points, and the lines of a BED file as regions.  read_bed's messages name the caller's program.  parse_cuts gives the
// cause alone and the caller puts its flag in front (`--quantize 1,,4: an empty field`); the cause says "cut" for
// --thresholds' depths too: perbase's messages are pinned byte for byte, and one wording serves both.
// Header-only.
#pragma once
#include <algorithm>
#include <cerrno>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>

#include "../../../include/goleft_depth.h"
#include "../../../include/goleft_depth_host.h"
#include "cli.hpp"

namespace gdh {
namespace regions {

inline bool parse_int(const std::string& s, int* out)
{
    char* end = nullptr;
    errno = 0;
    const long v = strtol(s.c_str(), &end, 10);
    if (s.empty() || errno || *end || v < INT32_MIN || v > INT32_MAX) return false;
    *out = (int)v;
    return true;
}

// A list of cut points C1,C2,...: at most GD_PERBASE_MAX_CUTS integers, increasing, from 1; *why names the cause
inline bool parse_cuts(const std::string& s, std::vector<int32_t>* cuts, std::string* why)
{
    cuts->clear();
    for (size_t b = 0;;) {
        const size_t e = s.find(',', b);
        const std::string tok = s.substr(b, e == std::string::npos ? e : e - b);
        if (tok.empty()) { *why = "an empty field"; return false; }
        int v = 0;
        bool digits = true;
        for (size_t i = tok[0] == '-' || tok[0] == '+' ? 1 : 0; i < tok.size(); ++i) digits = digits && tok[i] >= '0' && tok[i] <= '9';
        if (!digits || !parse_int(tok, &v)) { *why = "'" + tok + "' is not an integer"; return false; }
        if (v < 1) { *why = "cut " + tok + " is below 1"; return false; }
        if (!cuts->empty() && v <= cuts->back()) { *why = "cut " + tok + " is not above the cut before it"; return false; }
        cuts->push_back(v);
        if (cuts->size() > (size_t)GD_PERBASE_MAX_CUTS) { *why = "more than " + std::to_string(GD_PERBASE_MAX_CUTS) + " cuts"; return false; }
        if (e == std::string::npos) break;
        b = e + 1;
    }
    return true;
}

struct Region { int32_t tid; int64_t start, end; };

// Every line of a BED file in file order, parsed as depth parses a region and clipped to its chromosome; blank lines and
// lines that start with '#' are skipped.  names, when asked for: the line's fourth tab-separated field, or "unknown".
inline int read_bed(const char* prog, const std::string& path, const std::map<std::string, int>& tid_of, const std::vector<int64_t>& lens,
                    std::vector<Region>* out, std::vector<std::string>* names = nullptr)
{
    gdh::cli::Lines in;
    if (!in.open(path)) { fprintf(stderr, "%s: cannot open %s\n", prog, path.c_str()); return 1; }
    std::string line;
    std::vector<char> chrom(1 << 16);
    while (in.next(&line)) {
        if (line.empty() || line[0] == '#') continue;
        const std::string nl = line + "\n";
        int64_t s = 0, e = 0;
        if (nl.size() >= chrom.size() || gdh_chrom_start_end(nl.c_str(), nl.size(), chrom.data(), chrom.size(), &s, &e) != 0) {
            fprintf(stderr, "%s: %s:%lld: cannot get a region from this line\n", prog, path.c_str(), in.lineno);
            return 1;
        }
        const auto it = tid_of.find(chrom.data());
        if (it == tid_of.end()) {
            fprintf(stderr, "%s: %s:%lld: chromosome %s is not in the BAM header\n", prog, path.c_str(), in.lineno, chrom.data());
            return 1;
        }
        const int64_t len = lens[(size_t)it->second];
        e = std::min(e, len);
        s = std::min(s, e);
        if (e < s) e = s;
        out->push_back(Region{it->second, s, e});
        if (names) {
            size_t b = 0;
            for (int f = 0; f < 3 && b != std::string::npos; ++f) { b = line.find('\t', b); if (b != std::string::npos) ++b; }
            const std::string name = b == std::string::npos ? std::string() : line.substr(b, line.find('\t', b) - b);
            names->push_back(name.empty() ? std::string("unknown") : name);
        }
    }
    return 0;
}

}  // namespace regions
}  // namespace gdh
