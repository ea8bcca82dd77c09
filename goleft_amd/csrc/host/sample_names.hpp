// sample_names.hpp -- samplename.Names (samplename/samplename.go:14-37) on the text of a BAM header, shared by
// `covstats` (the last column of a row) and `samplename`.
#pragma once

#include <algorithm>
#include <string>
#include <vector>

namespace gdh {

// One @RG -> its SM (nothing when it has none); several -> the distinct non-empty SMs (first appearance here; the
// reference's order is Go's map order).
inline std::vector<std::string> sample_name_list(const std::string& text)
{
    std::vector<std::string> sms;
    size_t n_rg = 0, p = 0;
    while (p < text.size()) {
        size_t e = text.find('\n', p);
        if (e == std::string::npos) e = text.size();
        const std::string line = text.substr(p, e - p);
        p = e + 1;
        if (line.compare(0, 4, "@RG\t") != 0) continue;
        ++n_rg;
        std::string sm;
        size_t q = 4;
        while (q <= line.size()) {
            size_t t = line.find('\t', q);
            if (t == std::string::npos) t = line.size();
            if (t - q >= 3 && line.compare(q, 3, "SM:") == 0) { sm = line.substr(q + 3, t - q - 3); break; }
            q = t + 1;
        }
        sms.push_back(sm);
    }
    std::vector<std::string> out;
    if (n_rg == 1) {
        if (!sms[0].empty()) out.push_back(sms[0]);
    } else {
        for (const std::string& s : sms)
            if (!s.empty() && std::find(out.begin(), out.end(), s) == out.end()) out.push_back(s);
    }
    return out;
}

}  // namespace gdh
