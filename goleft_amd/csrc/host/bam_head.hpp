// bam_head.hpp -- what the commands that feed a whole BAM to the device range by range (covstats, index) read on the host
// first: the header -- references, text, and how many bytes of the inflated stream lie in front of the first record -- and
// the virtual offset of that record.
#pragma once

#include <zlib.h>

#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "bam_reader.hpp"
#include "gpu_ingest.hpp"

namespace gdh {

struct BamHead {
    std::vector<std::string> names;
    std::vector<int64_t> lengths;
    std::string text;
    uint64_t length = 0;        // bytes of the inflated stream in front of the first record
};

inline bool read_bam_head(const std::string& path, BamHead* h, std::string* err)
{
    gzFile f = gzopen(path.c_str(), "rb");
    if (!f) { *err = "cannot open " + path; return false; }
    auto rd = [&](void* dst, size_t n) { return n == 0 || gzread(f, dst, (unsigned)n) == (int)n; };
    uint8_t b4[4];
    auto u32 = [&](uint32_t* v) { if (!rd(b4, 4)) return false; *v = (uint32_t)b4[0] | ((uint32_t)b4[1] << 8) | ((uint32_t)b4[2] << 16) | ((uint32_t)b4[3] << 24); return true; };
    char magic[4];
    uint32_t l_text = 0, n_ref = 0;
    bool ok = rd(magic, 4) && memcmp(magic, "BAM\1", 4) == 0 && u32(&l_text);
    if (ok) { h->text.resize(l_text); ok = rd(&h->text[0], l_text) && u32(&n_ref); }
    h->length = 12ull + l_text;
    for (uint32_t r = 0; ok && r < n_ref; ++r) {
        uint32_t l_name = 0, l_ref = 0;
        std::string name;
        ok = u32(&l_name) && l_name > 0 && l_name < (1u << 20);
        if (ok) { name.resize(l_name); ok = rd(&name[0], l_name) && u32(&l_ref); }
        if (ok) {
            name.resize(strnlen(name.c_str(), name.size()));
            h->names.push_back(name);
            h->lengths.push_back((int64_t)(int32_t)l_ref);
            h->length += 8ull + l_name;
        }
    }
    gzclose(f);
    if (!ok) *err = path + ": not a BAM file or a truncated header";
    const size_t nul = h->text.find('\0');
    if (nul != std::string::npos) h->text.resize(nul);
    return ok;
}

// The virtual offset of the first record: the member that holds byte `header_length` of the inflated stream.  *have: there is
// such a member (a file that ends with its header has none).  false: the file does not begin with BGZF members.
inline bool first_record_voffset(int fd, uint64_t file_size, uint64_t header_length, uint64_t* voff, bool* have)
{
    *have = false;
    MemberTable mt;
    uint64_t span = std::min<uint64_t>(file_size, 1u << 20);
    for (;;) {
        if (!list_members_serial_fd(fd, 0, (size_t)span, &mt)) return false;
        uint64_t cum = 0;
        for (size_t m = 0; m < mt.n && !*have; ++m) {
            if (header_length < cum + mt.isize[m]) { *voff = (mt.off[m] << 16) | (header_length - cum); *have = true; }
            cum += mt.isize[m];
        }
        if (*have || span >= file_size) return true;
        span = std::min<uint64_t>(file_size, span * 4);
    }
}

}  // namespace gdh
