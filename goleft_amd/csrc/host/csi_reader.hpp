// csi_reader.hpp -- a .csi index (CSI version 1) as the device BAM read needs it: per reference the
// ANCHORS -- virtual offsets at which a record of the reference begins --, whether its bins hold chunks, the largest chunk
// end and the pseudo-bin's counts.  A .csi stores no linear index: the anchors are the sorted, distinct, non-zero values
// among the real bins' loffsets and chunk begins that are at or above the reference's smallest chunk begin.
//
// The file is BGZF (gzip members, read as any multi-member gzip); a payload that begins with "CSI\1" uncompressed is
// taken as it is.  Every count and offset is checked against the bytes that remain; bins come in any order; `aux` is
// skipped; n_no_coor may be absent.  Header only, zlib alone: tests/emul/csi_asan_main.cpp builds it with sanitizers.
#pragma once

#include <zlib.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

namespace gdh {

struct CsiIndex {
    int32_t min_shift = 0, depth = 0;
    std::vector<std::vector<uint64_t>> anchors;       // [n_ref]
    std::vector<char> has_chunks;                     // [n_ref] a real bin holds a chunk
    std::vector<uint64_t> chunk_end;                  // [n_ref] the largest chunk end of the real bins
    std::vector<int64_t> n_mapped, n_unmapped;        // [n_ref] of the pseudo-bin (none: -1 and 0)
    bool has_no_coor = false;
    uint64_t n_no_coor = 0;
};

// The pseudo-bin of a scheme with `depth` levels below bin 0: one behind the last real bin's successor.
inline uint64_t csi_pseudo_bin(int32_t depth) { return ((1ull << (3 * (depth + 1))) - 1) / 7 + 1; }

// The members of a gzip file, inflated one behind the other (at most `limit` bytes).
inline bool csi_inflate(const uint8_t* d, size_t n, std::vector<uint8_t>* out, std::string* err, size_t limit = (size_t)1 << 31)
{
    out->clear();
    if (n > 0xffffffffull) { if (err) *err = "the index is larger than is believable"; return false; }
    z_stream z;
    memset(&z, 0, sizeof z);
    if (inflateInit2(&z, 15 + 16) != Z_OK) { if (err) *err = "zlib cannot start"; return false; }
    std::vector<uint8_t> buf(1 << 16);
    z.next_in = const_cast<Bytef*>(d);
    z.avail_in = (uInt)n;
    const char* why = n ? nullptr : "truncated gzip data";
    while (!why) {
        z.next_out = buf.data();
        z.avail_out = (uInt)buf.size();
        const int rc = inflate(&z, Z_NO_FLUSH);
        const size_t got = buf.size() - z.avail_out;
        if (out->size() + got > limit) { why = "the index inflates to more than is believable"; break; }
        out->insert(out->end(), buf.data(), buf.data() + got);
        if (rc == Z_STREAM_END) {
            if (z.avail_in == 0) break;                                   // the last member ended with the file
            if (inflateReset(&z) != Z_OK) why = "zlib cannot restart";
        } else if (rc == Z_BUF_ERROR || (rc == Z_OK && z.avail_in == 0 && z.avail_out != 0)) why = "truncated gzip data";
        else if (rc != Z_OK) why = "damaged gzip data";
    }
    inflateEnd(&z);
    if (why && err) *err = why;
    return !why;
}

// The payload of a .csi -> *out.  false with *err: not a CSI, or a count or offset that the bytes do not hold.
inline bool parse_csi(const uint8_t* d, size_t n, CsiIndex* out, std::string* err)
{
    auto bad = [&](const char* what) { if (err) *err = what; return false; };
    auto r32 = [&](size_t p) { uint32_t v; memcpy(&v, d + p, 4); return v; };          // (little-endian hosts, as everywhere here)
    auto r64 = [&](size_t p) { uint64_t v; memcpy(&v, d + p, 8); return v; };
    if (n < 4 || memcmp(d, "CSI\1", 4) != 0) return bad("not a CSI");
    if (n < 16) return bad("truncated CSI");
    const int32_t min_shift = (int32_t)r32(4), depth = (int32_t)r32(8), l_aux = (int32_t)r32(12);
    if (min_shift < 0 || min_shift > 40 || depth < 0 || depth > 12) return bad("corrupt CSI: min_shift or depth");
    size_t p = 16;
    if (l_aux < 0 || (size_t)l_aux > n - p) return bad("truncated CSI");
    p += (size_t)l_aux;
    if (n - p < 4) return bad("truncated CSI");
    const int32_t n_ref = (int32_t)r32(p);
    p += 4;
    if (n_ref < 0 || (size_t)n_ref > (n - p) / 4) return bad("corrupt CSI: n_ref");     // every reference takes at least n_bin
    const uint64_t pseudo = csi_pseudo_bin(depth);
    CsiIndex x;
    x.min_shift = min_shift;
    x.depth = depth;
    x.anchors.assign((size_t)n_ref, std::vector<uint64_t>());
    x.has_chunks.assign((size_t)n_ref, 0);
    x.chunk_end.assign((size_t)n_ref, 0);
    x.n_mapped.assign((size_t)n_ref, -1);
    x.n_unmapped.assign((size_t)n_ref, 0);
    for (int32_t r = 0; r < n_ref; ++r) {
        if (n - p < 4) return bad("truncated CSI");
        const int32_t n_bin = (int32_t)r32(p);
        p += 4;
        if (n_bin < 0 || (size_t)n_bin > (n - p) / 16) return bad("corrupt CSI: n_bin");   // a bin takes at least 16 bytes
        std::vector<uint64_t>& v = x.anchors[(size_t)r];
        uint64_t first = ~0ull;
        for (int32_t b = 0; b < n_bin; ++b) {
            if (n - p < 16) return bad("truncated CSI");
            const uint32_t bin = r32(p);
            const uint64_t loffset = r64(p + 4);
            const int32_t n_chunk = (int32_t)r32(p + 12);
            p += 16;
            if (n_chunk < 0 || (size_t)n_chunk > (n - p) / 16) return bad("corrupt CSI: n_chunk");
            if (bin == pseudo) {
                if (n_chunk == 2) {                                 // {begin, end}, {n_mapped, n_unmapped}
                    x.n_mapped[(size_t)r] = (int64_t)r64(p + 16);
                    x.n_unmapped[(size_t)r] = (int64_t)r64(p + 24);
                }
            } else {
                if (loffset) v.push_back(loffset);
                for (int32_t k = 0; k < n_chunk; ++k) {
                    const uint64_t cb = r64(p + 16 * (size_t)k), ce = r64(p + 16 * (size_t)k + 8);
                    x.has_chunks[(size_t)r] = 1;
                    if (cb) v.push_back(cb);
                    first = std::min(first, cb);
                    x.chunk_end[(size_t)r] = std::max(x.chunk_end[(size_t)r], ce);
                }
            }
            p += 16 * (size_t)n_chunk;
        }
        std::sort(v.begin(), v.end());
        v.erase(std::unique(v.begin(), v.end()), v.end());
        v.erase(v.begin(), std::lower_bound(v.begin(), v.end(), first));     // (no chunk at all: nothing is left)
    }
    const size_t left = n - p;
    if (left >= 8) { x.has_no_coor = true; x.n_no_coor = r64(p); }
    else if (left != 0) return bad("truncated CSI");
    *out = std::move(x);
    return true;
}

// A .csi's bytes as they are in the file (BGZF), or its payload.
inline bool read_csi_bytes(const uint8_t* d, size_t n, CsiIndex* out, std::string* err)
{
    if (n >= 4 && memcmp(d, "CSI\1", 4) == 0) return parse_csi(d, n, out, err);
    if (n < 2 || d[0] != 0x1f || d[1] != 0x8b) { if (err) *err = "not a CSI"; return false; }
    std::vector<uint8_t> payload;
    if (!csi_inflate(d, n, &payload, err)) return false;
    return parse_csi(payload.data(), payload.size(), out, err);
}

}  // namespace gdh
