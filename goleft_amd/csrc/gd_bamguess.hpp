// gd_bamguess.hpp -- record starts of an inflated BAM stream WITHOUT an index, guessed.
//
// BAM records delimit themselves only forwards, and the device walk (gd_bamdecode.hpp) therefore enters the stream at
// record starts a .bai knows.  Making the .bai needs another way in: the inflated bytes of a range are cut into fixed
// slices (slice s is [first + s * slice, first + (s + 1) * slice), `first` being the range's known first record), one
// wave works per slice, and its lanes test 64 candidate offsets at a time, from the slice's first byte on, for the
// shape of a record (bam_candidate) and for a chain of `checks` further records behind it that keep that shape or run
// into the slice's end.  The lowest surviving offset is the slice's guess; a slice may have none (a read longer than
// the slice).  Slice 0 has no guess to make: it begins at `first`.
//
// A GUESS DECIDES SPEED, NEVER THE ANSWER: the walk that starts at a guess reports where it stopped, and the host
// (gd_api_index.inc) uses a segment's records only once the segment in front of it, itself confirmed, stopped exactly on
// its start.  bam_candidate compiles for the host (tests/emul/idxwalk_asan_main.cpp drives it behind guard pages): every
// byte it reads is checked against n_bytes first.
#pragma once
#include "gd_bamdecode.hpp"

namespace gd {

struct GuessJob {
    const uint8_t* data;            // inflated bytes of the range
    uint64_t n_bytes;
    uint64_t first;                 // the range's first record
    uint64_t slice;                 // bytes per slice (> 0)
    uint32_t n_slice;
    uint32_t checks;                // records the chain behind a candidate must hold
    int32_t  n_ref;
    const int32_t* ref_len;         // [n_ref]
    uint64_t* guess;                // [n_slice] the slice's guess; all ones: none
};

// Do the bytes at `off` look like a record?  *next: where the record behind it would begin.
__device__ __forceinline__ bool bam_candidate(const uint8_t* data, uint64_t n_bytes, uint64_t off, int32_t n_ref,
                                              const int32_t* ref_len, uint64_t* next)
{
    if (off > n_bytes || n_bytes - off < 36) return false;                // block_size and the 32 fixed bytes
    const uint8_t* const r = data + off;
    const uint32_t block_size = ld32(r);
    if (block_size < 32) return false;
    const int32_t ref = (int32_t)ld32(r + 4), pos = (int32_t)ld32(r + 8);
    const int32_t mref = (int32_t)ld32(r + 24), mpos = (int32_t)ld32(r + 28);
    if (ref < -1 || ref >= n_ref || mref < -1 || mref >= n_ref) return false;
    if (pos < -1 || (ref >= 0 && pos >= ref_len[ref])) return false;
    if (mpos < -1 || (mref >= 0 && mpos >= ref_len[mref])) return false;
    const uint32_t l_read_name = r[12];
    const uint32_t n_cigar = (uint32_t)r[16] | ((uint32_t)r[17] << 8);
    const uint64_t l_seq = ld32(r + 20);
    if (l_read_name < 1) return false;
    if (32ull + l_read_name + 4ull * n_cigar + (l_seq + 1) / 2 + l_seq > block_size) return false;
    const uint64_t nul = off + 36 + l_read_name - 1;                      // the name's last byte
    if (nul >= n_bytes || data[nul] != 0) return false;
    *next = off + 4ull + block_size;
    return true;
}

// The candidate at `off` and `checks` records behind it; a chain that reaches `end` (the slice's, or the range's) has passed.
__device__ __forceinline__ bool bam_candidate_chain(const uint8_t* data, uint64_t n_bytes, uint64_t off, uint64_t end, uint32_t checks,
                                                    int32_t n_ref, const int32_t* ref_len)
{
    uint64_t o = off;
    for (uint32_t k = 0; k <= checks; ++k) {
        if (k && (o >= end || n_bytes - o < 36)) return true;             // (o < end <= n_bytes here)
        uint64_t next = 0;
        if (!bam_candidate(data, n_bytes, o, n_ref, ref_len, &next)) return false;
        o = next;
    }
    return true;
}

__global__ __launch_bounds__(64) void gd_bam_guess_kernel(GuessJob j)
{
    const uint32_t s = blockIdx.x, lane = threadIdx.x;
    if (s >= j.n_slice) return;
    const uint64_t beg = j.first + (uint64_t)s * j.slice;
    const uint64_t end = beg + j.slice < j.n_bytes ? beg + j.slice : j.n_bytes;
    uint64_t found = ~0ull;
    if (s == 0) found = beg;
    else
        for (uint64_t base = beg; base < end; base += 64) {              // (the same trip count for every lane)
            const uint64_t o = base + lane;
            const bool ok = o < end && bam_candidate_chain(j.data, j.n_bytes, o, end, j.checks, j.n_ref, j.ref_len);
            const uint64_t m = __ballot(ok);
            if (m) { found = base + (uint64_t)__builtin_ctzll(m); break; }
        }
    if (lane == 0) j.guess[s] = found;
}

}  // namespace gd
