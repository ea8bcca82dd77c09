// gd_crai.hpp -- the slices of a .crai turned into sizes per 16 384-base tile (makeSizes, indexcov/crai/crai.go:56-127 of
// the reference).  A sequence is one reference of one index; its slices carry a state from one to
// the next (the tiles emitted so far, the value that waits for the next gap), so they are walked in order -- by one
// wavefront per sequence, with the state in scalar registers.  What is parallel is everything else: the sequences of a
// cohort, and the fills of a slice (the zeros of a gap, the n copies of a long slice's value), which all 64 lanes store.
//
//   crai_walk<P>             THE walk; the policy P says what a fill does
//   gd_crai_kernel<false>    CraiCount: nothing is stored; the walk ends with the tile count and the status of a sequence
//   gd_crai_kernel<true>     CraiWrite: the same walk after the scan of the counts, storing into the sequence's tiles
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gd {

constexpr int CRAI_WAVES = 4;                    // sequences of a workgroup
constexpr int64_t CRAI_TILE = 16384;             // crai.TileWidth
enum { CRAI_OK = 0, CRAI_PANIC_TILEWIDTH = 1, CRAI_PANIC_LOGIC = 2 };   // the reference's two panics (:89, :120)

struct CraiJob {
    int32_t n_seq;
    const int64_t* seq_off;                      // [n_seq + 1] into the three slice arrays
    const int64_t* aln_start;
    const int64_t* aln_span;
    const int32_t* slice_len;
    int64_t* tile_off;                           // [n_seq + 1]: count pass: the count of sequence s at [s + 1]; write pass: the scan
    int32_t* status;                             // [n_seq], count pass
    int64_t* sizes;                              // write pass
};

// lane k's value in a scalar register (k is the same in every lane)
__device__ __forceinline__ int64_t crai_lane(int64_t v, int k)
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, k);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)((uint64_t)v >> 32), k);
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

// int64(100000 * float64(sliceLen) / float64(alnSpan)) (:106): the product and the quotient each with their own rounding
__device__ __forceinline__ int64_t crai_per_base(int32_t slice_len, int64_t span)
{
#pragma clang fp contract(off)
    const double p = 100000.0 * (double)slice_len;
    const double q = p / (double)span;
    return (int64_t)q;
}

struct CraiCount {
    __device__ __forceinline__ void fill(int64_t, int64_t, int64_t, int64_t, int) const {}
};

// n tiles from tile `at` of the sequence: the first holds `first`, the others `val`; consecutive lanes, consecutive words
struct CraiWrite {
    int64_t* __restrict__ out;                   // the sequence's tiles
    int64_t room;                                // ... and how many the scan gave it
    __device__ __forceinline__ void fill(int64_t at, int64_t n, int64_t first, int64_t val, int lane) const
    {
        if (at + n > room) n = room - at;        // (the count pass ran the same walk: never taken)
        for (int64_t i = lane; i < n; i += 64) out[at + i] = i == 0 ? first : val;
    }
};

// One wavefront, one sequence.  Every value below but `lane` and the three loaded words is the same in all lanes.
template <class P>
__device__ __forceinline__ void crai_walk(const CraiJob& j, int s, int lane, const P& p, int64_t* n_out, int* status_out)
{
    const int64_t a = j.seq_off[s], b = j.seq_off[s + 1];
    int64_t n = 0, last_val = 0;                 // lastStart is TILE * n throughout
    int status = CRAI_OK;
    for (int64_t base = a; base < b && status == CRAI_OK; base += 64) {
        const int nb = (int)(b - base < 64 ? b - base : 64);
        int64_t v_start = 0, v_span = 0;
        int32_t v_len = 0;
        if (lane < nb) { v_start = j.aln_start[base + lane]; v_span = j.aln_span[base + lane]; v_len = j.slice_len[base + lane]; }
        for (int k = 0; k < nb; ++k) {
            int64_t start = crai_lane(v_start, k), span = crai_lane(v_span, k);
            const int32_t len = __builtin_amdgcn_readlane(v_len, k);
            // back fill gaps (:78-86): the first tile of the run takes the pending value
            const int64_t gap = start - CRAI_TILE - CRAI_TILE * n;
            if (gap > 0) {
                const int64_t g = (gap + CRAI_TILE - 1) >> 14;
                p.fill(n, g, last_val, 0, lane);
                n += g;
                last_val = 0;
            }
            int64_t over = start - CRAI_TILE * n;
            if (over > CRAI_TILE) { status = CRAI_PANIC_TILEWIDTH; break; }
            if (over < -CRAI_TILE) {             // a long read of the slice before reaches into this one (:91-99)
                const int64_t sh = ((-CRAI_TILE - over) + CRAI_TILE - 1) >> 14;
                start += sh * CRAI_TILE;
                span -= sh * CRAI_TILE;
                over = start - CRAI_TILE * n;
            }
            if (span <= 0) continue;
            const int64_t per_base = crai_per_base(len, span);
            const int64_t n_tiles = span >> 14;
            if (n_tiles == 0 && over < CRAI_TILE) { last_val = per_base; continue; }
            p.fill(n, n_tiles, per_base, per_base, lane);
            n += n_tiles;
            const int64_t cmp = (start + span) / CRAI_TILE;      // (truncates, as Go's)
            if (n > cmp + 1 || cmp < n - 1) { status = CRAI_PANIC_LOGIC; break; }
            last_val = per_base;
        }
    }
    *n_out = n;
    *status_out = status;
}

template <bool WRITE>
__global__ __launch_bounds__(CRAI_WAVES * 64) void gd_crai_kernel(CraiJob j)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    for (int64_t s = (int64_t)blockIdx.x * CRAI_WAVES + wave; s < j.n_seq; s += (int64_t)gridDim.x * CRAI_WAVES) {
        int64_t n;
        int status;
        if constexpr (WRITE) {
            const int64_t o = j.tile_off[s];
            crai_walk(j, (int)s, lane, CraiWrite{j.sizes + o, j.tile_off[s + 1] - o}, &n, &status);
        } else {
            crai_walk(j, (int)s, lane, CraiCount{}, &n, &status);
            if (lane == 0) { j.tile_off[s + 1] = n; j.status[s] = status; }
        }
    }
}

}  // namespace gd
