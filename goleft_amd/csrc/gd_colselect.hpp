// gd_colselect.hpp -- one exact order statistic per COLUMN of a row-major [rows][samples] matrix (DESIGN.md section
// 3.12): dcnv's SampleMedians (dcnv/dcnv.go:108-125 of the reference), sorted[k + int(0.65 * float64(n))] with k the
// zeros of the column and n the rest.  A column spans the whole matrix, so the selection streams it: a most-significant-
// digit-first radix select, 8 bits a pass.
//
//   gd_colselect_hist_kernel<T, FIRST>   one pass over the matrix: the digit histogram of every column, counting the
//                                        cells that still agree with the column's prefix.  Lanes run along samples
//                                        (lane l of a workgroup of the y-th column tile owns column 64 y + l, so a
//                                        wave's load of a row is 64 consecutive cells), the CS_WAVES waves of a workgroup
//                                        take rows, CS_ROWS each a turn: a slab of CS_SLAB rows, and a grid-stride loop
//                                        over the slabs.  The histogram is in LDS as [bin][column]: lane l only ever
//                                        touches words that are l mod 64, so the 32 lanes of a half-wave hit 32 distinct
//                                        banks whatever their digits are (LDS atomics bank as ds_write_b32 does: word
//                                        mod 32, per half-wave).  At the end the non-zero counters go to the global
//                                        [samples][256] table with one atomic each.
//   gd_colselect_pick_kernel<MODE>       one wavefront a column: the bin the rank falls in, the rank left inside it,
//                                        the prefix one digit longer; the counters are left zero for the next pass.
//   gd_colmid_pick_kernel                the float first pick with another rank: rows / 2 over all cells, zeros included.
//
// T = float: the keys are the bit patterns (non-negative floats order as their bits do; -0.0 is mapped to 0), four passes;
// the first also counts the exact zeros, in a register.  T = int64_t: the first pass is a histogram of the cell's LENGTH
// in bytes (0 for a zero, 9 for a negative cell, which the caller refuses), which gives the zeros, the rank and the
// length L of the answer; L digit passes follow, over the cells of at most L bytes -- the leading passes in which every
// digit is 0 are never run.  The host launches max L over the columns; a column that is done matches nothing.  Nothing
// passes through a float.
//
// LDS: 256 bins x 64 columns x 4 bytes = 64 KB a workgroup; designed for TWO workgroups of 512 threads per CU (128 KB of the
// 160 KB; sixteen waves, four per SIMD), hence CS_MAX_GRID = 512 workgroups.  No scratch: the CS_ROWS cells in flight are
// an unrolled array, nothing is indexed by a runtime value.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gd {

constexpr int CS_WAVES = 8;                      // waves of a histogram workgroup
constexpr int CS_WG = CS_WAVES * 64;
constexpr int CS_ROWS = 8;                       // rows a wave has in flight (16 measured no faster)
constexpr int CS_SLAB = CS_WAVES * CS_ROWS;      // rows of a workgroup's turn
constexpr int CS_COLS = 64;                      // columns of a workgroup: one per lane
constexpr int CS_BINS = 256;
constexpr int CS_WG_PER_CU = 2;
constexpr int CS_MAX_GRID = CS_WG_PER_CU * 256;  // workgroups of a launch, all column tiles together
constexpr int CS_MAX_N = 4096;
constexpr int CS_PICK_WAVES = 4;                 // columns of a pick workgroup
constexpr double CS_QUANTILE = 0.65;             // dcnv.go:121

enum { CS_PICK_FLOAT_FIRST = 0, CS_PICK_LENGTH = 1, CS_PICK_DIGIT = 2, CS_PICK_FLOAT_MID = 3 };

struct CsJob {
    const void* cells;                           // [n_rows][n] float or int64_t
    int64_t n_rows;
    int32_t n;
    uint32_t* counts;                            // [n][256], zero between the passes
    uint32_t* zeros;                             // [n] (float: the exact zeros of a column)
    uint64_t* prefix;                            // [n] the digits decided so far; the answer when rem is 0
    int32_t* rem;                                // [n] digits still to decide
    uint32_t* rank;                              // [n] rank among the cells that agree with the prefix
    uint64_t* nonzero;                           // [n] out: n of the column
    uint32_t* flags;                             // [0]: max rem after the length pass; [1]: a negative cell was seen
};

__device__ __forceinline__ uint64_t cs_key(float f)
{
    return f == 0.0f ? 0u : (uint64_t)__float_as_uint(f);        // (-0 is 0)
}
__device__ __forceinline__ uint64_t cs_key(int64_t v) { return (uint64_t)v; }

// bytes of a key: 0 for 0, 8 for 2^56 and above; 9 marks a negative cell
__device__ __forceinline__ uint32_t cs_length(uint64_t k)
{
    if (k >> 63) return 9;
    return k ? (uint32_t)(64 - __builtin_clzll(k) + 7) >> 3 : 0u;
}

template <class T, bool FIRST>
__global__ __launch_bounds__(CS_WG) void gd_colselect_hist_kernel(CsJob j)
{
    __shared__ uint32_t hist[CS_BINS * CS_COLS];
    const int lane = threadIdx.x & 63;
    const int wave = (int)(threadIdx.x >> 6);
    const int col = (int)blockIdx.y * CS_COLS + lane;
    const int n = j.n;
    for (int i = threadIdx.x; i < CS_BINS * CS_COLS; i += CS_WG) hist[i] = 0;
    __syncthreads();

    bool live = col < n;
    uint64_t prefix = 0;
    int shift = 0;                               // bits below the digit of this pass
    bool all = FIRST;                            // every cell agrees (no digit decided, 8 to go)
    if (!FIRST && live) {
        const int rem = j.rem[col];
        live = rem > 0;
        prefix = j.prefix[col];
        shift = 8 * (rem - 1);
        all = rem >= 8;
    }
    uint32_t zeros = 0;
    const auto count = [&](T cell) {
        const uint64_t k = cs_key(cell);
        uint32_t bin;
        if constexpr (FIRST && sizeof(T) == 8) {
            bin = cs_length(k);
        } else if constexpr (FIRST) {
            bin = (uint32_t)(k >> 24);
            zeros += k == 0 ? 1u : 0u;
        } else {
            if (!all && ((k >> shift) >> 8) != prefix) return;
            bin = (uint32_t)(k >> shift) & 255u;
        }
        atomicAdd(&hist[bin * CS_COLS + lane], 1u);
    };
    if (live) {
        // a slab starts at a wave-uniform pointer; what a lane adds to it does not change from slab to slab
        uint32_t off[CS_ROWS];
#pragma unroll
        for (int u = 0; u < CS_ROWS; ++u) off[u] = (uint32_t)(u * CS_WAVES + wave) * (uint32_t)n + (uint32_t)col;
        for (int64_t base = (int64_t)blockIdx.x * CS_SLAB; base < j.n_rows; base += (int64_t)gridDim.x * CS_SLAB) {
            const T* slab = static_cast<const T*>(j.cells) + (size_t)base * (size_t)n;
            if (base + CS_SLAB <= j.n_rows) {    // a whole slab: CS_ROWS loads in flight, no row is tested
                T v[CS_ROWS];
#pragma unroll
                for (int u = 0; u < CS_ROWS; ++u) v[u] = slab[off[u]];
#pragma unroll
                for (int u = 0; u < CS_ROWS; ++u) count(v[u]);
            } else {                             // the matrix's last rows
#pragma unroll
                for (int u = 0; u < CS_ROWS; ++u)
                    if (base + u * CS_WAVES + wave < j.n_rows) count(slab[off[u]]);
            }
        }
    }
    __syncthreads();
    // the workgroups of a tile add to the same counters at about the same time: each starts at another bin
    const int col0 = (int)blockIdx.y * CS_COLS, turn = (int)(blockIdx.x * 8u) * CS_COLS;
    for (int t = threadIdx.x; t < CS_BINS * CS_COLS; t += CS_WG) {
        const int i = (t + turn) & (CS_BINS * CS_COLS - 1);
        const uint32_t c = hist[i];              // (consecutive lanes, consecutive columns: no bank twice)
        const int cl = col0 + (i & (CS_COLS - 1));
        if (c && cl < n) atomicAdd(&j.counts[(size_t)cl * CS_BINS + (size_t)(i >> 6)], c);
    }
    if (FIRST && sizeof(T) == 4 && zeros) atomicAdd(&j.zeros[col], zeros);
}

// the rank dcnv.go:118-122 reads: k leading zeros, then int(0.65 * float64(n)) into the n others
__device__ __forceinline__ uint32_t cs_rank(uint64_t k, uint64_t n)
{
#pragma clang fp contract(off)
    return (uint32_t)(k + (uint64_t)(int64_t)(CS_QUANTILE * (double)n));
}

template <int MODE>
__device__ __forceinline__ void cs_pick(const CsJob& j)
{
    const int lane = threadIdx.x & 63;
    const int col = (int)blockIdx.x * CS_PICK_WAVES + (int)(threadIdx.x >> 6);
    if (col >= j.n) return;                      // (wave-uniform)
    int rem = 0;
    uint64_t prefix = 0;
    uint32_t rank = 0;
    if constexpr (MODE == CS_PICK_DIGIT) {
        rem = j.rem[col];
        if (rem == 0) return;                    // done: nothing was counted
        prefix = j.prefix[col];
        rank = j.rank[col];
    }
    // lane l holds bins 4 l .. 4 l + 3
    uint4* mine = reinterpret_cast<uint4*>(j.counts + (size_t)col * CS_BINS) + lane;
    const uint4 c = *mine;
    *mine = make_uint4(0, 0, 0, 0);
    const uint32_t own = c.x + c.y + c.z + c.w;
    uint32_t incl = own;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = __shfl_up(incl, o, 64);
        if (lane >= o) incl += up;
    }
    if constexpr (MODE != CS_PICK_DIGIT) {
        const uint64_t rows = (uint64_t)j.n_rows;
        uint64_t k;
        if constexpr (MODE == CS_PICK_FLOAT_FIRST || MODE == CS_PICK_FLOAT_MID) {
            k = j.zeros[col];
        } else {
            k = __shfl(c.x, 0, 64);                                // length 0
            const uint32_t negative = __shfl(c.y, 2, 64);           // length 9
            if (negative && lane == 0) j.flags[1] = 1;
        }
        const uint64_t nz = rows - k;
        if (lane == 0) j.nonzero[col] = nz;
        if (nz == 0) {                           // an all-zero column: the reference indexes an empty slice; here 0
            if (lane == 0) { j.prefix[col] = 0; j.rem[col] = 0; j.rank[col] = 0; }
            return;
        }
        rank = MODE == CS_PICK_FLOAT_MID ? (uint32_t)(rows / 2) : cs_rank(k, nz);
        rem = 4;
    }
    const uint32_t excl = incl - own;
    if (!(rank >= excl && rank < incl)) return;  // one lane goes on
    uint32_t bin = 4u * (uint32_t)lane, left = rank - excl;
    if (left >= c.x) {
        left -= c.x; ++bin;
        if (left >= c.y) {
            left -= c.y; ++bin;
            if (left >= c.z) { left -= c.z; ++bin; }
        }
    }
    if constexpr (MODE == CS_PICK_LENGTH) {
        // the cells shorter than the answer stay in the set (they sort below it), so the rank stays
        j.prefix[col] = 0;
        j.rem[col] = (int32_t)(bin > 8 ? 8 : bin);
        j.rank[col] = rank;
        atomicMax(&j.flags[0], bin > 8 ? 8u : bin);
    } else {
        j.prefix[col] = (prefix << 8) | bin;
        j.rem[col] = rem - 1;
        j.rank[col] = left;
    }
}

template <int MODE>
__global__ __launch_bounds__(CS_PICK_WAVES * 64) void gd_colselect_pick_kernel(CsJob j)
{
    cs_pick<MODE>(j);
}

// the first pick of a float matrix with the rank rows / 2 over ALL cells, zeros included: the upper median dcnv's Log2
// scaler centres a sample on (gd_svdlog2.hpp).  A kernel of its own, so that the three instances above stay what they were.
__global__ __launch_bounds__(CS_PICK_WAVES * 64) void gd_colmid_pick_kernel(CsJob j)
{
    cs_pick<CS_PICK_FLOAT_MID>(j);
}

}  // namespace gd
