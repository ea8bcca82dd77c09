// gd_chunkdebias.hpp -- dcnv's ChunkDebiaser (dcnv/debiaser/debiaser.go:125-171 of the reference) on a row-major
// [rows][samples] float32 matrix: the rows are cut into chunks by a covariate (GC), every sample's
// cells in a chunk are divided by their "median", sorted[(n - k) / 2] with n the rows of the chunk and k the sample's zeros
// in it.  The matrix is not permuted: the host hands over order[R] (the rows in ascending covariate order), slices[C + 1]
// (where each chunk starts in order) and chunk_of_row[R], so the reference's Sort and Unsort cost nothing.
//
//   gd_chunkdebias_median_kernel   a workgroup owns one (chunk, 64-column tile) at a time (blockIdx.y the tile, the chunks
//                                  strided over blockIdx.x) and runs the whole most-significant-digit-first radix select
//                                  itself: four 8-bit passes over the chunk's own rows, nothing global between them.
//                                  Lanes run along samples as in gd_colselect.hpp (lane l owns column 64 y + l; a wave's
//                                  load of a row is 64 consecutive cells); the CD_WAVES waves take the chunk's rows through
//                                  order[], CD_ROWS each a turn, the row index wave-uniform.  The counts are in LDS as
//                                  [bin][column]: lane l only touches words that are l mod 64, no bank twice in a
//                                  half-wave.  Between passes wave w reads (and zeroes) bins 32 w .. 32 w + 31 of its
//                                  lane's column into registers, the eight sums meet in LDS, and the one wave whose bins
//                                  hold the column's rank walks its registers: the prefix one digit longer, the rank left
//                                  inside the bin.  The first pass also counts the exact zeros (-0.0 is one) and sets the
//                                  rank (n - k) / 2.  The answer goes to med[chunk][sample]; no global atomics.
//   gd_chunkdebias_divide_kernel   lanes along samples again, a wave a row: q = (double)d / (double)med[chunk_of_row[r]][s]
//                                  when the median is > 0, (double)d otherwise; writes (float)q and, when asked, q.
//
// The keys are the cells' bit patterns (non-negative floats order as their bits do), read as integers so that no
// denormal mode matters.  LDS: 256 x 64 counters (64 KB) + 8 x 64 sums + 3 x 64 words of column state = 68 352 bytes a
// workgroup, designed for TWO workgroups of 512 threads per CU as gd_colselect.hpp is (sixteen waves, four per SIMD, at most
// 128 registers a lane).  No scratch: the cells in flight and the 32 bins of a wave are unrolled arrays.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gd {

constexpr int CD_WAVES = 8;                      // waves of a median workgroup
constexpr int CD_WG = CD_WAVES * 64;
constexpr int CD_ROWS = 8;                       // rows a wave has in flight: a wave-turn
constexpr int CD_TURN = CD_WAVES * CD_ROWS;      // rows of a workgroup's turn
constexpr int CD_COLS = 64;                      // columns of a workgroup: one per lane
constexpr int CD_BINS = 256;
constexpr int CD_SEG = CD_BINS / CD_WAVES;       // bins a wave scans between passes
constexpr int CD_WG_PER_CU = 2;
constexpr int CD_MAX_GRID = 4096;                // workgroups of a column tile; the chunks beyond are strided over them
constexpr int CD_MAX_N = 4096;
constexpr int CD_DIV_WAVES = 4;                  // rows of a divide workgroup's turn
constexpr int CD_DIV_MAX_GRID = 8192;

struct CdJob {
    const uint32_t* cells;                       // [n_rows][n] float32, as bits
    int64_t n_rows;
    int32_t n;
    uint32_t n_chunks;
    const uint32_t* order;                       // [n_rows] rows in ascending covariate order
    const uint32_t* slices;                      // [n_chunks + 1] chunk c is order[slices[c] .. slices[c + 1])
    const uint32_t* chunk_of_row;                // [n_rows]
    uint32_t* med;                               // [n_chunks][n] the medians, as bits (a zero is +0.0)
    float* out;                                  // [n_rows][n]
    double* out64;                               // [n_rows][n] or null
};

__device__ __forceinline__ uint32_t cd_key(uint32_t bits)
{
    return (bits << 1) ? bits : 0u;              // (-0 is 0; the caller refused every other negative)
}

__global__ __launch_bounds__(CD_WG) void gd_chunkdebias_median_kernel(CdJob j)
{
    __shared__ uint32_t hist[CD_BINS * CD_COLS];
    __shared__ uint32_t part[CD_WAVES * CD_COLS];
    __shared__ uint32_t s_prefix[CD_COLS], s_rank[CD_COLS], s_zeros[CD_COLS];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int col = (int)blockIdx.y * CD_COLS + lane;
    const int n = j.n;
    const bool live = col < n;
    for (int i = threadIdx.x; i < CD_BINS * CD_COLS; i += CD_WG) hist[i] = 0;

    for (uint32_t chunk = blockIdx.x; chunk < j.n_chunks; chunk += gridDim.x) {
        const uint32_t lo = j.slices[chunk], hi = j.slices[chunk + 1];
        if (wave == 0) { s_prefix[lane] = 0; s_rank[lane] = 0; s_zeros[lane] = 0; }
        __syncthreads();                         // (also: the counters are zero, and the last chunk's state was read)
#pragma unroll 1
        for (int pass = 0; pass < 4; ++pass) {
            const int shift = 24 - 8 * pass;
            const uint32_t prefix = s_prefix[lane];
            uint32_t zeros = 0;
            const auto count = [&](uint32_t bits) {
                const uint32_t k = cd_key(bits);
                if (pass == 0) zeros += k == 0 ? 1u : 0u;
                else if (((k >> shift) >> 8) != prefix) return;
                atomicAdd(&hist[((k >> shift) & 255u) * CD_COLS + lane], 1u);
            };
            if (live) {
                for (uint32_t base = lo; base < hi; base += CD_TURN) {
                    const uint32_t* at = j.order + base + wave;
                    if (hi - base >= (uint32_t)CD_TURN) {      // a whole turn: CD_ROWS loads in flight, no row is tested
                        uint32_t v[CD_ROWS];
#pragma unroll
                        for (int u = 0; u < CD_ROWS; ++u) {
                            const uint32_t row = __builtin_amdgcn_readfirstlane(at[u * CD_WAVES]);
                            v[u] = j.cells[(size_t)row * (size_t)n + (size_t)col];
                        }
#pragma unroll
                        for (int u = 0; u < CD_ROWS; ++u) count(v[u]);
                    } else {                     // the chunk's last rows
#pragma unroll
                        for (int u = 0; u < CD_ROWS; ++u)
                            if (base + (uint32_t)(u * CD_WAVES + wave) < hi) {
                                const uint32_t row = __builtin_amdgcn_readfirstlane(at[u * CD_WAVES]);
                                count(j.cells[(size_t)row * (size_t)n + (size_t)col]);
                            }
                    }
                }
            }
            if (pass == 0 && zeros) atomicAdd(&s_zeros[lane], zeros);
            __syncthreads();
            // this wave's CD_SEG bins of the lane's column, left zero for the next pass
            uint32_t c[CD_SEG], own = 0;
#pragma unroll
            for (int i = 0; i < CD_SEG; ++i) {
                uint32_t* p = &hist[(wave * CD_SEG + i) * CD_COLS + lane];
                c[i] = *p;
                *p = 0;
                own += c[i];
            }
            part[wave * CD_COLS + lane] = own;
            __syncthreads();
            // the rank (n - k) / 2 counts from the start of the sorted chunk, zeros included (debiaser.go:161)
            uint32_t rank = pass == 0 ? ((hi - lo) - s_zeros[lane]) / 2u : s_rank[lane];
            uint32_t excl = 0;
#pragma unroll
            for (int w = 0; w < CD_WAVES; ++w) excl += w < wave ? part[w * CD_COLS + lane] : 0u;
            __syncthreads();                     // (every wave has read the rank before one of them replaces it)
            if (rank >= excl && rank < excl + own) {           // one wave of the column goes on
                uint32_t left = rank - excl, bin = 0;
                bool found = false;
#pragma unroll
                for (int i = 0; i < CD_SEG; ++i) {
                    if (!found && left < c[i]) { found = true; bin = (uint32_t)(wave * CD_SEG + i); }
                    if (!found) left -= c[i];
                }
                s_prefix[lane] = (prefix << 8) | bin;
                s_rank[lane] = left;
            }
            __syncthreads();
        }
        if (wave == 0 && live) j.med[(size_t)chunk * (size_t)n + (size_t)col] = s_prefix[lane];
    }
}

__global__ __launch_bounds__(CD_DIV_WAVES * 64) void gd_chunkdebias_divide_kernel(CdJob j)
{
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int col = (int)blockIdx.y * CD_COLS + lane;
    const int n = j.n;
    if (col >= n) return;
    for (int64_t row = (int64_t)blockIdx.x * CD_DIV_WAVES + wave; row < j.n_rows; row += (int64_t)gridDim.x * CD_DIV_WAVES) {
        const uint32_t chunk = j.chunk_of_row[row];
        const size_t at = (size_t)row * (size_t)n + (size_t)col;
        const uint32_t m = j.med[(size_t)chunk * (size_t)n + (size_t)col];
        double q = (double)__uint_as_float(j.cells[at]);
        if (m != 0u) q = q / (double)__uint_as_float(m);       // (the median is a key: never negative, a zero is 0)
        j.out[at] = (float)q;
        if (j.out64) j.out64[at] = q;
    }
}

}  // namespace gd
