// gd_devmat.hpp -- what a row-major [rows][samples] depth matrix needs to stay in HBM between the consumers of DESIGN.md
// sections 3.10 - 3.13 (section 3.14): the int64 cells gd_depthwed_device leaves become the float32 matrix the float
// kernels read, a float32 matrix a caller hands over is held to what the host entry points hold theirs to, and the
// per-sample factors of `emdepth --scales` are applied in place.  Three streaming kernels, one pass each:
//
//   gd_devmat_from_cells_kernel   out = (float)cell: one rounding, to nearest even, the conversion em_depth does in
//                                 gd_emdepth.hpp.  flag[0] becomes 1 when any cell is negative.
//   gd_devmat_check_kernel        first[0] becomes the lowest flat index of a cell that is not (finite and >= 0), decided
//                                 on the bit pattern so that no denormal mode matters: a cell passes when its bits are
//                                 below +inf's, or are -0.0's -- what the host's !(d >= 0) || !isfinite(d) lets pass.
//                                 first[0] starts as all ones (no such cell).
//   gd_devmat_scale_kernel        in place, d = d * scale[s] in float32, not contracted: the one multiplication
//                                 `emdepth --scales` does per cell on the host.
//
// Lanes run along samples as in gd_colselect.hpp and gd_chunkdebias.hpp (lane l of the y-th column tile owns column
// 64 y + l, so a wave's access to a row is 64 consecutive cells); a wave owns a row at a time, the row index wave-uniform,
// DM_ROWS rows in flight a turn, and a grid-stride loop over the rows (at most DM_MAX_GRID workgroups of DM_WAVES waves a
// column tile).  A lane reads and writes its own indices only, so scaling in place is safe.  What a wave found meets in
// its first lane, which issues the one global atomic.  No LDS, no scratch: the cells in flight are an unrolled array.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gd {

constexpr int DM_WAVES = 4;                      // waves of a workgroup: rows of its turn
constexpr int DM_WG = DM_WAVES * 64;
constexpr int DM_ROWS = 4;                       // rows a wave has in flight
constexpr int DM_COLS = 64;                      // columns of a workgroup: one per lane
constexpr int DM_MAX_GRID = 2048;                // workgroups of a column tile; the rows beyond are strided over them
constexpr int DM_MAX_N = 4096;

struct DmJob {
    const int64_t* cells;                        // [n_rows][n] (from_cells)
    float* depths;                               // [n_rows][n] from_cells: out; check: read only; scale: in place
    const float* scale;                          // [n] (scale)
    int64_t n_rows;
    int32_t n;
    uint32_t* flag;                              // one word, zero before (from_cells)
    unsigned long long* first;                   // one word, all ones before (check)
};

__global__ __launch_bounds__(DM_WG) void gd_devmat_from_cells_kernel(DmJob j)
{
    const int lane = threadIdx.x & 63;
    const int col = (int)blockIdx.y * DM_COLS + lane;
    const size_t n = (size_t)j.n;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t step = (int64_t)gridDim.x * DM_WAVES;
    bool negative = false;
    if (col < j.n) {
        int64_t row = (int64_t)blockIdx.x * DM_WAVES + wave;
        for (; row + (DM_ROWS - 1) * step < j.n_rows; row += DM_ROWS * step) {       // a whole turn: DM_ROWS loads in flight
            int64_t v[DM_ROWS];
#pragma unroll
            for (int u = 0; u < DM_ROWS; ++u) v[u] = j.cells[(size_t)(row + u * step) * n + (size_t)col];
#pragma unroll
            for (int u = 0; u < DM_ROWS; ++u) {
                negative |= v[u] < 0;
                j.depths[(size_t)(row + u * step) * n + (size_t)col] = (float)v[u];
            }
        }
        for (; row < j.n_rows; row += step) {    // the last rows
            const int64_t v = j.cells[(size_t)row * n + (size_t)col];
            negative |= v < 0;
            j.depths[(size_t)row * n + (size_t)col] = (float)v;
        }
    }
    if (__any(negative) && lane == 0) atomicOr(j.flag, 1u);
}

// a float32 the host entry points refuse, by its bits: above +inf's (NaN, every negative but -0.0) or +inf's own
__device__ __forceinline__ bool dm_refused(uint32_t bits) { return bits >= 0x7f800000u && bits != 0x80000000u; }

__global__ __launch_bounds__(DM_WG) void gd_devmat_check_kernel(DmJob j)
{
    const int lane = threadIdx.x & 63;
    const int col = (int)blockIdx.y * DM_COLS + lane;
    const size_t n = (size_t)j.n;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t step = (int64_t)gridDim.x * DM_WAVES;
    const uint32_t* cells = reinterpret_cast<const uint32_t*>(j.depths);
    unsigned long long first = ~0ull;            // the rows ascend: the first cell this lane refuses is its lowest
    if (col < j.n) {
        int64_t row = (int64_t)blockIdx.x * DM_WAVES + wave;
        for (; row + (DM_ROWS - 1) * step < j.n_rows; row += DM_ROWS * step) {
            uint32_t v[DM_ROWS];
#pragma unroll
            for (int u = 0; u < DM_ROWS; ++u) v[u] = cells[(size_t)(row + u * step) * n + (size_t)col];
#pragma unroll
            for (int u = 0; u < DM_ROWS; ++u)
                if (dm_refused(v[u]) && first == ~0ull) first = (unsigned long long)((size_t)(row + u * step) * n + (size_t)col);
        }
        for (; row < j.n_rows; row += step)
            if (dm_refused(cells[(size_t)row * n + (size_t)col]) && first == ~0ull)
                first = (unsigned long long)((size_t)row * n + (size_t)col);
    }
    if (!__any(first != ~0ull)) return;          // (wave-uniform)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(first, o, 64);
        first = other < first ? other : first;
    }
    if (lane == 0) atomicMin(j.first, first);
}

__global__ __launch_bounds__(DM_WG) void gd_devmat_scale_kernel(DmJob j)
{
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int col = (int)blockIdx.y * DM_COLS + lane;
    const size_t n = (size_t)j.n;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t step = (int64_t)gridDim.x * DM_WAVES;
    if (col >= j.n) return;
    const float f = j.scale[col];
    int64_t row = (int64_t)blockIdx.x * DM_WAVES + wave;
    for (; row + (DM_ROWS - 1) * step < j.n_rows; row += DM_ROWS * step) {
        float v[DM_ROWS];
#pragma unroll
        for (int u = 0; u < DM_ROWS; ++u) v[u] = j.depths[(size_t)(row + u * step) * n + (size_t)col];
#pragma unroll
        for (int u = 0; u < DM_ROWS; ++u) j.depths[(size_t)(row + u * step) * n + (size_t)col] = v[u] * f;
    }
    for (; row < j.n_rows; row += step) {
        const size_t at = (size_t)row * n + (size_t)col;
        j.depths[at] = j.depths[at] * f;
    }
}

}  // namespace gd
