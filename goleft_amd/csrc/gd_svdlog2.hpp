// gd_svdlog2.hpp -- dcnv's Log2 scaler (dcnv/scalers/scalers.go:134-164 of the reference, through ColCentered{gmean},
// :63-100 and :126-132) around the SVD debiaser of gd_svddebias.hpp: l = log2(1 + a), every SAMPLE
// centred on its upper median over all rows, c_j = sorted(l_.j)[rows / 2], zeros included; the cut and the projection of
// section 3.16 on z = l - c; out = max(0, 2^(z' + c) - 1), one rounding to float32.
//
// Two definitions of this project's, where the reference's own test and its code disagree:
//   the "- 1"   the reference's UnScale returns 2^x, so a round trip gives depth + 1 and its TestLog2RoundTrip
//               (scalers_test.go:49-79), which wants the input back within 0.001, fails.  The test's contract is served.
//   the clamp   a zero cell can leave the projection with a negative exponent: max(0, .), as ZScore.UnScale has it.
//
// log2 is monotone, so c_j = log2(1 + m_j) with m_j the rows / 2-th smallest raw cell of the column: gd_colselect.hpp's
// radix select finds m_j on the float32 bits (gd_colmid_pick_kernel), and nothing is sorted.
//
//   gd_svl_centre_kernel        centre[j] = sl_log(m_j), float64, from the select's keys: the same routine the cells go
//                               through, so a cell that IS its column's centre gives z = 0 exactly.
//   gd_svl_gram_kernel          gd_svd_gram_kernel with z = sl_z(a, centre[column]): the same tiles, slabs, chunks, LDS and
//                               order of additions; gd_svd_gram_sum_kernel sums its partials in slab order.
//   gd_svl_project_kernel<NV>   gd_svd_project_kernel<NV> with the same z, and out = (float)max(0, exp2(z' + c) - 1).  A
//                               lane reads its own columns before it writes them: out may be the input.
//
// z is never stored: log2 in float64 is a software routine of a few dozen instructions, and the Gram kernel converts a cell
// once per pair of tiles its column is in.  A form that staged l once as float64 (8 bytes a cell) was measured beside this
// one: its kernels were faster and its call slower, by the allocation of twice the matrix; DESIGN.md section 3.17 has the
// table.  No scratch, no atomics; LDS in the Gram kernel only.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gd_svddebias.hpp"

namespace gd {

struct SlJob {
    const float* cells;                          // [n_rows][n]
    float* out;                                  // [n_rows][n]; may be cells
    int64_t n_rows;
    int32_t n;
    int32_t slabs;
    const uint64_t* keys;                        // [n] the select's answers: a float's bits in the low word
    double* centre;                              // [n] log2(1 + m_j)
    double* part;                                // [pairs][slabs][64][64]
    const double* vt;                            // [n_removed][n]
    int32_t n_removed;
};

__device__ __forceinline__ double sl_log(float a) { return log2(1.0 + (double)a); }
__device__ __forceinline__ double sl_z(float a, double ce) { return sl_log(a) - ce; }

__global__ __launch_bounds__(SV_WG) void gd_svl_centre_kernel(SlJob j)
{
    const int i = (int)blockIdx.x * SV_WG + (int)threadIdx.x;
    if (i < j.n) j.centre[i] = sl_log(__uint_as_float((uint32_t)j.keys[i]));
}

// blockIdx.x the slab, blockIdx.y the pair of tiles, as in gd_svd_gram_kernel
__global__ __launch_bounds__(SV_WG) void gd_svl_gram_kernel(SlJob j)
{
    __shared__ double za[SV_CHUNK][SV_TILE], zb[SV_CHUNK][SV_TILE];
    const int tid = threadIdx.x;
    const int n = j.n;
    const int T = (n + SV_TILE - 1) / SV_TILE;
    int ti = 0, p = (int)blockIdx.y;
    while (p >= T - ti) { p -= T - ti; ++ti; }
    const int tj = ti + p;
    const int64_t r0 = (int64_t)blockIdx.x * SV_SLAB;
    const int64_t r1 = r0 + SV_SLAB < j.n_rows ? r0 + SV_SLAB : j.n_rows;
    const int ty = tid >> 4, tx = tid & 15;                  // the thread's 4 x 4 of the block: rows 4 ty .., columns 4 tx ..
    const int lr = tid >> 6, lc = tid & 63;                  // as a loader: row lr of every four, column lc of both tiles
    const int ca = ti * SV_TILE + lc, cb = tj * SV_TILE + lc;
    const double cea = ca < n ? j.centre[ca] : 0.0, ceb = cb < n ? j.centre[cb] : 0.0;
    double acc[4][4];
#pragma unroll
    for (int x = 0; x < 4; ++x)
#pragma unroll
        for (int y = 0; y < 4; ++y) acc[x][y] = 0.0;

    for (int64_t r = r0; r < r1; r += SV_CHUNK) {
        __syncthreads();                         // (the chunk before this one has been read)
#pragma unroll
        for (int u = 0; u < SV_CHUNK / 4; ++u) {
            const int64_t row = r + 4 * u + lr;
            const bool ok = row < r1;
            const float* src = j.cells + (size_t)(ok ? row : r0) * (size_t)n;
            za[4 * u + lr][lc] = ok && ca < n ? sl_z(src[ca], cea) : 0.0;
            zb[4 * u + lr][lc] = ok && cb < n ? sl_z(src[cb], ceb) : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < SV_CHUNK; ++k) {
            double a[4], b[4];
#pragma unroll
            for (int x = 0; x < 4; ++x) {
                a[x] = za[k][ty * 4 + x];
                b[x] = zb[k][tx * 4 + x];
            }
#pragma unroll
            for (int x = 0; x < 4; ++x)
#pragma unroll
                for (int y = 0; y < 4; ++y) acc[x][y] += a[x] * b[y];
        }
    }

    double* part = j.part + ((size_t)blockIdx.y * (size_t)j.slabs + (size_t)blockIdx.x) * (size_t)(SV_TILE * SV_TILE);
#pragma unroll
    for (int x = 0; x < 4; ++x)
#pragma unroll
        for (int y = 0; y < 4; ++y) part[(ty * 4 + x) * SV_TILE + tx * 4 + y] = acc[x][y];
}

template <int NV>
__global__ __launch_bounds__(SV_WG) void gd_svl_project_kernel(SlJob j)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int n = j.n;
    const int K = j.n_removed;
    for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < j.n_rows; row += (int64_t)gridDim.x * 4) {
        const float* a = j.cells + (size_t)row * (size_t)n;
        double z[NV], dz[NV];
#pragma unroll
        for (int u = 0; u < NV; ++u) {
            const int c = lane + 64 * u;
            z[u] = c < n ? sl_z(a[c], j.centre[c]) : 0.0;
            dz[u] = 0.0;
        }
        for (int k = 0; k < K; ++k) {
            const double* v = j.vt + (size_t)k * (size_t)n;
            double vv[NV];
            double t = 0.0;
#pragma unroll
            for (int u = 0; u < NV; ++u) {
                const int c = lane + 64 * u;
                vv[u] = c < n ? v[c] : 0.0;
                t += z[u] * vv[u];
            }
            t = sv_wave_sum(t);
#pragma unroll
            for (int u = 0; u < NV; ++u) dz[u] += t * vv[u];
        }
        float* o = j.out + (size_t)row * (size_t)n;
#pragma unroll
        for (int u = 0; u < NV; ++u) {
            const int c = lane + 64 * u;
            if (c < n) {
                const double r = exp2((z[u] - dz[u]) + j.centre[c]) - 1.0;
                o[c] = (float)(r > 0.0 ? r : 0.0);
            }
        }
    }
}

}  // namespace gd
