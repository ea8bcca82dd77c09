// gd_svddebias.hpp -- dcnv's SVD debiaser (dcnv/debiaser/debiaser.go:173-200 of the reference) flanked by its z-score
// scaler (dcnv/scalers/scalers.go:24-56) on a row-major [rows][samples] float32 matrix.  The
// singular vectors come from the samples x samples Gram matrix G = Z^T Z, whose eigenpairs the host solves (gd_eigh.hpp):
// 2 <= samples <= SV_MAX_N bounds that O(N^3) solve and the registers a row takes in the projection.  Z is never stored:
// z = (a - m_row) / sd_row (0 for a row whose sd is 0; z = a without the z-score) is formed in float64 where it is used,
// by the one expression sv_z() in both passes.
//
// The Gram kernel and the projection are templates over a scaler policy P, which supplies what the scalers differ in and
// nothing else: Row, a row's state, and row() that loads it; Col, a column's state, and col(); z() from a cell; back() from
// z' to a float32 depth (row() and col() load nothing where their last argument is false: a row past the slab, a column
// past N).  SvLinear below is "none" and the z-score, told apart by the job's zscore field when the kernel
// runs; SvLog2 is gd_svdlog2.hpp's.  Tiles, slabs, chunks, LDS and the order of additions are the same for every scaler
// because there is one text of them.
//
//   gd_svd_rowstats_kernel    a wave per row: m = sum / N, sd = sqrt(sum (a - m)^2 / (N - 1)), two passes in float64
//                             (lane l sums columns l, l + 64, ...; the lanes meet in an xor butterfly, which leaves the
//                             same bits in every lane) into stats[row][2].
//   gd_svd_gram_kernel<P>     a workgroup of 256 threads owns a (slab of SV_SLAB rows, pair of 64-column tiles ti <= tj):
//                             only the upper triangle of tiles is computed.  SV_CHUNK rows at a time, the z of both
//                             tiles' columns go to LDS as float64 (2 x 16 x 64 x 8 bytes = 16 KB; a thread converts the
//                             two cells of one row and column, 256-byte rows of loads), and every thread adds the
//                             chunk's products to its 4 x 4 corner of the 64 x 64 block of G: plain v_fma_f64, rows in
//                             ascending order.  Rows past the slab and columns past N enter as zeros.  The block goes to
//                             part[pair][slab] with plain stores.  (A v_mfma_f64_16x16x4_f64 kernel fed from global
//                             memory gave the same bits in 1.65 times the time)
//   gd_svd_gram_sum_kernel    G[i][j] = G[j][i] = the partials of (i, j), i <= j, summed IN SLAB ORDER: no float atomics,
//                             so two calls give the same bytes, and G is symmetric to the bit.
//   gd_svd_project_kernel<P, NV>
//                             a wave per row, the row's z in NV = ceil(N / 64) registers a lane (1, 2, 4, 8 or 16):
//                             c_k = sum_j z_j V[j][k] by the same butterfly for each of the n removed vectors,
//                             z' = z - sum_k c_k V[j][k], then out = P::back(z'): (float)z', or (float)max(0, z' sd + m)
//                             with the z-score.  A column's state is loaded where it is used, not held.  A lane reads
//                             its own columns before it writes them: out may be the input.  V is read as vt[k][j] straight from global memory -- n x N float64, 24 KB at 200 samples and
//                             n = 15, at most 120 KB: every wave of the device reads the same lines, so they stay in the
//                             vector L1 / L2.  A copy in LDS would need 120 KB at the limits, one workgroup a CU, and a
//                             staging pass per workgroup; the loads it would save are L1 hits behind the row's own
//                             stream from HBM.  n = 0 runs no arithmetic of the projection and still writes out.
//
// No scratch, no atomics; LDS in the Gram kernel only.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gd {

constexpr int SV_MIN_N = 2;
constexpr int SV_MAX_N = 1024;                   // samples: the host's O(N^3) solve, 16 float64 a lane in the projection
constexpr int SV_MAX_K = 15;                     // components the reference removes at most
constexpr int SV_TILE = 64;                      // columns of a Gram tile
constexpr int SV_SLAB = 1024;                    // rows of a Gram workgroup
constexpr int SV_WG = 256;                       // four waves
constexpr int SV_CHUNK = 16;                     // rows of a slab in LDS at a time
constexpr int SV_MAX_GRID = 4096;                // workgroups of the row kernels; the rows beyond are strided over them

struct SvJob {
    const float* cells;                          // [n_rows][n]
    float* out;                                  // [n_rows][n]; may be cells
    int64_t n_rows;
    int32_t n;
    int32_t zscore;
    double* stats;                               // [n_rows][2] mean, sd (zscore only)
    double* part;                                // [pairs][slabs][64][64]
    double* gram;                                // [n][n]
    const double* vt;                            // [n_removed][n]
    int32_t n_removed;
    int32_t slabs;
    const uint64_t* keys;                        // [n] the select's answers: a float's bits in the low word (log2 only)
    double* centre;                              // [n] log2(1 + m_j) (log2 only)
};

// the same bits in every lane: at each step both partners add the same two values
__device__ __forceinline__ double sv_wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ double sv_inv(double sd) { return sd > 0.0 ? 1.0 / sd : 0.0; }
__device__ __forceinline__ double sv_z(float a, double m, double inv) { return ((double)a - m) * inv; }

// "none" and the z-score: a row's mean and sd from stats (0 and 1 without the z-score), nothing for a column
struct SvLinear {
    struct Row { double m = 0.0, sd = 1.0, inv = 1.0; };
    struct Col {};
    static __device__ __forceinline__ Row row(const SvJob& j, int64_t row, bool ok)
    {
        Row r;
        if (j.zscore && ok) {
            r.m = j.stats[2 * (size_t)row];
            r.sd = j.stats[2 * (size_t)row + 1];
            r.inv = sv_inv(r.sd);
        }
        return r;
    }
    static __device__ __forceinline__ Col col(const SvJob&, int, bool) { return Col{}; }
    static __device__ __forceinline__ double z(float a, const Row& r, const Col&) { return sv_z(a, r.m, r.inv); }
    static __device__ __forceinline__ float back(const SvJob& j, double zp, const Row& r, const Col&)
    {
        if (j.zscore) {
            zp = zp * r.sd + r.m;
            zp = zp > 0.0 ? zp : 0.0;
        }
        return (float)zp;
    }
};

__global__ __launch_bounds__(SV_WG) void gd_svd_rowstats_kernel(SvJob j)
{
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int n = j.n;
    for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < j.n_rows; row += (int64_t)gridDim.x * 4) {
        const float* a = j.cells + (size_t)row * (size_t)n;
        double s = 0;
        for (int c = lane; c < n; c += 64) s += (double)a[c];
        const double m = sv_wave_sum(s) / (double)n;
        double q = 0;
        for (int c = lane; c < n; c += 64) {
            const double d = (double)a[c] - m;
            q += d * d;
        }
        const double sd = sqrt(sv_wave_sum(q) / (double)(n - 1));
        if (lane == 0) {
            j.stats[2 * (size_t)row] = m;
            j.stats[2 * (size_t)row + 1] = sd;
        }
    }
}

// blockIdx.x the slab, blockIdx.y the pair of tiles: pairs are numbered row by row of the upper triangle
template <class P>
__global__ __launch_bounds__(SV_WG) void gd_svd_gram_kernel(SvJob j)
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
    const typename P::Col cola = P::col(j, ca, ca < n), colb = P::col(j, cb, cb < n);
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
            const typename P::Row rs = P::row(j, row, ok);
            const float* src = j.cells + (size_t)(ok ? row : r0) * (size_t)n;
            za[4 * u + lr][lc] = ok && ca < n ? P::z(src[ca], rs, cola) : 0.0;
            zb[4 * u + lr][lc] = ok && cb < n ? P::z(src[cb], rs, colb) : 0.0;
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

// blockIdx.y the pair, blockIdx.x a sixteenth of its 64 x 64 block
__global__ __launch_bounds__(SV_WG) void gd_svd_gram_sum_kernel(SvJob j)
{
#pragma clang fp contract(off)
    const int n = j.n;
    const int T = (n + SV_TILE - 1) / SV_TILE;
    int ti = 0, p = (int)blockIdx.y;
    while (p >= T - ti) { p -= T - ti; ++ti; }
    const int tj = ti + p;
    const int e = (int)blockIdx.x * SV_WG + (int)threadIdx.x;
    const int gi = ti * SV_TILE + (e >> 6), gj = tj * SV_TILE + (e & 63);
    if (gi >= n || gj >= n || gi > gj) return;
    const double* part = j.part + (size_t)blockIdx.y * (size_t)j.slabs * (size_t)(SV_TILE * SV_TILE) + (size_t)e;
    double g = 0;
    for (int s = 0; s < j.slabs; ++s) g += part[(size_t)s * (size_t)(SV_TILE * SV_TILE)];
    j.gram[(size_t)gi * (size_t)n + (size_t)gj] = g;
    j.gram[(size_t)gj * (size_t)n + (size_t)gi] = g;
}

template <class P, int NV>
__global__ __launch_bounds__(SV_WG) void gd_svd_project_kernel(SvJob j)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int n = j.n;
    const int K = j.n_removed;
    for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < j.n_rows; row += (int64_t)gridDim.x * 4) {
        const float* a = j.cells + (size_t)row * (size_t)n;
        const typename P::Row rs = P::row(j, row, true);
        double z[NV], dz[NV];
#pragma unroll
        for (int u = 0; u < NV; ++u) {
            const int c = lane + 64 * u;
            z[u] = c < n ? P::z(a[c], rs, P::col(j, c, true)) : 0.0;
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
            if (c < n) o[c] = P::back(j, z[u] - dz[u], rs, P::col(j, c, true));
        }
    }
}

}  // namespace gd
