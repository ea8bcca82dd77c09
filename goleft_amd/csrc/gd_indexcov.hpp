// gd_indexcov.hpp -- `goleft indexcov` (indexcov/indexcov.go, types.go of the reference) on the tile sizes of a
// cohort of .bai linear indexes.
//
//   gd_ic_median_kernel     Index.init (:83-125): per sample the 98th-percentile cap and the capped weighted median,
//                           found by two radix selects over the unsorted sizes (no sort, nothing written but the result)
//   gd_ic_depth_kernel      NormalizedDepth (:129-151): float32(float64(size) / median), capped at 50 000
//   gd_ic_pass_kernel       one workgroup per (sample, reference): the %.3g cell of every tile, the 70 CountsAtDepth
//                           slots (:170-177), counter.count (:1062-1078) and the pca8 bytes (:688-705)
//   gd_ic_cn_kernel         GetCN (:957-991) of one sex reference: a radix select over the non-zero depths
//   gd_ic_rowsum_kernel /   the exact Gram matrix G = X * X^T of the pca8 bytes: signed 8-bit MFMA on bytes biased
//   gd_ic_gram_kernel /     by -128, 32-bit accumulators flushed to 64 bits every IC_KCHUNK columns, corrected
//   gd_ic_gram_fin_kernel   with the row sums
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gd_round3g.hpp"

namespace gd {

constexpr int IC_SLOTS = 70;                     // indexcov.go:153
constexpr int IC_WG = 256;
constexpr int IC_KSTEP = 64;                     // columns of one MFMA
constexpr int IC_KCHUNK = 16384;                 // columns between two flushes: 128^2 * 16384 = 2^28 < 2^31
constexpr int IC_BLOCK = 32;                     // samples of a Gram block (2 x 2 MFMA tiles)

struct IcJob {
    int32_t n_samples, n_refs;
    const int64_t* sizes;                        // every tile of every sample, sample after sample, reference after reference
    const int64_t* sample_off;                   // [n_samples + 1] into sizes
    const int64_t* tile_off;                     // [n_samples * n_refs] into sizes: the tiles of a kept reference
    const int32_t* tile_cnt;                     // [n_samples * n_refs] (0 for a sample whose median is 0)
    const uint8_t* is_sex;                       // [n_refs]
    const int32_t* longest;                      // [n_refs]
    const int64_t* cell_off;                     // [n_refs] into cells: longest[r] rows of n_samples
    const int64_t* col_off;                      // [n_refs] into a row of X (non-sex references)
    int64_t* median;                             // [n_samples]
    float* depth;                                // parallel to sizes
    uint32_t* cells;
    int32_t* slots;                              // [n_refs][n_samples][70]
    unsigned long long* counters;                // [n_samples][4]: out, low, hi, in
    double* cn;                                  // [n_refs][n_samples]
    uint8_t* X;                                  // [n_pad][m_pad]
    int64_t m_pad;
};

__device__ __forceinline__ unsigned long long ic_wg_sum(unsigned long long v, unsigned long long* lds)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    __syncthreads();                             // (lds may still be read from the previous call)
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned long long t = 0;
    for (int w = 0; w < IC_WG / 64; ++w) t += lds[w];
    return t;
}

// One workgroup per sample.  (The sizes are re-read from memory once per bit of the largest size, for each of the two
// selects -- about 70 passes, most of indexcov's device time.  The next step is a radix select with 8-bit histograms in
// LDS: 8 passes per select.)  sorted[k] of the reference is the smallest v with #{s <= v} > k; the median is the
// smallest v with sum{min(s, n98) : s <= v} > total / 2.  Both are found bit by bit from the top.
__global__ __launch_bounds__(IC_WG) void gd_ic_median_kernel(IcJob j)
{
    __shared__ unsigned long long lds[IC_WG / 64];
    const int s = blockIdx.x;
    const int64_t a = j.sample_off[s], n = j.sample_off[s + 1] - a;
    const uint64_t* __restrict__ v = reinterpret_cast<const uint64_t*>(j.sizes + a);
    if (n <= 0) { if (threadIdx.x == 0) j.median[s] = -1; return; }   // (the host refuses such a sample)
    unsigned long long mx = 0;
    for (int64_t i = threadIdx.x; i < n; i += IC_WG) mx = v[i] > mx ? v[i] : mx;
    for (int o = 32; o > 0; o >>= 1) { const unsigned long long t = __shfl_down(mx, o, 64); mx = t > mx ? t : mx; }
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = mx;
    __syncthreads();
    mx = lds[0];
    for (int w = 1; w < IC_WG / 64; ++w) mx = lds[w] > mx ? lds[w] : mx;
    const int bits = mx ? 64 - __clzll(mx) : 0;
    const unsigned long long k98 = (unsigned long long)(int64_t)(0.98 * (double)n);   // int(0.98 * float64(len))
    unsigned long long n98 = 0;
    for (int b = bits - 1; b >= 0; --b) {
        const unsigned long long t = n98 | ((1ull << b) - 1);
        unsigned long long c = 0;
        for (int64_t i = threadIdx.x; i < n; i += IC_WG) c += v[i] <= t ? 1u : 0u;
        c = ic_wg_sum(c, lds);
        if (c <= k98) n98 |= 1ull << b;
    }
    unsigned long long tot = 0;
    for (int64_t i = threadIdx.x; i < n; i += IC_WG) tot += v[i] < n98 ? v[i] : n98;
    tot = ic_wg_sum(tot, lds);
    const unsigned long long half = (unsigned long long)((int64_t)tot / 2);
    unsigned long long med = 0;
    if (tot == 0) med = mx;                      // no cumulative sum exceeds total / 2 = 0: idx falls back to the last of the sorted sizes
    else
        for (int b = bits - 1; b >= 0; --b) {
            const unsigned long long t = med | ((1ull << b) - 1);
            unsigned long long c = 0;
            for (int64_t i = threadIdx.x; i < n; i += IC_WG) c += v[i] <= t ? (v[i] < n98 ? v[i] : n98) : 0u;
            c = ic_wg_sum(c, lds);
            if (c <= half) med |= 1ull << b;
        }
    if (threadIdx.x == 0) j.median[s] = (int64_t)med;
}

// grid (blocks over the sample's tiles, sample)
__global__ __launch_bounds__(IC_WG) void gd_ic_depth_kernel(IcJob j)
{
    const int s = blockIdx.y;
    const int64_t a = j.sample_off[s], n = j.sample_off[s + 1] - a;
    const double med = (double)j.median[s];
    for (int64_t i = (int64_t)blockIdx.x * IC_WG + threadIdx.x; i < n; i += (int64_t)gridDim.x * IC_WG) {
        float d = 0.f;
        if (med > 0) {
            d = (float)((double)j.sizes[a + i] / med);
            if (d > 50000.f) d = 50000.f;
        }
        j.depth[a + i] = d;
    }
}

// CountsAtDepth's slot: float32 multiply, then float32 add, each rounded on its own (Go on amd64 fuses nothing).
__device__ __forceinline__ int ic_slot(float d)
{
#pragma clang fp contract(off)
    const float c = 70.f * (float)(2.0 / 3.0);   // slots * float32(slotsMid): one rounding of the exact product
    const float p = d * c;
    const float f = p + 0.5f;
    const int v = (int)f;                        // tint (:159-167)
    return v < IC_SLOTS ? (v < 0 ? 0 : v) : IC_SLOTS - 1;
}

// uint8(65535 / MaxCN * dp + 0.5) as Go on amd64 computes it: the float32 reaches 65 535.5, the conversion truncates to an
// integer and keeps its low 8 bits (a quirk of the reference, restated: DESIGN.md section 5).
__device__ __forceinline__ uint8_t ic_pca8(float dp)
{
#pragma clang fp contract(off)
    const float p = 8191.875f * dp;              // float32(65535) / float32(8)
    const float f = p + 0.5f;
    return (uint8_t)((int)f & 0xff);
}

// grid (reference, sample)
__global__ __launch_bounds__(IC_WG) void gd_ic_pass_kernel(IcJob j)
{
    __shared__ int hist[IC_SLOTS];
    __shared__ int cnt4[4];                      // out, low, hi, in
    const int r = blockIdx.x, s = blockIdx.y;
    const int N = j.n_samples;
    const size_t sr = (size_t)s * j.n_refs + r;
    const int n = j.tile_cnt[sr], longest = j.longest[r];
    const bool sex = j.is_sex[r] != 0;
    const float* __restrict__ dep = j.depth + j.tile_off[sr];
    for (int i = threadIdx.x; i < IC_SLOTS; i += IC_WG) hist[i] = 0;
    if (threadIdx.x < 4) cnt4[threadIdx.x] = 0;
    __syncthreads();
    uint32_t* __restrict__ cells = j.cells + j.cell_off[r];
    uint8_t* __restrict__ x = sex ? nullptr : j.X + (size_t)s * j.m_pad + j.col_off[r];
    int c_out = 0, c_low = 0, c_hi = 0, c_in = 0;
    for (int i = threadIdx.x; i < longest; i += IC_WG) {
        if (i >= n) { cells[(size_t)i * N + s] = 0; continue; }      // depthsFor prints "0" past the sample's last tile
        const float d = dep[i];
        cells[(size_t)i * N + s] = gd_round3g(d);
        atomicAdd(&hist[ic_slot(d)], 1);
        if (!sex) {
            const float dp = d > 8.f ? 8.f : d;                      // MaxCN, after the row and the slot were made
            x[i] = ic_pca8(dp);
            if (dp < 0.85f || dp > 1.15f) {
                ++c_out;
                if (dp > 1.15f) ++c_hi;
                else if (dp < 0.15f) ++c_low;
            } else ++c_in;
        }
    }
    // (X was cleared: the zeros behind the sample's tiles, up to longest + 1 bytes, are there already)
    if (!sex) {
        for (int o = 32; o > 0; o >>= 1) {
            c_out += __shfl_down(c_out, o, 64); c_low += __shfl_down(c_low, o, 64);
            c_hi += __shfl_down(c_hi, o, 64); c_in += __shfl_down(c_in, o, 64);
        }
        if ((threadIdx.x & 63) == 0) {
            atomicAdd(&cnt4[0], c_out); atomicAdd(&cnt4[1], c_low); atomicAdd(&cnt4[2], c_hi); atomicAdd(&cnt4[3], c_in);
        }
    }
    __syncthreads();
    int* __restrict__ out = j.slots + ((size_t)r * N + s) * IC_SLOTS;
    for (int i = threadIdx.x; i < IC_SLOTS; i += IC_WG) out[i] = hist[i];
    if (!sex && threadIdx.x < 4) {
        unsigned long long v = (unsigned long long)cnt4[threadIdx.x];
        if (threadIdx.x < 2) v += (unsigned long long)(longest - n);  // missing tiles count as out and low
        if (v) atomicAdd(&j.counters[(size_t)s * 4 + threadIdx.x], v);
    }
}

// grid (reference, sample); references that are not sex references leave at once.
__global__ __launch_bounds__(IC_WG) void gd_ic_cn_kernel(IcJob j)
{
    __shared__ unsigned long long lds[IC_WG / 64];
    const int r = blockIdx.x, s = blockIdx.y;
    if (!j.is_sex[r] || j.longest[r] == 0) return;
    const size_t sr = (size_t)s * j.n_refs + r;
    const int n = j.tile_cnt[sr];
    const uint32_t* __restrict__ u = reinterpret_cast<const uint32_t*>(j.depth + j.tile_off[sr]);   // depths are >= 0: the bits order them
    unsigned long long c = 0;                    // non-zero in the low half, < 0.02 among them in the high half
    const uint32_t lim = __float_as_uint(0.02f);
    for (int i = threadIdx.x; i < n; i += IC_WG) {
        const uint32_t b = u[i];
        if (b) c += 1ull + (b < lim ? 1ull << 32 : 0ull);
    }
    c = ic_wg_sum(c, lds);
    const uint32_t nz = (uint32_t)c, lows = (uint32_t)(c >> 32);
    double med = -0.1;
    if (nz) {
        uint32_t drop = 0;
        if ((double)lows / (double)n > 0.3) drop = lows;             // the share is taken over ALL tiles (:977)
        const uint32_t left = nz - drop;
        med = 0;
        if (left) {
            // rank among the non-zero values, sorted: the zeros sort in front of them
            const unsigned long long k = (unsigned long long)(n - (int)nz) + drop + (unsigned long long)(int64_t)((double)left * 0.4);
            uint32_t v = 0;
            for (int b = 31; b >= 0; --b) {
                const uint32_t t = v | ((1u << b) - 1);
                unsigned long long q = 0;
                for (int i = threadIdx.x; i < n; i += IC_WG) q += u[i] <= t ? 1u : 0u;
                q = ic_wg_sum(q, lds);
                if (q <= k) v |= 1u << b;
            }
            med = (double)(2.f * __uint_as_float(v));                // float32(Ploidy) * tmp[...]
        }
    }
    if (threadIdx.x == 0) j.cn[(size_t)r * j.n_samples + s] = med;
}

// One workgroup per row of X.
__global__ __launch_bounds__(IC_WG) void gd_ic_rowsum_kernel(const uint8_t* __restrict__ X, int64_t m_pad, long long* __restrict__ sums)
{
    __shared__ unsigned long long lds[IC_WG / 64];
    const uint32_t* __restrict__ row = reinterpret_cast<const uint32_t*>(X + (size_t)blockIdx.x * m_pad);
    unsigned long long t = 0;
    for (int64_t i = threadIdx.x; i < m_pad / 4; i += IC_WG) {
        const uint32_t w = row[i];
        t += (w & 0xff) + ((w >> 8) & 0xff) + ((w >> 16) & 0xff) + (w >> 24);
    }
    t = ic_wg_sum(t, lds);
    if (threadIdx.x == 0) sums[blockIdx.x] = (long long)t;
}

typedef int ic_v4i __attribute__((ext_vector_type(4)));

// grid (pairs of 32-sample blocks bi <= bj, chunks of IC_KCHUNK columns); the four waves of a workgroup take every
// fourth 64-column step of the chunk and each computes the whole 32 x 32 block as 2 x 2 tiles of
// v_mfma_i32_16x16x64_i8.  Lane l supplies, as A and as B alike, the 16 bytes at columns 16 * (l >> 4) .. + 15 of row
// l & 15 of its tile: the instruction pairs element t of lane group g of A with element t of group g of B, so any
// assignment of columns to (g, t) that A and B share sums the same products.  The result register q of lane l is
// row 4 * (l >> 4) + q (the A tile's), column l & 15 (the B tile's).
// P[i][j] += sum over the chunk of (X[i][k] - 128) * (X[j][k] - 128), exact: |product| <= 2^14, 2^14 chunk columns.
__global__ __launch_bounds__(IC_WG) void gd_ic_gram_kernel(const uint8_t* __restrict__ X, int64_t m_pad, int n_pad,
                                                           const int2* __restrict__ pairs, long long* __restrict__ P)
{
    const int2 pr = pairs[blockIdx.x];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t k0 = (int64_t)blockIdx.y * IC_KCHUNK;
    const int64_t k1 = k0 + IC_KCHUNK < m_pad ? k0 + IC_KCHUNK : m_pad;
    const size_t col = (size_t)16 * (lane >> 4);
    const uint8_t* __restrict__ a0 = X + (size_t)(pr.x * IC_BLOCK + (lane & 15)) * m_pad + col;
    const uint8_t* __restrict__ a1 = a0 + (size_t)16 * m_pad;
    const uint8_t* __restrict__ b0 = X + (size_t)(pr.y * IC_BLOCK + (lane & 15)) * m_pad + col;
    const uint8_t* __restrict__ b1 = b0 + (size_t)16 * m_pad;
    ic_v4i acc00 = {0, 0, 0, 0}, acc01 = {0, 0, 0, 0}, acc10 = {0, 0, 0, 0}, acc11 = {0, 0, 0, 0};
    const ic_v4i bias = {(int)0x80808080, (int)0x80808080, (int)0x80808080, (int)0x80808080};
    for (int64_t k = k0 + (int64_t)wave * IC_KSTEP; k < k1; k += 4 * IC_KSTEP) {
        const ic_v4i fa0 = *reinterpret_cast<const ic_v4i*>(a0 + k) ^ bias;      // x - 128 as a signed byte
        const ic_v4i fa1 = *reinterpret_cast<const ic_v4i*>(a1 + k) ^ bias;
        const ic_v4i fb0 = *reinterpret_cast<const ic_v4i*>(b0 + k) ^ bias;
        const ic_v4i fb1 = *reinterpret_cast<const ic_v4i*>(b1 + k) ^ bias;
        acc00 = __builtin_amdgcn_mfma_i32_16x16x64_i8(fa0, fb0, acc00, 0, 0, 0);
        acc01 = __builtin_amdgcn_mfma_i32_16x16x64_i8(fa0, fb1, acc01, 0, 0, 0);
        acc10 = __builtin_amdgcn_mfma_i32_16x16x64_i8(fa1, fb0, acc10, 0, 0, 0);
        acc11 = __builtin_amdgcn_mfma_i32_16x16x64_i8(fa1, fb1, acc11, 0, 0, 0);
    }
    // the flush: 32-bit sums of one chunk into the 64-bit matrix
    const int ri = pr.x * IC_BLOCK + 4 * (lane >> 4), cj = pr.y * IC_BLOCK + (lane & 15);
    unsigned long long* __restrict__ Pu = reinterpret_cast<unsigned long long*>(P);
    for (int q = 0; q < 4; ++q) {
        atomicAdd(&Pu[(size_t)(ri + q) * n_pad + cj], (unsigned long long)(long long)acc00[q]);
        atomicAdd(&Pu[(size_t)(ri + q) * n_pad + cj + 16], (unsigned long long)(long long)acc01[q]);
        atomicAdd(&Pu[(size_t)(ri + 16 + q) * n_pad + cj], (unsigned long long)(long long)acc10[q]);
        atomicAdd(&Pu[(size_t)(ri + 16 + q) * n_pad + cj + 16], (unsigned long long)(long long)acc11[q]);
    }
}

// G[i][j] = P[i][j] + 128 * (S_i + S_j) - 128^2 * m_pad (the padding columns hold 0, i.e. -128 after the bias); blocks
// below the diagonal were not computed: they are the transposes of those above it.
__global__ __launch_bounds__(IC_WG) void gd_ic_gram_fin_kernel(const long long* __restrict__ P, const long long* __restrict__ sums,
                                                               int n, int n_pad, int64_t m_pad, long long* __restrict__ G)
{
    const int64_t t = (int64_t)blockIdx.x * IC_WG + threadIdx.x;
    if (t >= (int64_t)n * n) return;
    const int i = (int)(t / n), jj = (int)(t % n);
    const bool up = i / IC_BLOCK <= jj / IC_BLOCK;
    const long long p = up ? P[(size_t)i * n_pad + jj] : P[(size_t)jj * n_pad + i];
    G[t] = p + 128 * (sums[i] + sums[jj]) - 16384 * (long long)m_pad;
}

}  // namespace gd
