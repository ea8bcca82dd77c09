// gd_emdepth.hpp -- emdepth.EMDepth (emdepth/emdepth.go:117-206 of the reference) per site of
// a sites x samples depth matrix: the copy-number centres lambda[0..8] of one row, then every cell's copy number
// (Type / adjustCN, :272-304) and its log2 fold change against CN 2 (Log2FC, :250-260).
//
//   gd_emdepth_kernel<T, REGS>   one wavefront owns one row, EM_WAVES rows a workgroup, a grid-stride loop over the rows.
//                                T is the cell type: float (depths as given) or int64_t (the cells gd_depthwed_device
//                                leaves, each narrowed to float32 and, with a scale, multiplied by scale[s] in float32:
//                                one rounding each).
//
// The register / re-read boundary is EM_REG_MAX = 256 samples: REGS = true holds the row in EM_REGS = 4 float32
// registers a lane, loaded once (coalesced: lane l holds samples l, 64 + l, ...); REGS = false (257 .. 4096 samples)
// reads the row again in every pass -- 32 + 1 passes for the median, one per EM pass, one for the calls -- from a row of
// at most 32 KB that stays in the L2.  Nothing is indexed by a runtime value, so nothing lives in scratch, and the kernel
// uses no LDS: every cross-lane step is a butterfly of wave-wide shuffles, after which all 64 lanes hold the same
// value, so the centres, the pass count and every branch on them are wave-uniform.
//
// The median is the exact order statistic: depths map to 32-bit keys that order as the floats do, and the k-th smallest
// key is found bit by bit from the top (32 counting passes).  Duplicates need no care: the k-th key is a value.
//
// The arithmetic on the nine centres is float64 in the reference's order of operations, never contracted into fused
// multiply-adds.  Sums over a bin are taken in lane order, not in sample order: exact whenever the depths are integers
// (times one power of two), within N * 2^-53 relative otherwise.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gd {

constexpr int EM_WAVES = 4;                      // rows of a workgroup
constexpr int EM_REGS = 4;                       // float32 registers of a lane that hold a row
constexpr int EM_REG_MAX = EM_REGS * 64;         // the longest row held in registers
constexpr int EM_MAX_N = 4096;
constexpr int EM_MAX_GRID = 2048;                // workgroups of a launch: eight per CU
constexpr int EM_CENTRES = 9;                    // maxCN + 1
constexpr int EM_MAXITER = 10;
constexpr double EM_EPS = 0.01;

struct EmJob {
    const void* cells;                           // [n_rows][n] float or int64_t
    const float* scale;                          // [n] or nullptr (int64_t cells only)
    int64_t n_rows;
    int32_t n;
    double pw[EM_CENTRES];                       // pow(i / 2, 1.1) of the host's libm; [0] and [2] are not read
    double* lambda;                              // [n_rows][9]; each output may be nullptr
    uint8_t* iters;                              // [n_rows]
    uint8_t* cn;                                 // [n_rows][n]
    float* log2fc;                               // [n_rows][n]
};

__device__ __forceinline__ int em_wave_sum(int v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double em_wave_sum(double v)
{
#pragma clang fp contract(off)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float em_wave_min(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
    return v;
}

__device__ __forceinline__ float em_depth(const float* row, const float*, int s)
{
    const float d = row[s];
    return d == 0.0f ? 0.0f : d;                 // (-0 is 0: one key, one sign of the centres)
}
__device__ __forceinline__ float em_depth(const int64_t* row, const float* scale, int s)
{
#pragma clang fp contract(off)
    float d = (float)row[s];
    if (scale) d = d * scale[s];
    return d == 0.0f ? 0.0f : d;
}

// One row as its wavefront sees it: each(f) calls f(depth, sample) for the samples of this lane.
template <class T, bool REGS>
struct EmRow {
    const T* row;
    const float* scale;
    int n, lane;
    float v[REGS ? EM_REGS : 1];

    __device__ __forceinline__ void load()
    {
        if constexpr (REGS) {
#pragma unroll
            for (int r = 0; r < EM_REGS; ++r) {
                const int s = r * 64 + lane;
                v[r] = s < n ? em_depth(row, scale, s) : 0.0f;
            }
        }
    }
    template <class F>
    __device__ __forceinline__ void each(F&& f) const
    {
        if constexpr (REGS) {
#pragma unroll
            for (int r = 0; r < EM_REGS; ++r) {
                const int s = r * 64 + lane;
                if (s < n) f(v[r], s);
            }
        } else {
            for (int s = lane; s < n; s += 64) f(em_depth(row, scale, s), s);
        }
    }
};

// keys that order as the floats do (all of them, the negative ones too)
__device__ __forceinline__ uint32_t em_key(float f)
{
    const uint32_t b = __float_as_uint(f);
    return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ float em_unkey(uint32_t k) { return __uint_as_float((k >> 31) ? k ^ 0x80000000u : ~k); }

// b[k] of the sorted row
template <class Row>
__device__ __forceinline__ float em_select(const Row& row, int k)
{
    uint32_t prefix = 0;
    for (int bit = 31; bit >= 0; --bit) {
        int c = 0;                               // keys that agree with the prefix above `bit` and have a 0 there
        row.each([&](float d, int) { c += ((em_key(d) ^ prefix) >> bit) == 0 ? 1 : 0; });
        c = em_wave_sum(c);
        if (k >= c) { k -= c; prefix |= 1u << bit; }
    }
    return em_unkey(prefix);
}

// median32 (:18-29): b[N/2] for odd N, (b[N/2] + b[N/2 + 1]) / 2 for even N (the reference's off-by-one, kept)
template <class Row>
__device__ __forceinline__ double em_median(const Row& row)
{
#pragma clang fp contract(off)
    const int n = row.n, k = n / 2;
    const float a = em_select(row, k);
    if (n & 1) return (double)a;
    int le = 0;
    float above = __builtin_inff();
    row.each([&](float d, int) { if (d <= a) ++le; else above = fminf(above, d); });
    le = em_wave_sum(le);
    above = em_wave_min(above);
    const float b = le >= k + 2 ? a : above;     // (n >= 4: b[k + 1] exists)
    return ((double)a + (double)b) / 2;
}

// sort.SearchFloat64s(lambda, d) (:161, :274): THE binary search, i, j = 0, 9; h = (i + j) / 2; lambda[h] >= d ? j = h :
// i = h + 1 -- the centres are not always ascending, and a scan would answer differently then.  Unrolled into its
// decision tree: every index is a constant.  The leaf also hands back lambda[idx] and lambda[idx - 1].
struct EmHit { int idx; double at, below; };

template <int I, int J>
__device__ __forceinline__ EmHit em_search(const double (&l)[EM_CENTRES], double d)
{
    if constexpr (I >= J) {
        return EmHit{I, I < EM_CENTRES ? l[I < EM_CENTRES ? I : 0] : 0.0, I > 0 ? l[I > 0 ? I - 1 : 0] : 0.0};
    } else {
        constexpr int H = (I + J) / 2;
        return l[H] >= d ? em_search<I, H>(l, d) : em_search<H + 1, J>(l, d);
    }
}

// the bin of one depth in a pass (:152-176)
__device__ __forceinline__ int em_bin(const double (&l)[EM_CENTRES], double d)
{
#pragma clang fp contract(off)
    if (d > l[1] && d < l[3]) {
        const double a2 = fabs(d - l[2]);
        if (a2 < fabs(d - l[1]) && a2 < fabs(d - l[3])) return 2;
    }
    const EmHit h = em_search<0, EM_CENTRES>(l, d);
    if (h.idx == 0) return 0;
    if (h.idx == EM_CENTRES) return EM_CENTRES - 1;
    return fabs(d - h.at) < fabs(d - h.below) ? h.idx : h.idx - 1;
}

// pmf (emdepth/stats.go:14-23); the reference's table of the first 1000 lgamma values holds what Lgamma returns.
// Out of line on purpose: inlined, the log / lgamma / exp of two Poisson terms per cell of a row's four registers made
// the kernel 12 000 instructions and 234 vector registers (two waves a SIMD); called, it is 3 200 and 114 (four).
__device__ __noinline__ double em_pmf(double k, double mu)
{
#pragma clang fp contract(off)
    const double a = k * log(mu);
    const double b = a - lgamma(k + 1.0);
    return exp(b - mu);
}

template <class T, bool REGS>
__global__ __launch_bounds__(EM_WAVES * 64) void gd_emdepth_kernel(EmJob j)
{
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int n = j.n;
    for (int64_t r = (int64_t)blockIdx.x * EM_WAVES + wave; r < j.n_rows; r += (int64_t)gridDim.x * EM_WAVES) {
        EmRow<T, REGS> row;
        row.row = static_cast<const T*>(j.cells) + (size_t)r * (size_t)n;
        row.scale = j.scale; row.n = n; row.lane = lane;
        row.load();

        const double m = em_median(row);
        double l[EM_CENTRES], last[EM_CENTRES];
        l[0] = EM_EPS * m;
        l[2] = m;
#pragma unroll
        for (int i = 1; i < EM_CENTRES; ++i)
            if (i != 2) l[i] = m * j.pw[i];
        last[0] = l[0];                          // lambda[0] never moves: `last` is what a pass classifies against

        double sumd = 100, maxd = 100;
        int iter = 0;
        for (; iter < EM_MAXITER && sumd > EM_EPS && maxd > 0.5; ++iter) {
#pragma unroll
            for (int i = 1; i < EM_CENTRES; ++i) last[i] = l[i];
            // step 1 + the one bin the update usually needs
            double s2 = 0;
            int c2 = 0;
            row.each([&](float df, int) {
                const double d = (double)df;
                if (em_bin(last, d) == 2) { s2 += d; ++c2; }
            });
            s2 = em_wave_sum(s2);
            c2 = em_wave_sum(c2);
            // step 2 (:180-192)
            l[2] = c2 ? s2 / (double)c2 : 0.0;
            if (l[2] == 0.0) {
                // rare: the bins 1 .. 7 of the same classification
                double bs[8];
                int bc[8];
#pragma unroll
                for (int i = 1; i < 8; ++i) { bs[i] = 0; bc[i] = 0; }
                row.each([&](float df, int) {
                    const double d = (double)df;
                    const int b = em_bin(last, d);
#pragma unroll
                    for (int i = 1; i < 8; ++i) { bs[i] += b == i ? d : 0.0; bc[i] += b == i ? 1 : 0; }
                });
                const double fn = (double)n;
#pragma unroll
                for (int i = 1; i < 8; ++i) {
                    const double sum = em_wave_sum(bs[i]);
                    const int cnt = em_wave_sum(bc[i]);
                    const double pdepth = (double)cnt / fn;
                    if (l[i] < EM_EPS) l[i] = EM_EPS;
                    const double mean = cnt ? sum / (double)cnt : 0.0;
                    const double t = mean * (2.0 / (double)i);
                    l[2] += t * pdepth;
                }
            }
            // step 3 (:194-202)
#pragma unroll
            for (int i = 1; i < EM_CENTRES; ++i) l[i] = l[2] * ((double)i / 2.0);
            const double span = l[2] - l[1];
            l[1] -= span / 1.5;
            l[3] += span / 1.5;
            sumd = 0; maxd = 0;
#pragma unroll
            for (int i = 0; i < EM_CENTRES; ++i) {
                const double d = fabs(l[i] - last[i]);
                sumd += d;
                if (d > maxd) maxd = d;
            }
        }

        if (lane == 0) {
            if (j.lambda) {
#pragma unroll
                for (int i = 0; i < EM_CENTRES; ++i) j.lambda[(size_t)r * EM_CENTRES + i] = l[i];
            }
            if (j.iters) j.iters[r] = (uint8_t)iter;
        }
        if (!j.cn && !j.log2fc) continue;
        // Type + adjustCN (:272-304), Log2FC (:256)
        uint8_t* cn_row = j.cn ? j.cn + (size_t)r * (size_t)n : nullptr;
        float* fc_row = j.log2fc ? j.log2fc + (size_t)r * (size_t)n : nullptr;
        row.each([&](float df, int s) {
            const double d = (double)df;
            if (cn_row) {
                const EmHit h = em_search<0, EM_CENTRES>(l, d);
                int cn;
                double mu = h.at;
                if (h.idx == 0) cn = 0;
                else if (h.idx == EM_CENTRES) cn = EM_CENTRES;       // 9, as the code has it (its unit test expects 8)
                else if (fabs(d - h.at) < fabs(d - h.below)) cn = h.idx;
                else { cn = h.idx - 1; mu = h.below; }
                if (cn != 2 && cn < EM_CENTRES) {
                    const double k = trunc(0.5 + d);
                    const double o = em_pmf(k, mu), o2 = em_pmf(k, l[2]);
                    if (o * 0.9 < o2) cn = 2;
                }
                cn_row[s] = (uint8_t)cn;
            }
            if (fc_row) fc_row[s] = (float)log2(d / l[2]);
        });
    }
}

}  // namespace gd
