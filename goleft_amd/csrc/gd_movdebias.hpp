// gd_movdebias.hpp -- dcnv's GeneralDebiaser (dcnv/debiaser/debiaser.go:98-123 of the reference; the debiaser dcnv's main
// runs, Window = 9) on a row-major [rows][samples] float32 matrix: every sample is divided by a
// moving median over the rows in covariate order.  The matrix is not permuted: the host hands over order[R], the rows in
// ascending covariate order (ties by row), so the reference's Sort and Unsort cost nothing.
//
// With c[i] the sample's cell of row order[i], W the odd window and mid = (W - 1) / 2 + 1, the Go loop pushes the sequence
// P[t] = c[t] (t < mid), c[t + mid] (t >= mid), R - mid values in all, and divides row i by the median of P[lo .. hi):
// hi = mid (i < mid), min(i + 1, max(mid, R - mid)) otherwise; lo = max(0, hi - W).  Every window is a closed-form range
// of a fixed sequence, so a segment of sorted positions can start anywhere: it loads the at most W pushed rows before it.
//
//   gd_movdebias_kernel<CAP>   a workgroup is ONE wave and owns a (64-column tile, segment of sorted positions) pair:
//                              blockIdx.y the tile, blockIdx.x the segment.  Lanes run along samples as in
//                              gd_chunkdebias.hpp (lane l owns column 64 y + l; the load of a permuted row's slice is 64
//                              consecutive cells, the row index wave-uniform).  The window is an LDS ring [slot][lane] of
//                              keys (the cells' bit patterns, -0.0 as 0: non-negative floats order as their bits do) beside
//                              a byte [slot][lane] with each key's RANK in the window, ties ordered by age.  A push walks
//                              the ring once: the leaving key lowers the ranks above it, the arriving key raises the
//                              ranks above it and counts its own; the keys whose rank is (m - 1) / 2 and m / 2 (m values
//                              in the window; one key when m = W) are picked up on the way -- one loop for a window that
//                              still grows (nothing leaves, two picks), one for a full one (one pick).  O(W) LDS words a
//                              step, exact, no float arithmetic: the ranks do not depend on where the segment began.
//                              MD_BATCH steps load their rows first (the pushed row and the row to divide, both through
//                              order[]), then run.  The median is (double)key for a full window, the float64 mean of the
//                              two middle keys for a partial one; out = (float)((double)c / max(median, 1.0)).
//
// Three instances, by the LDS a window needs (5 bytes a slot and lane): CAP 15 (4 800 bytes), 63 (20 160), 255 (81 600; two
// workgroups a CU).  No scratch (the rows in flight are unrolled arrays), no global atomics, nothing global between
// workgroups.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gd {

constexpr int MD_COLS = 64;                      // columns of a workgroup: one per lane
constexpr int MD_BATCH = 8;                      // steps whose rows are loaded together
#define MD_UNROLL 8                              /* slots of the ring a push has in flight */
constexpr int MD_MAX_W = 255;
constexpr int MD_MAX_N = 4096;
constexpr int MD_CAP_SMALL = 15, MD_CAP_MID = 63, MD_CAP_BIG = 255;
constexpr int64_t MD_SEG_SMALL = 256, MD_SEG_BIG = 1024;     // sorted positions of a segment: W <= MD_CAP_MID, above

struct MdJob {
    const uint32_t* cells;                       // [n_rows][n] float32, as bits
    int64_t n_rows;
    int32_t n;
    int32_t window;                              // W, odd
    int64_t segment;                             // sorted positions a workgroup owns
    const uint32_t* order;                       // [n_rows] rows in ascending covariate order
    float* out;                                  // [n_rows][n]
    double* med;                                 // [n_rows][n] the divisors before the max, or null
};

__device__ __forceinline__ uint32_t md_key(uint32_t bits)
{
    return (bits << 1) ? bits : 0u;              // (-0 is 0; the caller refused every other negative)
}

template <int CAP>
__global__ __launch_bounds__(MD_COLS) void gd_movdebias_kernel(MdJob j)
{
#pragma clang fp contract(off)
    __shared__ uint32_t ring[CAP * MD_COLS];
    __shared__ uint8_t rank[CAP * MD_COLS];
    const int lane = threadIdx.x;
    const int n = j.n;
    const int own = (int)blockIdx.y * MD_COLS + lane;
    const bool live = own < n;
    const size_t col = (size_t)(live ? own : n - 1);           // (a dead lane reads the last column and stores nothing)
    const int W = j.window;
    const int64_t R = j.n_rows;
    const int64_t mid = (W - 1) / 2 + 1;
    const int64_t pushes = R - mid > mid ? R - mid : mid;      // |P|
    const int64_t a = (int64_t)blockIdx.x * j.segment;
    const int64_t b = a + j.segment < R ? a + j.segment : R;
    if (a >= b) return;

    int m = 0;                                   // values in the window
    int slot = 0;                                // where the next one goes: the oldest, once the window is full
    uint32_t k1 = 0, k2 = 0;                     // the keys of rank (m - 1) / 2 and m / 2

    // the row whose cell is P[t]
    const auto pushed_row = [&](int64_t t) -> size_t {
        return (size_t)__builtin_amdgcn_readfirstlane(j.order[t < mid ? t : t + mid]);
    };
    // One value enters the window; once the window is full the oldest leaves it.  Two loops, neither with a branch in its
    // body, so that the LDS reads of MD_UNROLL slots are in flight together (a workgroup is one wave and a CU holds two of
    // the largest: nothing else hides their latency, and the walk is bound by its vector instructions).  `above` counts the
    // keys y stands below; y is the youngest, so it stands above every key that equals it.
    const auto push = [&](uint32_t y) {
        uint32_t above = 0;
        if (m < W) {                             // the window grows by one: slots 0 .. m - 1 stay, y goes to slot m
            const uint32_t r1 = (uint32_t)m / 2u, r2 = (uint32_t)(m + 1) / 2u;     // (m + 1 values: ranks m / 2 and (m + 1) / 2)
#pragma unroll MD_UNROLL
            for (int s = 0; s < m; ++s) {
                const uint32_t e = ring[s * MD_COLS + lane];
                const uint32_t up = y < e ? 1u : 0u;
                const uint32_t r = rank[s * MD_COLS + lane] + up;
                above += up;
                rank[s * MD_COLS + lane] = (uint8_t)r;
                if (r == r1) k1 = e;
                if (r == r2) k2 = e;
            }
            const uint32_t ry = (uint32_t)m - above;
            ring[m * MD_COLS + lane] = y;
            rank[m * MD_COLS + lane] = (uint8_t)ry;
            if (ry == r1) k1 = y;
            if (ry == r2) k2 = y;
            ++m;
            slot = m == W ? 0 : m;
        } else {                                 // the window slides: the key of `slot`, the oldest, leaves
            const uint32_t r1 = (uint32_t)(W - 1) / 2u;
            const uint32_t x = ring[slot * MD_COLS + lane];
            // the leaving key's slot goes through the loop like the others, with a rank no pick can meet (r1 <= 127)
            rank[slot * MD_COLS + lane] = 255;
#pragma unroll MD_UNROLL
            for (int s = 0; s < W; ++s) {
                const uint32_t e = ring[s * MD_COLS + lane];
                const uint32_t up = y < e ? 1u : 0u;
                // x is older than e: it stood below an equal key
                const uint32_t r = rank[s * MD_COLS + lane] - (x <= e ? 1u : 0u) + up;
                above += up;
                rank[s * MD_COLS + lane] = (uint8_t)r;
                if (r == r1) k1 = e;
            }
            const uint32_t ry = (uint32_t)(W - 1) - (above - (y < x ? 1u : 0u));
            ring[slot * MD_COLS + lane] = y;
            rank[slot * MD_COLS + lane] = (uint8_t)ry;
            if (ry == r1) k1 = y;
            k2 = k1;
            slot = slot + 1 == W ? 0 : slot + 1;
        }
    };

    // the window of the segment's first row: P[lo0 .. hi0)
    const int64_t hi0 = a < mid ? mid : (a + 1 < pushes ? a + 1 : pushes);
    const int64_t lo0 = hi0 > W ? hi0 - W : 0;
    for (int64_t t0 = lo0; t0 < hi0; t0 += MD_BATCH) {
        uint32_t v[MD_BATCH];
#pragma unroll
        for (int u = 0; u < MD_BATCH; ++u)
            if (t0 + u < hi0) v[u] = j.cells[pushed_row(t0 + u) * (size_t)n + col];
#pragma unroll
        for (int u = 0; u < MD_BATCH; ++u)
            if (t0 + u < hi0) push(md_key(v[u]));
    }

    for (int64_t i0 = a; i0 < b; i0 += MD_BATCH) {
        uint32_t cv[MD_BATCH], pv[MD_BATCH];
        size_t at[MD_BATCH];
#pragma unroll
        for (int u = 0; u < MD_BATCH; ++u) {
            const int64_t i = i0 + u;
            if (i < b) {
                at[u] = (size_t)__builtin_amdgcn_readfirstlane(j.order[i]) * (size_t)n + col;
                cv[u] = j.cells[at[u]];
                // row i pushes P[i] when its window ends one later than row i - 1's (the first row's is loaded already)
                if (i > a && i >= mid && i < pushes) pv[u] = j.cells[pushed_row(i) * (size_t)n + col];
            }
        }
#pragma unroll
        for (int u = 0; u < MD_BATCH; ++u) {
            const int64_t i = i0 + u;
            if (i < b) {
                if (i > a && i >= mid && i < pushes) push(md_key(pv[u]));
                double median = (double)__uint_as_float(k1);
                if (k1 != k2) median = (median + (double)__uint_as_float(k2)) / 2.0;
                const double q = (double)__uint_as_float(cv[u]) / (median > 1.0 ? median : 1.0);
                if (live) {
                    j.out[at[u]] = (float)q;
                    if (j.med) j.med[at[u]] = median;
                }
            }
        }
    }
}

}  // namespace gd
