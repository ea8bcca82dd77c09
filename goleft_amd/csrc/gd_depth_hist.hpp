// gd_depth_hist.hpp -- the per-base vector reduced along the depth axis: a histogram with sum,
// minimum and maximum over a list of regions, and per-region counts of the depth bins of section 3.21.
//
// Both kernels walk one host-built table: an entry per (region, chunk of DH_CHUNK consecutive positions), the chunks on a
// grid whose origin is the 16-byte boundary at or below the region's first element (gd_perbase_runs.hpp's grid), so a lane's
// DH_PER_LANE consecutive positions are four aligned 16-byte loads; a group of four that the region covers only in part (its
// head and its tail) is loaded element by element under a bounds test.  dh_lane_load feeds both kernels: the values and a
// mask of the positions the region holds.  A position outside the region is in no count -- it is not a depth of 0.
//
//   gd_dh_hist_kernel         a persistent grid, every workgroup striding over the table.  Bins below DH_LDS_BINS are counted
//                             in a uint32 LDS table, the bins above go straight to the call's uint64 table by atomic; at the
//                             end a workgroup adds its non-zero LDS bins with one 64-bit atomic each.  Depth is piecewise
//                             constant, so a lane merges equal neighbours before it adds (an LDS add per lane-run), and a wave
//                             whose 1024 positions all agree adds once.  Sum, minimum and maximum: per lane, per wave, then
//                             one atomic each per workgroup.
//   gd_dh_region_bins_kernel  a workgroup per table entry: per cut the lane's count of positions at or above it, added over
//                             the wave, the four waves meet in LDS, and lane b turns them into bin b's count by a difference
//                             and adds it to the region's row with one 64-bit atomic when it is not 0.
//
// Everything is an integer count: the order of the atomics does not change a result.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gd {

constexpr uint32_t DH_WG = 256;                          // lanes of a workgroup
constexpr uint32_t DH_PER_LANE = 16;                     // consecutive positions of a lane
constexpr uint32_t DH_CHUNK = DH_WG * DH_PER_LANE;       // positions of a table entry
constexpr uint32_t DH_LDS_BINS = 8192;                   // bins counted in LDS: 32 KB a workgroup, four workgroups a CU
constexpr uint32_t DH_WG_PER_CU = 4;
constexpr uint32_t DH_MAX_CHUNKS_PER_WG = 1u << 18;      // 2^30 positions: a uint32 LDS counter cannot overflow
constexpr int DH_MAX_CUTS = 32;                          // = GD_PERBASE_MAX_CUTS

struct DhRegion {
    int64_t base_off;              // the contig's per-base vector, indexed by position, starts at DhJob::perbase + base_off
    int64_t start, end;            // the region, not empty
    int64_t g0;                    // origin of the chunk grid: start minus the elements d + start lies past a 16-byte boundary
    uint32_t chunk_off;            // the table index of the region's first chunk
    uint32_t row;                  // gd_region_bins: the region's row of counts
};

struct DhStats {                   // gd_depth_hist's scalars; the call starts them at {0, INT32_MAX, INT32_MIN}
    unsigned long long sum;
    int32_t min, max;
};

struct DhJob {
    const int32_t* perbase;        // the context's kept vector (a kernel argument: the loads are global loads)
    const DhRegion* tab;
    const uint32_t* chunk_region;  // [n_chunks]: index into tab
    uint32_t n_chunks;
    uint32_t top;                  // histogram: n_bins - 1, the bin of every depth at or above it
    unsigned long long* out;       // histogram: [n_bins]; region bins: [rows][n_cuts + 1]; zeroed by the call
    DhStats* stats;                // histogram only
    int32_t n_cuts;                // region bins only
    int32_t cuts[DH_MAX_CUTS];     // strictly increasing, from 1; [0, n_cuts) are read
};

// The values of this lane's positions p0 .. p0 + 15 of the contig's vector d and, as bit i of the result, whether the region holds p0 + i.
__device__ __forceinline__ uint32_t dh_lane_load(const int32_t* __restrict__ d, const DhRegion& t, int64_t p0, int32_t (&v)[DH_PER_LANE])
{
    uint32_t m = 0;
#pragma unroll
    for (uint32_t q = 0; q < DH_PER_LANE / 4; ++q) {
        const int64_t p = p0 + 4 * q;
        if (p >= t.start && p + 4 <= t.end) {
            const int4 x = *reinterpret_cast<const int4*>(d + p);
            v[4 * q] = x.x; v[4 * q + 1] = x.y; v[4 * q + 2] = x.z; v[4 * q + 3] = x.w;
            m |= 0xfu << (4 * q);
        } else {
#pragma unroll
            for (uint32_t e = 0; e < 4; ++e) {
                const bool in = p + e >= t.start && p + e < t.end;
                v[4 * q + e] = in ? d[p + e] : 0;
                m |= (in ? 1u : 0u) << (4 * q + e);
            }
        }
    }
    return m;
}

// n positions of bin k
__device__ __forceinline__ void dh_add(const DhJob& j, uint32_t* s_bin, uint32_t k, uint32_t n)
{
    if (k < DH_LDS_BINS) atomicAdd(&s_bin[k], n);
    else atomicAdd(&j.out[k], (unsigned long long)n);
}

__global__ __launch_bounds__(256) void gd_dh_hist_kernel(DhJob j)
{
    __shared__ uint32_t s_bin[DH_LDS_BINS];
    __shared__ long long s_sum[DH_WG / 64];
    __shared__ int32_t s_min[DH_WG / 64], s_max[DH_WG / 64];
    const uint32_t n_lds = j.top + 1u < DH_LDS_BINS ? j.top + 1u : DH_LDS_BINS;      // every bin is <= top
    for (uint32_t k = threadIdx.x; k < n_lds; k += DH_WG) s_bin[k] = 0;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    long long sum = 0;
    int32_t lo = INT32_MAX, hi = INT32_MIN;
    for (uint32_t ch = blockIdx.x; ch < j.n_chunks; ch += gridDim.x) {
        const DhRegion t = j.tab[j.chunk_region[ch]];
        const int64_t p0 = t.g0 + (int64_t)(ch - t.chunk_off) * DH_CHUNK + (int64_t)threadIdx.x * DH_PER_LANE;
        int32_t v[DH_PER_LANE];
        const uint32_t m = dh_lane_load(j.perbase + t.base_off, t, p0, v);
        uint32_t b[DH_PER_LANE];
        bool one = m == 0xffffu;                                   // all 16 held, and of one bin
#pragma unroll
        for (uint32_t i = 0; i < DH_PER_LANE; ++i) {
            if ((m >> i) & 1u) {
                sum += v[i];
                lo = v[i] < lo ? v[i] : lo;
                hi = v[i] > hi ? v[i] : hi;
            }
            const uint32_t d = v[i] < 0 ? 0u : (uint32_t)v[i];     // (a depth is never negative: no index below the table)
            b[i] = d < j.top ? d : j.top;
            one = one && b[i] == b[0];
        }
        const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)b[0]);
        if (__ballot(one && b[0] == first) == ~0ull) {             // the wave's 1024 positions agree: one add
            if (lane == 0u) dh_add(j, s_bin, first, 64u * DH_PER_LANE);
            continue;
        }
        // a lane-run ends at position i when the region does not hold i + 1 or its bin differs
        uint32_t run = 0;
#pragma unroll
        for (uint32_t i = 0; i < DH_PER_LANE; ++i) {
            const bool in = (m >> i) & 1u;
            run += in ? 1u : 0u;
            const bool last = i + 1 == DH_PER_LANE || !((m >> (i + 1)) & 1u) || b[(i + 1) % DH_PER_LANE] != b[i];
            if (in && last) {
                dh_add(j, s_bin, b[i], run);
                run = 0;
            }
        }
    }
    // sum, minimum, maximum: over the wave, the waves through LDS, one atomic each
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        sum += __shfl_down(sum, o, 64);
        const int32_t l2 = __shfl_down(lo, o, 64), h2 = __shfl_down(hi, o, 64);
        lo = l2 < lo ? l2 : lo;
        hi = h2 > hi ? h2 : hi;
    }
    if (lane == 0u) { s_sum[threadIdx.x >> 6] = sum; s_min[threadIdx.x >> 6] = lo; s_max[threadIdx.x >> 6] = hi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (uint32_t w = 1; w < DH_WG / 64; ++w) {
            sum += s_sum[w];
            lo = s_min[w] < lo ? s_min[w] : lo;
            hi = s_max[w] > hi ? s_max[w] : hi;
        }
        if (lo <= hi) {                                            // the workgroup saw a position
            atomicAdd(&j.stats->sum, (unsigned long long)sum);
            atomicMin(&j.stats->min, lo);
            atomicMax(&j.stats->max, hi);
        }
    }
    for (uint32_t k = threadIdx.x; k < n_lds; k += DH_WG) {
        const uint32_t n = s_bin[k];
        if (n) atomicAdd(&j.out[k], (unsigned long long)n);
    }
}

__global__ __launch_bounds__(256) void gd_dh_region_bins_kernel(DhJob j)
{
    __shared__ uint32_t s_ge[DH_WG / 64][DH_MAX_CUTS];             // per wave and cut: positions at or above the cut
    const uint32_t ch = blockIdx.x;
    if (ch >= j.n_chunks) return;
    const DhRegion t = j.tab[j.chunk_region[ch]];
    const int64_t c0 = t.g0 + (int64_t)(ch - t.chunk_off) * DH_CHUNK;
    int32_t v[DH_PER_LANE];
    const uint32_t m = dh_lane_load(j.perbase + t.base_off, t, c0 + (int64_t)threadIdx.x * DH_PER_LANE, v);
#pragma unroll
    for (uint32_t i = 0; i < DH_PER_LANE; ++i) v[i] = (m >> i) & 1u ? v[i] : INT32_MIN;      // below every cut
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (int32_t k = 0; k < j.n_cuts; ++k) {
        const int32_t cut = j.cuts[k];
        uint32_t n = 0;
#pragma unroll
        for (uint32_t i = 0; i < DH_PER_LANE; ++i) n += v[i] >= cut ? 1u : 0u;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) n += __shfl_down(n, o, 64);
        if (lane == 0u) s_ge[wave][k] = n;
    }
    __syncthreads();
    // bin b: the positions at or above cut b - 1 (all the chunk's, for b = 0) that are not at or above cut b
    const int32_t b = (int32_t)threadIdx.x;
    if (b <= j.n_cuts) {
        const int64_t p_lo = c0 > t.start ? c0 : t.start, p_hi = c0 + DH_CHUNK < t.end ? c0 + DH_CHUNK : t.end;
        uint32_t above = (uint32_t)(p_hi - p_lo), at = 0;
        if (b > 0) above = s_ge[0][b - 1] + s_ge[1][b - 1] + s_ge[2][b - 1] + s_ge[3][b - 1];
        if (b < j.n_cuts) at = s_ge[0][b] + s_ge[1][b] + s_ge[2][b] + s_ge[3][b];
        if (above != at) atomicAdd(&j.out[(size_t)t.row * (size_t)(j.n_cuts + 1) + (size_t)b], (unsigned long long)(above - at));
    }
}

}  // namespace gd
