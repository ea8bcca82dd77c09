// gd_perbase_runs.hpp -- the per-base vector of a region as runs of equal value: count, scan, emit.
//
// The value of a position is its depth, or with cut points the number of cuts <= its depth (its bin).  A position starts a
// run when it is the region's first or its value differs from its left neighbour's.  The region is cut into chunks of
// PB_CHUNK consecutive positions on a grid whose origin is the 16-byte boundary at or below the region's first element, so a
// lane's PB_PER_LANE consecutive positions are four aligned 16-byte loads; a group of four that the region covers only in
// part (the head and the tail) is loaded element by element.
//
//   gd_pb_count_kernel<CUTS>  a workgroup per chunk: the run starts of the chunk, counted (a ballot and a population count
//                             per position slot and wave, the four wave totals added through LDS) -> chunk_cnt[chunk]
//   gd_pb_scan_kernel         one workgroup: exclusive scan of the chunk counts, 4096 a round with a carry; base[n_chunks]
//                             is the number of runs
//   gd_pb_emit_kernel<CUTS>   the count pass's predicate again: a run start's rank in its chunk (lanes below it in the wave
//                             by mbcnt of the same ballots, waves below it through LDS) places it in an LDS image of the
//                             chunk's runs, which the workgroup then stores contiguously at base[chunk]; every store index
//                             is checked against the arrays' capacity
//
// The left neighbour of a lane's first position is the last value of the lane below it (one shuffle); lane 0 of a wave loads
// the one element in front of the wave's positions.  No workgroup waits for another and nothing is atomic: the same bytes
// from call to call.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gd {

constexpr uint32_t PB_WG = 256;                          // lanes of a workgroup
constexpr uint32_t PB_PER_LANE = 16;                     // consecutive positions of a lane
constexpr uint32_t PB_CHUNK = PB_WG * PB_PER_LANE;       // positions of a chunk
constexpr uint32_t PB_SCAN_ROUND = PB_WG * 16;           // chunk counts the scan takes per round
constexpr int PB_MAX_CUTS = 32;                          // = GD_PERBASE_MAX_CUTS

struct PbJob {
    const int32_t* d;              // the contig's per-base vector, indexed by position
    int64_t start, end;            // the region
    int64_t g0;                    // origin of the chunk grid: start minus the elements d + start lies past a 16-byte boundary
    uint32_t* chunk_cnt;           // [n_chunks]
    uint32_t* chunk_base;          // [n_chunks + 1]
    uint32_t n_chunks;
    int32_t n_cuts;
    uint32_t* run_start;           // [cap]
    int32_t* run_value;            // [cap]
    uint64_t cap;
    int32_t cuts[PB_MAX_CUTS];     // strictly increasing; [0, n_cuts) are read
};

// The values of this lane's positions (0 outside the region) and, as bit i of the result, whether position p0 + i starts a run.
template <bool CUTS>
__device__ __forceinline__ uint32_t pb_lane_starts(const PbJob& j, int64_t p0, int32_t (&v)[PB_PER_LANE])
{
#pragma unroll
    for (uint32_t q = 0; q < PB_PER_LANE / 4; ++q) {
        const int64_t p = p0 + 4 * q;
        if (p >= j.start && p + 4 <= j.end) {
            const int4 x = *reinterpret_cast<const int4*>(j.d + p);
            v[4 * q] = x.x; v[4 * q + 1] = x.y; v[4 * q + 2] = x.z; v[4 * q + 3] = x.w;
        } else {
#pragma unroll
            for (uint32_t e = 0; e < 4; ++e) v[4 * q + e] = (p + e >= j.start && p + e < j.end) ? j.d[p + e] : 0;
        }
    }
    // lane 0 of a wave: the element in front of the wave's positions, where the region holds it
    int32_t left = 0;
    const bool own_left = (threadIdx.x & 63u) == 0u && p0 > j.start && p0 <= j.end;
    if (own_left) left = j.d[p0 - 1];
    if (CUTS) {
        int32_t b[PB_PER_LANE], bl = 0;
#pragma unroll
        for (uint32_t i = 0; i < PB_PER_LANE; ++i) b[i] = 0;
        for (int32_t k = 0; k < j.n_cuts; ++k) {
            const int32_t cut = j.cuts[k];
#pragma unroll
            for (uint32_t i = 0; i < PB_PER_LANE; ++i) b[i] += v[i] >= cut ? 1 : 0;
            bl += left >= cut ? 1 : 0;
        }
#pragma unroll
        for (uint32_t i = 0; i < PB_PER_LANE; ++i) v[i] = b[i];
        left = bl;
    }
    const int32_t below = __shfl_up(v[PB_PER_LANE - 1], 1, 64);
    if (!own_left) left = below;
    uint32_t m = 0;
#pragma unroll
    for (uint32_t i = 0; i < PB_PER_LANE; ++i) {
        const int64_t p = p0 + i;
        const bool in = p >= j.start && p < j.end;
        if (in && (p == j.start || v[i] != (i ? v[i - 1] : left))) m |= 1u << i;
    }
    return m;
}

template <bool CUTS>
__global__ __launch_bounds__(256) void gd_pb_count_kernel(PbJob j)
{
    __shared__ uint32_t s_cnt[PB_WG / 64];
    const int64_t p0 = j.g0 + (int64_t)blockIdx.x * PB_CHUNK + (int64_t)threadIdx.x * PB_PER_LANE;
    int32_t v[PB_PER_LANE];
    const uint32_t m = pb_lane_starts<CUTS>(j, p0, v);
    uint32_t n = 0;
#pragma unroll
    for (uint32_t i = 0; i < PB_PER_LANE; ++i) n += (uint32_t)__popcll(__ballot((m >> i) & 1u));
    if ((threadIdx.x & 63u) == 0u) s_cnt[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0 && blockIdx.x < j.n_chunks) j.chunk_cnt[blockIdx.x] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
}

__global__ __launch_bounds__(256) void gd_pb_scan_kernel(PbJob j)
{
    __shared__ uint32_t s_wave[PB_WG / 64];
    __shared__ uint32_t s_carry;
    if (threadIdx.x == 0) s_carry = 0;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint32_t base = 0; base < j.n_chunks; base += PB_SCAN_ROUND) {
        const uint32_t t0 = base + threadIdx.x * 16u;
        uint32_t x[16], sum = 0;
#pragma unroll
        for (uint32_t i = 0; i < 16; ++i) { x[i] = t0 + i < j.n_chunks ? j.chunk_cnt[t0 + i] : 0u; sum += x[i]; }
        uint32_t inc = sum;                                    // inclusive scan of the lanes' sums over the wave
#pragma unroll
        for (uint32_t d = 1; d < 64; d <<= 1) {
            const uint32_t up = __shfl_up(inc, d, 64);
            if (lane >= d) inc += up;
        }
        if (lane == 63u) s_wave[wave] = inc;
        __syncthreads();
        uint32_t at = s_carry + inc - sum;
        for (uint32_t w = 0; w < wave; ++w) at += s_wave[w];
#pragma unroll
        for (uint32_t i = 0; i < 16; ++i) {
            if (t0 + i < j.n_chunks) j.chunk_base[t0 + i] = at;
            at += x[i];
        }
        __syncthreads();
        if (threadIdx.x == PB_WG - 1) s_carry = at;
        __syncthreads();
    }
    if (threadIdx.x == 0) j.chunk_base[j.n_chunks] = s_carry;
}

template <bool CUTS>
__global__ __launch_bounds__(256) void gd_pb_emit_kernel(PbJob j)
{
    __shared__ uint2 s_run[PB_CHUNK];                          // the chunk's runs {start, value}, in position order
    __shared__ uint32_t s_cnt[PB_WG / 64];
    const int64_t p0 = j.g0 + (int64_t)blockIdx.x * PB_CHUNK + (int64_t)threadIdx.x * PB_PER_LANE;
    int32_t v[PB_PER_LANE];
    const uint32_t m = pb_lane_starts<CUTS>(j, p0, v);
    uint32_t n = 0, r = 0;                                     // run starts of the wave; of the lanes below this one
#pragma unroll
    for (uint32_t i = 0; i < PB_PER_LANE; ++i) {
        const uint64_t b = __ballot((m >> i) & 1u);
        n += (uint32_t)__popcll(b);
        r = __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, r));
    }
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0u) s_cnt[wave] = n;
    __syncthreads();
    uint32_t total = 0;
#pragma unroll
    for (uint32_t w = 0; w < PB_WG / 64; ++w) {
        if (w < wave) r += s_cnt[w];
        total += s_cnt[w];
    }
#pragma unroll
    for (uint32_t i = 0; i < PB_PER_LANE; ++i)
        if ((m >> i) & 1u) {
            if (r < PB_CHUNK) s_run[r] = make_uint2((uint32_t)(p0 + i), (uint32_t)v[i]);
            ++r;
        }
    __syncthreads();
    if (blockIdx.x >= j.n_chunks) return;
    const uint64_t base = j.chunk_base[blockIdx.x];
    if (total > PB_CHUNK) total = PB_CHUNK;
    for (uint32_t k = threadIdx.x; k < total; k += PB_WG) {
        const uint64_t at = base + k;
        if (at < j.cap) {
            const uint2 x = s_run[k];
            j.run_start[at] = x.x;
            j.run_value[at] = (int32_t)x.y;
        }
    }
}

}  // namespace gd
