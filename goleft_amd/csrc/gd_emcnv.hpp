// gd_emcnv.hpp -- emdepth.Cache (emdepth/emdepth.go:216-398 of the reference): the aberrant
// cells of a sites x samples depth matrix joined into CNV calls per sample, on what gd_emdepth_kernel leaves in HBM.
//
// The reference walks the sites in order (Cache.Add, then Clear(nil)); here the walk is restated in a form without a
// loop-carried list (section 3.11, "the parallel form"):
//
//   member[r][s]  the cell's state (U: log2fc >= 0.40, D: <= -0.80) is U or D and equals the state one row up
//   F[a]          the first row r > a with (start[r] - end[a]) mod 2^32 >= 30000; R when there is none and the final
//                 test (start[R-1] + 100000 - end[a]) holds, R + 1 (never) otherwise
//   s != 0        consecutive members a < b of a column are one CNV iff F[a] > b; it is emitted at F[last member]
//   s == 0        every member is its own list, emitted iff F[a] == a + 1 (the reference deletes key 0 in every Clear
//                 that finds a list)
//   PSize(e)      the columns s != 0 whose latest member a < e has F[a] >= e, plus member[e-1][0]
//
// makecnvs (:376-398) skips members with -0.5 < fc < 0.3.  A member has fc >= 0.4 or fc <= -0.8, so the skip never
// fires, a non-empty list never gives nil, and no carry for a nil is built.
//
// Kernels, per block of rows (gd_emcnv_add*):
//   gd_emcnv_member_kernel<T>   one wavefront a row: states from float64 log2 of the float64 quotient, the row's member
//                               bits (one 64-bit word per 64 samples, by ballot) and their count
//   gd_emcnv_scan_*             exclusive scan of uint32 counts into uint64 offsets (tile sums, top, apply)
//   gd_emcnv_gather_kernel<T>   depth, cn and float32 log2fc of the members into the arena, in (row, sample) order
// and once, in gd_emcnv_finish:
//   gd_emcnv_span_kernel<L>     min and max of the starts over blocks of 64 and of 4096 rows
//   gd_emcnv_gap_kernel         F, one thread a row, stepping over whole blocks that cannot hold a gap row
//   gd_emcnv_chunk_kernel       columns cut into chunks of EMCNV_CHUNK rows, one lane per (chunk, sample): the chunk's
//                               first and last member, the length of its last run, whether the chunk is one run
//   gd_emcnv_carry_kernel       one lane a column over the chunk summaries (R / EMCNV_CHUNK steps without a dependent
//                               load): what each chunk starts from
//   gd_emcnv_emit_kernel<P>     the chunk walk again.  P = 0 counts: PSize per row (ballots), CNVs per emit row and the
//                               emit row's sample bits.  P = 1 scatters: a CNV's slot is its emit row's offset plus the
//                               rank of its sample among that row's bits.
//   gd_emcnv_members_kernel     one wavefront a CNV walks up its column from the last member, 64 rows a step, and copies
//                               from the arena
// Every output position is a scan of counts or a rank among bits: integer atomics only add counts and set bits, so
// two runs give the same bytes.  All lanes of a wave read the same member word of a row: the walk over a chunk costs one
// broadcast load a row.  Nothing is indexed by a runtime register index: no scratch.  LDS: the scans' 2 KB.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gd_emdepth.hpp"

namespace gd {

constexpr int EMCNV_CHUNK = 256;                 // rows of a column chunk
constexpr int EMCNV_WAVES = 4;                   // waves of a workgroup (rows, or (chunk, word) pairs)
constexpr int EMCNV_WG = EMCNV_WAVES * 64;
constexpr int EMCNV_MAX_GRID = 2048;             // workgroups of a launch of the two per-block kernels, which stride over the rows
constexpr int EMCNV_SCAN_TILE = EMCNV_WG * 4;    // elements a scan workgroup takes
constexpr uint32_t EMCNV_GAP = 30000;            // Clear: p.Start - last.End < 30000 keeps the list (:360)
constexpr uint32_t EMCNV_FINAL = 100000;         // Clear(nil): last.Start + 100000 (:353)
constexpr uint32_t EMCNV_NONE = 0xffffffffu;
constexpr uint32_t EMCNV_HALF = 0x80000000u;     // start ^ EMCNV_HALF is start + 2^31 (mod 2^32)
constexpr uint32_t EMCNV_ONE_RUN = 0x80000000u;  // chunk summary: the chunk's members are one run
constexpr double EMCNV_LOWER = -0.80, EMCNV_UPPER = 0.40;        // :224-225
enum : uint8_t { EMCNV_N = 0, EMCNV_U = 1, EMCNV_D = 2, EMCNV_X = 3 };

// Same (:227-247) as a state per cell: U and D are what `non2` keeps when both rows agree
__device__ __forceinline__ uint8_t emcnv_state(float depth, double lambda2)
{
#pragma clang fp contract(off)
    const double fc = log2((double)depth / lambda2);
    if (fc >= EMCNV_UPPER) return EMCNV_U;
    if (fc <= EMCNV_LOWER) return EMCNV_D;
    if (fc > EMCNV_LOWER && fc < EMCNV_UPPER) return EMCNV_N;
    return EMCNV_X;                              // NaN
}

__device__ __forceinline__ uint64_t emcnv_below(int lane) { return (1ull << lane) - 1ull; }

// members of row `r` in front of sample (w, lane)
__device__ __forceinline__ uint32_t emcnv_rank(const uint64_t* bits_row, int w, int lane)
{
    uint32_t k = 0;
    for (int j = 0; j < w; ++j) k += (uint32_t)__popcll(bits_row[j]);
    return k + (uint32_t)__popcll(bits_row[w] & emcnv_below(lane));
}

struct EmcnvBlock {
    const void* cells;                           // [n_rows][n] float or int64_t: the block
    const float* scale;                          // [n] or nullptr
    const double* lambda;                        // [n_rows][9] of the block
    const uint8_t* cn;                           // [n_rows][n] of the block
    const float* log2fc;
    int64_t n_rows;                              // of the block
    int64_t row0;                                // rows before it
    int32_t n, words;
    const uint8_t* carry_in;                     // [n] states of row row0 - 1 (not read when row0 == 0)
    uint8_t* carry_out;                          // [n] states of the block's last row
    uint64_t* mbits;                             // [rows][words], all blocks
    uint32_t* rowcnt;                            // [n_rows] of the block
    const uint64_t* rowoff;                      // [rows]: members in front of a row, all blocks
    float* m_depth; uint8_t* m_cn; float* m_fc;  // the arena
};

template <class T>
__global__ __launch_bounds__(EMCNV_WG) void gd_emcnv_member_kernel(EmcnvBlock j)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int n = j.n;
    for (int64_t r = (int64_t)blockIdx.x * EMCNV_WAVES + wave; r < j.n_rows; r += (int64_t)gridDim.x * EMCNV_WAVES) {
        const T* row = static_cast<const T*>(j.cells) + (size_t)r * (size_t)n;
        const double l2 = j.lambda[(size_t)r * EM_CENTRES + 2];
        const double l2up = r > 0 ? j.lambda[(size_t)(r - 1) * EM_CENTRES + 2] : 0.0;
        uint32_t cnt = 0;
        for (int w = 0; w < j.words; ++w) {
            const int s = w * 64 + lane;
            bool member = false;
            if (s < n) {
                const uint8_t st = emcnv_state(em_depth(row, j.scale, s), l2);
                uint8_t up;
                if (r > 0) up = emcnv_state(em_depth(row - n, j.scale, s), l2up);
                else if (j.row0 == 0) up = st;   // the first Add compares the row with itself (:332-339)
                else up = j.carry_in[s];
                member = (st == EMCNV_U || st == EMCNV_D) && st == up;
                if (r == j.n_rows - 1) j.carry_out[s] = st;
            }
            const uint64_t bits = __ballot(member);
            if (lane == 0) j.mbits[(size_t)(j.row0 + r) * (size_t)j.words + w] = bits;
            cnt += (uint32_t)__popcll(bits);
        }
        if (lane == 0) j.rowcnt[r] = cnt;
    }
}

template <class T>
__global__ __launch_bounds__(EMCNV_WG) void gd_emcnv_gather_kernel(EmcnvBlock j)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int n = j.n;
    for (int64_t r = (int64_t)blockIdx.x * EMCNV_WAVES + wave; r < j.n_rows; r += (int64_t)gridDim.x * EMCNV_WAVES) {
        const T* row = static_cast<const T*>(j.cells) + (size_t)r * (size_t)n;
        const uint64_t* bits_row = j.mbits + (size_t)(j.row0 + r) * (size_t)j.words;
        uint64_t at = j.rowoff[j.row0 + r];
        for (int w = 0; w < j.words; ++w) {
            const uint64_t bits = bits_row[w];
            const int s = w * 64 + lane;
            if ((bits >> lane) & 1ull) {         // (a set bit has s < n)
                const uint64_t i = at + (uint64_t)__popcll(bits & emcnv_below(lane));
                j.m_depth[i] = em_depth(row, j.scale, s);
                j.m_cn[i] = j.cn[(size_t)r * (size_t)n + s];
                j.m_fc[i] = j.log2fc[(size_t)r * (size_t)n + s];
            }
            at += (uint64_t)__popcll(bits);
        }
    }
}

// ---- exclusive scan of uint32 counts into uint64 offsets: out[i] = base + in[0] + .. + in[i - 1] ----
__device__ __forceinline__ uint64_t emcnv_wg_scan(uint64_t v, uint64_t* lds, uint64_t* total)
{
    // inclusive scan over the workgroup's threads; returns the exclusive value
    const int t = threadIdx.x;
    lds[t] = v;
    __syncthreads();
    for (int o = 1; o < EMCNV_WG; o <<= 1) {
        const uint64_t add = t >= o ? lds[t - o] : 0;
        __syncthreads();
        lds[t] += add;
        __syncthreads();
    }
    const uint64_t incl = lds[t];
    *total = lds[EMCNV_WG - 1];
    __syncthreads();
    return incl - v;
}

__global__ __launch_bounds__(EMCNV_WG) void gd_emcnv_scan_tile_kernel(const uint32_t* in, uint64_t n, uint64_t* tile_sum)
{
    __shared__ uint64_t lds[EMCNV_WG];
    const uint64_t at = (uint64_t)blockIdx.x * EMCNV_SCAN_TILE + (uint64_t)threadIdx.x * 4;
    uint64_t v = 0;
    for (int k = 0; k < 4; ++k)
        if (at + k < n) v += in[at + k];
    uint64_t total;
    (void)emcnv_wg_scan(v, lds, &total);
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = total;
}

// one workgroup: the tile sums become the tiles' offsets; out_total[0] = base + everything
__global__ __launch_bounds__(EMCNV_WG) void gd_emcnv_scan_top_kernel(uint64_t* tile_sum, uint64_t n_tiles, uint64_t base,
                                                                     uint64_t* out_total)
{
    __shared__ uint64_t lds[EMCNV_WG];
    uint64_t run = base;
    for (uint64_t t0 = 0; t0 < n_tiles; t0 += EMCNV_WG) {
        const uint64_t i = t0 + threadIdx.x;
        const uint64_t v = i < n_tiles ? tile_sum[i] : 0;
        uint64_t total;
        const uint64_t ex = emcnv_wg_scan(v, lds, &total);
        if (i < n_tiles) tile_sum[i] = run + ex;
        run += total;
    }
    if (threadIdx.x == 0) out_total[0] = run;
}

__global__ __launch_bounds__(EMCNV_WG) void gd_emcnv_scan_apply_kernel(const uint32_t* in, uint64_t n, const uint64_t* tile_off,
                                                                       uint64_t* out)
{
    __shared__ uint64_t lds[EMCNV_WG];
    const uint64_t at = (uint64_t)blockIdx.x * EMCNV_SCAN_TILE + (uint64_t)threadIdx.x * 4;
    uint32_t x[4];
    uint64_t v = 0;
    for (int k = 0; k < 4; ++k) {
        x[k] = at + k < n ? in[at + k] : 0;
        v += x[k];
    }
    uint64_t total;
    uint64_t run = tile_off[blockIdx.x] + emcnv_wg_scan(v, lds, &total);
    for (int k = 0; k < 4; ++k) {
        if (at + k < n) out[at + k] = run;
        run += x[k];
    }
}

// ---- finish ----
struct EmcnvJob {
    uint32_t R;                                  // rows
    int32_t n, words;
    uint32_t n_chunks;
    const uint32_t* start; const uint32_t* end;  // [R]
    uint32_t* F;                                 // [R]
    uint32_t* span1;                             // [ceil(R / 64)][4]: min, max of start and of start + 2^31 over 64 rows
    uint32_t* span2;                             // [ceil(R / 4096)][4]: the same over 4096 rows
    const uint64_t* mbits;                       // [R][words]
    const uint64_t* rowoff;                      // [R]
    // chunk summaries [n_chunks][words * 64]; gd_emcnv_carry_kernel turns first / tail into what the chunk starts from
    uint32_t* first;                             // first member        -> the latest member before the chunk
    uint32_t* last;                              // last member
    uint32_t* lastF;                             // F[last]
    uint32_t* tail;                              // length of the last run | EMCNV_ONE_RUN -> length of the open run
    uint32_t* psize;                             // [R + 1]
    uint32_t* ecnt;                              // [R + 1] CNVs emitted at a row
    uint64_t* ebits;                             // [R + 1][words] their samples
    const uint64_t* eoff;                        // [R + 1]
    uint32_t* c_sample; uint32_t* c_psize; uint32_t* c_emit; uint32_t* c_count; uint32_t* c_last;   // [n_cnvs]
    uint64_t n_cnvs;
    const uint64_t* member_off;                  // [n_cnvs + 1]
    const float* m_depth; const uint8_t* m_cn; const float* m_fc;    // the arena
    uint32_t* o_row; float* o_depth; uint8_t* o_cn; float* o_fc;     // [n_members]
};

// The span of the starts of a block of rows, as (min, max) of start and of start + 2^31 (mod 2^32): a window of 30 000
// positions does not wrap in at least one of the two, so "every start of the block lies inside the window" is two
// compares.  LEVEL 1: blocks of 64 rows; LEVEL 2: blocks of 64 of those (4096 rows).  One wavefront a block.
__device__ __forceinline__ uint32_t emcnv_wave_min(uint32_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const uint32_t x = (uint32_t)__shfl_xor((int)v, o, 64); v = x < v ? x : v; }
    return v;
}
__device__ __forceinline__ uint32_t emcnv_wave_max(uint32_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const uint32_t x = (uint32_t)__shfl_xor((int)v, o, 64); v = x > v ? x : v; }
    return v;
}

template <int LEVEL>
__global__ __launch_bounds__(EMCNV_WG) void gd_emcnv_span_kernel(EmcnvJob j)
{
    const int lane = threadIdx.x & 63;
    const uint64_t b = (uint64_t)blockIdx.x * EMCNV_WAVES + (uint64_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t n1 = ((uint64_t)j.R + 63) / 64, n_out = LEVEL == 1 ? n1 : (n1 + 63) / 64;
    if (b >= n_out) return;
    const uint64_t n_in = LEVEL == 1 ? (uint64_t)j.R : n1;
    uint64_t i = b * 64 + lane;
    if (i >= n_in) i = b * 64;                   // (the block's first element is there: it stands in for the missing ones)
    uint32_t mn, mx, mns, mxs;
    if constexpr (LEVEL == 1) {
        mn = mx = j.start[i];
        mns = mxs = mn ^ EMCNV_HALF;
    } else {
        mn = j.span1[i * 4]; mx = j.span1[i * 4 + 1]; mns = j.span1[i * 4 + 2]; mxs = j.span1[i * 4 + 3];
    }
    mn = emcnv_wave_min(mn); mx = emcnv_wave_max(mx); mns = emcnv_wave_min(mns); mxs = emcnv_wave_max(mxs);
    uint32_t* out = (LEVEL == 1 ? j.span1 : j.span2) + b * 4;
    if (lane == 0) { out[0] = mn; out[1] = mx; out[2] = mns; out[3] = mxs; }
}

// every start of the block lies in [lo, lo + 29999] (mod 2^32): no row of it is a gap for an end of `lo`
__device__ __forceinline__ bool emcnv_all_inside(const uint32_t* span, uint32_t lo)
{
    const uint32_t hi = lo + (EMCNV_GAP - 1);
    if (hi >= lo) return span[0] >= lo && span[1] <= hi;
    const uint32_t los = lo ^ EMCNV_HALF;        // (lo is within 30 000 of 2^32: shifted by 2^31 the window does not wrap)
    return span[2] >= los && span[3] <= los + (EMCNV_GAP - 1);
}

// F, one thread a row: forward from a + 1 to the first gap row, over whole blocks of 4096 and of 64 rows whose starts
// all lie inside the window.  On tiled rows that is 30 000 / width steps; on rows that never gap (repeated positions) at
// most 63 + 63 + R / 4096 instead of R.  The grid covers the rows (R / 256 < 2^24 workgroups).
__global__ __launch_bounds__(EMCNV_WG) void gd_emcnv_gap_kernel(EmcnvJob j)
{
    const uint32_t R = j.R;
    const uint64_t a = (uint64_t)blockIdx.x * EMCNV_WG + threadIdx.x;
    if (a >= R) return;
    const uint32_t e = j.end[a];
    uint32_t f = (uint32_t)(j.start[R - 1] + EMCNV_FINAL - e) >= EMCNV_GAP ? R : R + 1;
    for (uint64_t r = a + 1; r < R;) {
        if ((r & 4095) == 0 && emcnv_all_inside(j.span2 + (r >> 12) * 4, e)) { r += 4096; continue; }
        if ((r & 63) == 0 && emcnv_all_inside(j.span1 + (r >> 6) * 4, e)) { r += 64; continue; }
        if ((uint32_t)(j.start[r] - e) >= EMCNV_GAP) { f = (uint32_t)r; break; }
        ++r;
    }
    j.F[a] = f;
}

// The (chunk, word) pairs are the wave items of the two chunk kernels; their grids cover the pairs (at most 2^24 chunks
// of 64 words, four pairs a workgroup: below 2^31 workgroups), so no loop strides over them.
__global__ __launch_bounds__(EMCNV_WG) void gd_emcnv_chunk_kernel(EmcnvJob j)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t items = (uint64_t)j.n_chunks * (uint64_t)j.words;
    const uint64_t it = (uint64_t)blockIdx.x * EMCNV_WAVES + wave;
    if (it < items) {
        const uint32_t c = (uint32_t)(it / (uint64_t)j.words);
        const int w = (int)(it % (uint64_t)j.words);
        const bool col0 = w == 0 && lane == 0;   // sample 0 keeps no list: it takes no part here
        const uint64_t r0 = (uint64_t)c * EMCNV_CHUNK;
        const uint64_t r1 = r0 + EMCNV_CHUNK < j.R ? r0 + EMCNV_CHUNK : j.R;
        uint32_t first = EMCNV_NONE, last = EMCNV_NONE, lastF = 0, tail = 0;
        bool one = true;
        for (uint64_t r = r0; r < r1; ++r) {
            const uint64_t bits = j.mbits[r * (uint64_t)j.words + w];
            if (bits == 0) continue;
            if (((bits >> lane) & 1ull) && !col0) {
                if (last == EMCNV_NONE) { first = (uint32_t)r; tail = 1; }
                else if (lastF > r) ++tail;
                else { tail = 1; one = false; }
                last = (uint32_t)r;
                lastF = j.F[r];
            }
        }
        const size_t o = (size_t)c * (size_t)j.words * 64 + (size_t)w * 64 + lane;
        j.first[o] = first; j.last[o] = last; j.lastF[o] = lastF; j.tail[o] = tail | (one ? EMCNV_ONE_RUN : 0u);
    }
}

__global__ __launch_bounds__(EMCNV_WG) void gd_emcnv_carry_kernel(EmcnvJob j)
{
    const size_t pad = (size_t)j.words * 64;
    const size_t s = (size_t)blockIdx.x * EMCNV_WG + threadIdx.x;
    if (s >= pad) return;
    uint32_t latest = EMCNV_NONE, latestF = 0, run = 0;
    for (uint32_t c = 0; c < j.n_chunks; ++c) {
        const size_t o = (size_t)c * pad + s;
        const uint32_t first = j.first[o], last = j.last[o], lastF = j.lastF[o], t = j.tail[o];
        j.first[o] = latest;
        j.tail[o] = run;
        if (last != EMCNV_NONE) {
            const bool joined = latest != EMCNV_NONE && latestF > first;
            const uint32_t len = t & ~EMCNV_ONE_RUN;
            run = (t & EMCNV_ONE_RUN) && joined ? run + len : len;
            latest = last;
            latestF = lastF;
        }
    }
}

template <int PHASE>
__device__ __forceinline__ void emcnv_close(const EmcnvJob& j, int w, int lane, uint32_t a, uint32_t e, uint32_t k)
{
    if (e > j.R) return;                         // R + 1: the final test failed, the list is never emitted
    if constexpr (PHASE == 0) {
        atomicAdd(&j.ecnt[e], 1u);
        atomicOr(reinterpret_cast<unsigned long long*>(&j.ebits[(size_t)e * (size_t)j.words + w]), 1ull << lane);
    } else {
        const uint64_t i = j.eoff[e] + emcnv_rank(j.ebits + (size_t)e * (size_t)j.words, w, lane);
        j.c_sample[i] = (uint32_t)(w * 64 + lane);
        j.c_psize[i] = j.psize[e];
        j.c_emit[i] = e;
        j.c_count[i] = k;
        j.c_last[i] = a;
    }
}

template <int PHASE>
__global__ __launch_bounds__(EMCNV_WG) void gd_emcnv_emit_kernel(EmcnvJob j)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t items = (uint64_t)j.n_chunks * (uint64_t)j.words;
    const uint64_t it = (uint64_t)blockIdx.x * EMCNV_WAVES + wave;
    if (it < items) {
        const uint32_t c = (uint32_t)(it / (uint64_t)j.words);
        const int w = (int)(it % (uint64_t)j.words);
        const bool col0 = w == 0 && lane == 0;
        const uint64_t r0 = (uint64_t)c * EMCNV_CHUNK;
        const uint64_t r1 = r0 + EMCNV_CHUNK < j.R ? r0 + EMCNV_CHUNK : j.R;
        const size_t o = (size_t)c * (size_t)j.words * 64 + (size_t)w * 64 + lane;
        uint32_t latest = j.first[o], run = j.tail[o];
        uint32_t latestF = latest != EMCNV_NONE ? j.F[latest] : 0;
        // pending(s, r): the list of column s is not empty when Clear runs for row r (r == R: Clear(nil))
        auto pending = [&](uint64_t r) {
            const bool p = col0 ? (r > 0 && (j.mbits[(r - 1) * (uint64_t)j.words] & 1ull))
                                : (latest != EMCNV_NONE && latestF >= r);
            const uint32_t k = (uint32_t)__popcll(__ballot(p));
            if (lane == 0 && k) atomicAdd(&j.psize[r], k);
        };
        for (uint64_t r = r0; r < r1; ++r) {
            const uint64_t bits = j.mbits[r * (uint64_t)j.words + w];
            if constexpr (PHASE == 0) pending(r);
            if (bits == 0) continue;
            if ((bits >> lane) & 1ull) {
                if (col0) {
                    const uint32_t f = j.F[r];
                    if (f == (uint32_t)r + 1) emcnv_close<PHASE>(j, w, lane, (uint32_t)r, f, 1u);
                } else {
                    if (latest != EMCNV_NONE && latestF > r) ++run;
                    else {
                        if (latest != EMCNV_NONE) emcnv_close<PHASE>(j, w, lane, latest, latestF, run);
                        run = 1;
                    }
                    latest = (uint32_t)r;
                    latestF = j.F[r];
                }
            }
        }
        if (c == j.n_chunks - 1) {
            if constexpr (PHASE == 0) pending(j.R);
            if (!col0 && latest != EMCNV_NONE) emcnv_close<PHASE>(j, w, lane, latest, latestF, run);
        }
    }
}

// One wavefront a CNV: lane l looks at row (top - l) of the CNV's column, a ballot says which of the 64 rows hold members,
// and every such lane copies its member -- 64 rows a step, so a run over 100 000 rows takes 1 600 steps, not 100 000.
// The grid covers the CNVs (gd_emcnv_finish refuses more than 2^33 - 4 of them).
__global__ __launch_bounds__(EMCNV_WG) void gd_emcnv_members_kernel(EmcnvJob j)
{
    const int lane = threadIdx.x & 63;
    const uint64_t i = (uint64_t)blockIdx.x * EMCNV_WAVES + (uint64_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (i >= j.n_cnvs) return;
    const uint32_t s = j.c_sample[i];
    const int w = (int)(s >> 6), b = (int)(s & 63);
    const uint64_t off = j.member_off[i];
    uint32_t left = j.c_count[i];                // members still above `top`, its own included
    int64_t top = (int64_t)j.c_last[i];
    while (left > 0 && top >= 0) {               // (the run's members are there: `left` reaches 0 first)
        const int64_t r = top - lane;
        const bool m = r >= 0 && ((j.mbits[(uint64_t)r * (uint64_t)j.words + w] >> b) & 1ull);
        const uint64_t found = __ballot(m);
        const uint32_t before = (uint32_t)__popcll(found & emcnv_below(lane));       // members of rows nearer the top
        if (m && before < left) {
            const uint64_t src = j.rowoff[r] + emcnv_rank(j.mbits + (uint64_t)r * (uint64_t)j.words, w, b);
            const uint64_t dst = off + (left - 1 - before);
            j.o_row[dst] = (uint32_t)r;
            j.o_depth[dst] = j.m_depth[src];
            j.o_cn[dst] = j.m_cn[src];
            j.o_fc[dst] = j.m_fc[src];
        }
        const uint32_t n = (uint32_t)__popcll(found);
        left = n >= left ? 0 : left - n;
        top -= 64;
    }
}

}  // namespace gd
