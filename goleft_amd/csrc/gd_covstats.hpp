// gd_covstats.hpp -- `goleft covstats` on the device: every record of a fed range in file order, the reference's
// sampling loop as a scan, and histograms of what it samples (covstats/covstats.go:122-220).
//   gd_cs_walk_kernel     (gd_bamdecode.hpp: the one record walk under its covstats policy) one wave per segment; a
//                         segment runs across references and through the unplaced tail: it ends at the next anchor or,
//                         for the range's last segment, at the first record the range does not hold completely.  Every
//                         record is extracted to a CsRec slot of its segment (room for a record per 36 bytes)
//   gd_cs_compact_kernel  the slots of every segment -> one dense array in file order
//   gd_cs_tile_kernel     per tile of records: how many are "good" (mapped, neither duplicate nor QC-failed) and how
//                         many are eligible for an insert
//   gd_cs_tscan_kernel    exclusive scan of the tile totals (one workgroup)
//   gd_cs_select_kernel   per record: its rank among the sizes and among the inserts, its role, and whether it ends the
//                         loop (the n-th insert, or the single-end break): the first such record by atomic minimum
//   gd_cs_hist_kernel     the counts over [0, stop], and the sizes / inserts / template lengths into dense histograms
//                         (a wave adds its most common bin with one atomic) with an overflow list for what falls outside
#pragma once
#include "gd_bamdecode.hpp"

namespace gd {

// Role bits of a record in the sampling loop (gd_cs_select_kernel).
enum : uint32_t {
    CS_UNMAPPED = 1u, CS_COUNTED = 2u, CS_BAD = 4u, CS_DUP = 8u, CS_PROPER = 16u, CS_SIZE = 32u, CS_INSERT = 64u,
};
constexpr int CS_TILE = 1024;        // records per tile of the scan (256 threads x 4)
constexpr int CS_HBINS = 1 << 16;    // dense bins per histogram
constexpr int64_t CS_LO_SIZE = 0, CS_LO_INS = -(CS_HBINS / 2), CS_LO_TL = -(CS_HBINS / 2);

// accumulators (device, 64-bit words): [0..6] unmapped, counted, bad, dup, proper, sizes, inserts; [7] the stop record
// (~0: none); [8..10] overflow entries of sizes, inserts, template lengths
enum { CS_ACC_STOP = 7, CS_ACC_OVF = 8, CS_ACC_WORDS = 12 };

struct CsScanJob {
    const CsRec* rec;               // the range's records, file order
    uint64_t n;
    uint64_t first;                 // records before it still belong to the skip
    int64_t  target;                // -n: inserts to sample
    int64_t  sizes0, ins0;          // sizes and inserts taken in the ranges before
    uint32_t* tile_g;               // [n_tiles] good records of the tile
    uint32_t* tile_e;               // [n_tiles] records eligible for an insert
    uint64_t* pre_g;                // [n_tiles] exclusive prefixes
    uint64_t* pre_e;
    uint32_t n_tiles;
    uint8_t* role;                  // [n]
    unsigned long long* acc;        // [CS_ACC_WORDS]
    unsigned long long* hist;       // [3 * CS_HBINS]: sizes, inserts, template lengths
    int64_t* ovf;                   // [3 * ovf_cap]
    uint64_t ovf_cap;
};

__device__ __forceinline__ bool cs_good(const CsRec& r) { return !(r.flag & 0x4u) && !(r.flag & 0x600u); }
__device__ __forceinline__ bool cs_eligible(const CsRec& r)
{
    return cs_good(r) && (r.flag & 0x2u) && r.pos < r.next_pos && r.mlen != CS_NOT_M;
}

// The segments' slots -> the dense array (a workgroup per segment).
__global__ __launch_bounds__(256) void gd_cs_compact_kernel(const CsRec* slots, const uint64_t* slot_base, const uint64_t* rec_base,
                                                            const uint32_t* n_rec, uint32_t n_seg, CsRec* recs)
{
    const uint32_t s = blockIdx.x;
    if (s >= n_seg) return;
    const CsRec* const src = slots + slot_base[s];
    CsRec* const dst = recs + rec_base[s];
    for (uint32_t k = threadIdx.x; k < n_rec[s]; k += blockDim.x) dst[k] = src[k];
}

// Sum of v over the workgroup (256 threads: four waves).
__device__ __forceinline__ uint32_t cs_block_sum(uint32_t v, uint32_t* s_tmp)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63u) == 0u) s_tmp[threadIdx.x >> 6] = v;
    __syncthreads();
    return s_tmp[0] + s_tmp[1] + s_tmp[2] + s_tmp[3];
}

__global__ __launch_bounds__(256) void gd_cs_tile_kernel(CsScanJob j)
{
    __shared__ uint32_t s_tmp[4];
    const uint64_t t = blockIdx.x;
    uint32_t g = 0, e = 0;
    for (int q = 0; q < 4; ++q) {
        const uint64_t i = t * CS_TILE + (uint64_t)q * 256 + threadIdx.x;
        if (i >= j.first && i < j.n) {
            const CsRec r = j.rec[i];
            g += cs_good(r) ? 1u : 0u;
            e += cs_eligible(r) ? 1u : 0u;
        }
    }
    const uint32_t G = cs_block_sum(g, s_tmp);
    const uint32_t E = cs_block_sum(e, s_tmp);
    if (threadIdx.x == 0) { j.tile_g[t] = G; j.tile_e[t] = E; }
}

// Exclusive scan of the tile totals: thread x takes a contiguous run of tiles.
__global__ __launch_bounds__(256) void gd_cs_tscan_kernel(CsScanJob j)
{
    __shared__ uint64_t s_g[256], s_e[256];
    const uint32_t per = (j.n_tiles + 255u) / 256u;
    const uint32_t b = threadIdx.x * per, e = min(j.n_tiles, b + per);
    uint64_t g = 0, x = 0;
    for (uint32_t k = b; k < e; ++k) { g += j.tile_g[k]; x += j.tile_e[k]; }
    s_g[threadIdx.x] = g;
    s_e[threadIdx.x] = x;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t ag = 0, ae = 0;
        for (int k = 0; k < 256; ++k) {
            const uint64_t tg = s_g[k], te = s_e[k];
            s_g[k] = ag; s_e[k] = ae;
            ag += tg; ae += te;
        }
    }
    __syncthreads();
    g = s_g[threadIdx.x];
    x = s_e[threadIdx.x];
    for (uint32_t k = b; k < e; ++k) {
        j.pre_g[k] = g; j.pre_e[k] = x;
        g += j.tile_g[k]; x += j.tile_e[k];
    }
}

// Thread x of a tile holds records 4x .. 4x+3 of it: their ranks from the tile's prefix and an LDS scan of the threads.
__global__ __launch_bounds__(256) void gd_cs_select_kernel(CsScanJob j)
{
    __shared__ uint32_t s_g[2][256], s_e[2][256];
    const uint64_t t = blockIdx.x;
    const uint32_t x = threadIdx.x;
    const uint64_t i0 = t * CS_TILE + 4ull * x;
    CsRec r[4];
    uint32_t g = 0, e = 0;
    for (int q = 0; q < 4; ++q) {
        const uint64_t i = i0 + q;
        if (i >= j.first && i < j.n) {
            r[q] = j.rec[i];
            g += cs_good(r[q]) ? 1u : 0u;
            e += cs_eligible(r[q]) ? 1u : 0u;
        }
    }
    // inclusive Hillis-Steele scan over the 256 threads
    int cur = 0;
    s_g[0][x] = g;
    s_e[0][x] = e;
    __syncthreads();
    for (uint32_t o = 1; o < 256u; o <<= 1) {
        uint32_t vg = s_g[cur][x], ve = s_e[cur][x];
        if (x >= o) { vg += s_g[cur][x - o]; ve += s_e[cur][x - o]; }
        s_g[cur ^ 1][x] = vg;
        s_e[cur ^ 1][x] = ve;
        cur ^= 1;
        __syncthreads();
    }
    int64_t sz = j.sizes0 + (int64_t)j.pre_g[t] + (int64_t)(s_g[cur][x] - g);   // sizes taken before this thread's first record
    int64_t in = j.ins0 + (int64_t)j.pre_e[t] + (int64_t)(s_e[cur][x] - e);
    const int64_t two_n = 2 * j.target;
    for (int q = 0; q < 4; ++q) {
        const uint64_t i = i0 + q;
        if (i >= j.n) break;
        if (i < j.first) { j.role[i] = 0; continue; }
        const CsRec& c = r[q];
        uint32_t role = 0;
        bool ends = false;
        if (c.flag & 0x4u) {
            role = CS_UNMAPPED;
        } else if (c.flag & 0x600u) {
            role = CS_COUNTED | CS_BAD | ((c.flag & 0x400u) ? CS_DUP : 0u);
        } else {
            role = CS_COUNTED | ((c.flag & 0x2u) ? CS_PROPER : 0u);
            if (sz < two_n) role |= CS_SIZE;
            else if (in == 0) ends = true;                  // single-end data: the loop breaks here (counted, proper)
            if (!ends && cs_eligible(c)) {
                role |= CS_INSERT;
                if (in == j.target - 1) ends = true;        // the n-th insert
            }
            ++sz;                                            // (ranks of the good and eligible records, break or not:
            if (cs_eligible(c)) ++in;                        //  nothing after the first record that ends the loop counts)
        }
        j.role[i] = (uint8_t)role;
        if (ends) atomicMin(&j.acc[CS_ACC_STOP], (unsigned long long)i);
    }
}

// Adds 1 at bin b of h for every lane with want: the wave's most common bin (that of the first lane that wants) with one
// atomic, the rest lane by lane.  Every lane of the wave calls it.
__device__ __forceinline__ void cs_hist_add(unsigned long long* h, bool want, uint32_t b)
{
    const unsigned long long m = __ballot(want);
    if (m == 0ull) return;
    const int leader = __ffsll((long long)m) - 1;
    const uint32_t lb = (uint32_t)__shfl((int)b, leader, 64);
    const bool same = want && b == lb;
    const unsigned long long sm = __ballot(same);
    if ((int)(threadIdx.x & 63u) == leader) atomicAdd(h + lb, (unsigned long long)__popcll(sm));
    if (want && !same) atomicAdd(h + b, 1ull);
}

__device__ __forceinline__ void cs_put(const CsScanJob& j, int k, int64_t lo, bool take, int64_t v)
{
    const bool in_win = take && v >= lo && v < lo + CS_HBINS;
    cs_hist_add(j.hist + (size_t)k * CS_HBINS, in_win, in_win ? (uint32_t)(v - lo) : 0u);
    if (take && !in_win) {
        const unsigned long long at = atomicAdd(&j.acc[CS_ACC_OVF + k], 1ull);
        if (at < j.ovf_cap) j.ovf[(size_t)k * j.ovf_cap + at] = v;
    }
}

__global__ __launch_bounds__(256) void gd_cs_hist_kernel(CsScanJob j)
{
    __shared__ unsigned long long s_cnt[7];
    if (threadIdx.x < 7) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const unsigned long long stop = j.acc[CS_ACC_STOP];
    const uint64_t end = stop < j.n ? stop + 1 : j.n;
    uint32_t cnt[7] = {0, 0, 0, 0, 0, 0, 0};
    const uint64_t t = blockIdx.x;
    for (int q = 0; q < 4; ++q) {                           // (a uniform trip count: cs_hist_add needs the whole wave)
        const uint64_t i = t * CS_TILE + (uint64_t)q * 256 + threadIdx.x;
        const bool in = i >= j.first && i < end;
        const uint32_t role = in ? j.role[i] : 0u;
        CsRec c{};
        if (role & (CS_SIZE | CS_INSERT)) c = j.rec[i];
        for (int b = 0; b < 7; ++b) cnt[b] += (role >> b) & 1u;
        cs_put(j, 0, CS_LO_SIZE, (role & CS_SIZE) != 0u, (int64_t)c.qlen);
        cs_put(j, 1, CS_LO_INS, (role & CS_INSERT) != 0u, (int64_t)c.next_pos - ((int64_t)c.pos + (int64_t)c.mlen));
        cs_put(j, 2, CS_LO_TL, (role & CS_INSERT) != 0u, (int64_t)c.tlen);
    }
    for (int b = 0; b < 7; ++b) {
        uint32_t v = cnt[b];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
        if ((threadIdx.x & 63u) == 0u && v) atomicAdd(&s_cnt[b], (unsigned long long)v);
    }
    __syncthreads();
    if (threadIdx.x < 7 && s_cnt[threadIdx.x]) atomicAdd(&j.acc[threadIdx.x], s_cnt[threadIdx.x]);
}

}  // namespace gd
