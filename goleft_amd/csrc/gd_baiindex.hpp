// gd_baiindex.hpp -- from the records of a range (IdxRec, gd_bamdecode.hpp) to what a .bai is assembled from.
//
//   gd_idx_compact_kernel  the slots of every confirmed segment -> one dense array in file order
//   gd_idx_tile_kernel     per record: is it the HEAD of a run (its (reference, bin) differs from its predecessor's; the
//                          predecessor of a range's first record is the last record of the range before), the order checks
//                          (the first offender of each kind by atomic minimum of its ordinal), mapped / unmapped / unplaced
//                          counts (a wave whose records share a reference adds once); per tile the number of heads
//   gd_idx_tscan_kernel    exclusive scan of the tile totals (one workgroup)
//   gd_idx_runs_kernel     the heads in file order: run k begins at head k's virtual offset and ends at head k + 1's (the end
//                          of a record is the begin of the one behind it); the last run's end is the host's (the range's
//                          resume point, or the next range's first head).  Unplaced records form runs too (reference -1):
//                          they end the run in front of them and are dropped by the host
//   gd_idx_linear_kernel   the linear index: per (reference, window of 2^min_shift positions: 16 kb in a .bai) the smallest begin of a record that touches it,
//                          one 64-bit atomic minimum per window and run of lanes (in file order the lowest lane of a wave
//                          holds the smallest begin: a lane whose predecessor covers the window leaves it to that lane).
//                          The array lives as long as the run: a window that continues across ranges comes out as one.
//                          A record that reaches beyond its reference's windows (a read hanging far over the end) is
//                          clamped and reported: the host grows the array and runs the kernel again (minima: idempotent)
#pragma once
#include "gd_bamdecode.hpp"

namespace gd {

constexpr uint32_t IX_TILE = 256;
// acc words: counts, then the ordinal of the first record that ...
enum : uint32_t {
    IX_ACC_NO_COOR = 0,        // records with refID < 0
    IX_ACC_HEADS,              // heads of the range (written by the scan)
    IX_ACC_OVER,               // the most windows a record reaches beyond its reference's share of the linear array (0: none does)
    IX_ERR_BACK,               // ... lies in front of its predecessor on the same reference
    IX_ERR_RESUME,             // ... belongs to a lower reference than its predecessor
    IX_ERR_PLACED,             // ... is placed and follows an unplaced one
    IX_ERR_SPAN,               // ... has POS < 0 or an end beyond the geometry's limit (2^29 for a .bai)
    IX_ACC_WORDS
};

struct IdxRun { int32_t ref; uint32_t bin; uint64_t beg, end; };   // = gd_index_run

struct IdxJob {
    const IdxRec* rec;             // [n] the range's records in file order
    uint64_t n;
    uint64_t rec0;                 // ordinal in the file of rec[0]
    int32_t  has_prev, prev_ref, prev_bin, prev_beg;   // the record in front of rec[0]
    uint32_t* tile_cnt;            // [n_tiles]
    uint64_t* tile_base;           // [n_tiles]
    uint32_t n_tiles;
    int32_t  n_ref;
    IdxRun* runs;                  // [runs_cap]
    uint64_t runs_cap;
    unsigned long long* ref_cnt;   // [n_ref][2] mapped, unmapped
    unsigned long long* acc;       // [IX_ACC_WORDS]
    const uint64_t* lin_off;       // [n_ref + 1]
    unsigned long long* lin;       // [lin_off[n_ref]] all ones: unset
    uint32_t min_shift = 14;       // a window of the linear array spans 2^min_shift positions (14: a .bai's 16 kb)
};

__global__ __launch_bounds__(256) void gd_idx_compact_kernel(const IdxRec* slots, const uint64_t* slot_base, const uint64_t* rec_base,
                                                             const uint32_t* n_rec, uint32_t n_seg, IdxRec* recs, uint64_t n_recs)
{
    const uint32_t s = blockIdx.x;
    if (s >= n_seg) return;
    const IdxRec* const src = slots + slot_base[s];
    const uint64_t base = rec_base[s];
    for (uint32_t k = threadIdx.x; k < n_rec[s]; k += blockDim.x)
        if (base + k < n_recs) recs[base + k] = src[k];
}

// (reference, bin) of record i as one word; an unplaced record's is that of reference -1
__device__ __forceinline__ uint64_t idx_key(int32_t ref, uint32_t bin)
{
    return ref < 0 ? ~0ull : ((uint64_t)(uint32_t)ref << 32) | (bin & IX_BIN);
}

__device__ __forceinline__ bool idx_is_head(const IdxJob& j, uint64_t i, const IdxRec& c)
{
    if (i == 0) return !j.has_prev || idx_key(c.ref, c.bin) != idx_key(j.prev_ref, (uint32_t)j.prev_bin);
    const IdxRec p = j.rec[i - 1];
    return idx_key(c.ref, c.bin) != idx_key(p.ref, p.bin);
}

__global__ __launch_bounds__(256) void gd_idx_tile_kernel(IdxJob j)
{
    __shared__ uint32_t s_cnt[4];
    const uint64_t i = (uint64_t)blockIdx.x * IX_TILE + threadIdx.x;
    const bool valid = i < j.n;
    IdxRec c{-3, 0, 0, 0u, 0ull};
    bool head = false;
    if (valid) {
        c = j.rec[i];
        head = idx_is_head(j, i, c);
        int32_t pref = -2, pbeg = 0;                        // -2: no predecessor
        if (i) { const IdxRec p = j.rec[i - 1]; pref = p.ref; pbeg = p.beg; }
        else if (j.has_prev) { pref = j.prev_ref; pbeg = j.prev_beg; }
        const unsigned long long ord = j.rec0 + i;
        if (c.ref >= 0) {
            if (pref == -1) atomicMin(j.acc + IX_ERR_PLACED, ord);
            else if (pref >= 0 && c.ref < pref) atomicMin(j.acc + IX_ERR_RESUME, ord);
            else if (pref == c.ref && c.beg < pbeg) atomicMin(j.acc + IX_ERR_BACK, ord);
            if (c.bin & IX_BADSPAN) atomicMin(j.acc + IX_ERR_SPAN, ord);
        }
    }
    // counts: one addition per wave when its records share a reference
    const int32_t r0 = __shfl(c.ref, 0, 64);
    const bool uniform = __ballot(valid && c.ref != r0) == 0ull;
    const bool unm = (c.bin & IX_UNMAPPED) != 0u;
    if (uniform) {
        const uint32_t nm = (uint32_t)__popcll(__ballot(valid && !unm)), nu = (uint32_t)__popcll(__ballot(valid && unm));
        if ((threadIdx.x & 63u) == 0u && nm + nu) {
            if (r0 < 0) atomicAdd(j.acc + IX_ACC_NO_COOR, (unsigned long long)(nm + nu));
            else if (r0 < j.n_ref) {
                if (nm) atomicAdd(j.ref_cnt + 2ull * (uint32_t)r0, (unsigned long long)nm);
                if (nu) atomicAdd(j.ref_cnt + 2ull * (uint32_t)r0 + 1, (unsigned long long)nu);
            }
        }
    } else if (valid) {
        if (c.ref < 0) atomicAdd(j.acc + IX_ACC_NO_COOR, 1ull);
        else if (c.ref < j.n_ref) atomicAdd(j.ref_cnt + 2ull * (uint32_t)c.ref + (unm ? 1 : 0), 1ull);
    }
    const uint32_t n = (uint32_t)__popcll(__ballot(head));
    if ((threadIdx.x & 63u) == 0u) s_cnt[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) j.tile_cnt[blockIdx.x] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
}

__global__ __launch_bounds__(256) void gd_idx_tscan_kernel(IdxJob j)
{
    __shared__ uint64_t s_part[256];
    __shared__ uint64_t s_carry;
    if (threadIdx.x == 0) s_carry = 0;
    __syncthreads();
    for (uint32_t base = 0; base < j.n_tiles; base += 256) {
        const uint32_t t = base + threadIdx.x;
        const uint64_t v = t < j.n_tiles ? j.tile_cnt[t] : 0;
        s_part[threadIdx.x] = v;
        __syncthreads();
        for (uint32_t d = 1; d < 256; d <<= 1) {             // inclusive scan, in place
            const uint64_t add = threadIdx.x >= d ? s_part[threadIdx.x - d] : 0;
            __syncthreads();
            s_part[threadIdx.x] += add;
            __syncthreads();
        }
        const uint64_t carry = s_carry;
        if (t < j.n_tiles) j.tile_base[t] = carry + s_part[threadIdx.x] - v;
        __syncthreads();
        if (threadIdx.x == 255) s_carry = carry + s_part[255];
        __syncthreads();
    }
    if (threadIdx.x == 0) j.acc[IX_ACC_HEADS] = s_carry;
}

__global__ __launch_bounds__(256) void gd_idx_runs_kernel(IdxJob j)
{
    __shared__ uint32_t s_cnt[4];
    const uint64_t i = (uint64_t)blockIdx.x * IX_TILE + threadIdx.x;
    IdxRec c{-3, 0, 0, 0u, 0ull};
    bool head = false;
    if (i < j.n) { c = j.rec[i]; head = idx_is_head(j, i, c); }
    const uint64_t m = __ballot(head);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (lane == 0) s_cnt[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    uint64_t k = j.tile_base[blockIdx.x] + (uint64_t)__popcll(m & ((1ull << lane) - 1ull));
    for (uint32_t w = 0; w < wave; ++w) k += s_cnt[w];
    if (!head) return;
    if (k < j.runs_cap) { IdxRun* const r = j.runs + k; r->ref = c.ref < 0 ? -1 : c.ref; r->bin = c.bin & IX_BIN; r->beg = c.vbeg; }
    if (k && k - 1 < j.runs_cap) j.runs[k - 1].end = c.vbeg;
}

__global__ __launch_bounds__(256) void gd_idx_linear_kernel(IdxJob j)
{
    const uint64_t i = (uint64_t)blockIdx.x * IX_TILE + threadIdx.x;
    int32_t ref = -3;
    uint32_t w0 = 1, w1 = 0;                                // the windows this lane touches: w0 .. w1 (none: w0 > w1)
    uint64_t vbeg = 0, base = 0;
    if (i < j.n) {
        const IdxRec c = j.rec[i];
        if (c.ref >= 0 && c.ref < j.n_ref && !(c.bin & IX_BADSPAN)) {
            ref = c.ref;
            vbeg = c.vbeg;
            base = j.lin_off[ref];
            const uint64_t nwin = j.lin_off[ref + 1] - base;
            w0 = (uint32_t)c.beg >> j.min_shift;
            w1 = ((uint32_t)c.end - 1u) >> j.min_shift;
            if (w1 >= nwin) {                              // the host grows the array and runs this kernel again
                atomicMax(j.acc + IX_ACC_OVER, (unsigned long long)(w1 - nwin + 1u));
                if (w0 >= nwin) { w0 = 1; w1 = 0; ref = -3; }
                else w1 = (uint32_t)nwin - 1u;
            }
        }
    }
    const int32_t pref = __shfl_up(ref, 1, 64);
    const uint32_t pw0 = __shfl_up(w0, 1, 64), pw1 = __shfl_up(w1, 1, 64);
    const bool has_prev = (threadIdx.x & 63u) != 0u && pref == ref && ref >= 0;
    for (uint64_t w = w0; w <= w1 && ref >= 0; ++w) {
        if (has_prev && pw0 <= w && w <= pw1) continue;     // the lane in front covers it: its begin is smaller
        atomicMin(j.lin + base + w, (unsigned long long)vbeg);
    }
}

}  // namespace gd
