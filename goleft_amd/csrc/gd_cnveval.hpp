// gd_cnveval.hpp -- cnveval.Evaluate (cnveval/cnveval.go:163-341 of the reference): the calls of
// every sample scored against a truth set, as counts FP / FN / TP / TN per (sample, size class).
//
// The reference walks a sample's sorted calls with a cursor that it carries from truth to truth.  Here every (sample,
// truth) pair stands alone: the calls that can overlap a truth start at the first one whose running maximum of ends
// passes the truth's start, found by a binary search over key[] = chromosome rank << 32 | running maximum of the ends
// on that chromosome (non-decreasing along a sample's sorted calls; the host fills it while it checks the order).
//
//   gd_cnveval_positive_kernel   steps 1 - 3.  One workgroup a sample that has calls; its work items stride over the
//                                (truth, sample) entries that name the sample.  Every call that matches such a truth
//                                gets CE_OWN, the first one in sorted order CE_COUNTED and the truth a TP; a truth
//                                without one is an FN.  The calls never COUNTED are the sample's FP of step 3: its
//                                calls per class less the calls a work item was the first to mark.  The entry also sets
//                                the sample's bit in the truth's membership word.
//   gd_cnveval_pairs_kernel      step 4, the quadratic one, launched behind the first so that flags[] and member[] are
//                                complete.  One workgroup owns one sample and CE_WG truths a pass (grid.y workgroups a
//                                sample stride over the truths); a work item is one (sample, truth) pair: skipped when
//                                the truth names the sample, else a TN when no call matches, else an FP for every call
//                                from the first match up to a match that is OWN or the end of the truth.
//
// All counters are 64-bit integers.  A work item keeps its counts in named registers (nothing is indexed by a runtime
// value: no scratch), a wavefront sums them by shuffles, the wavefronts of a workgroup meet in twelve LDS words, and
// the workgroup adds the non-zero ones to stats[sample] with integer atomics: the sums do not depend on the order.
// flags[] and member[] are written with atomic ORs only.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gd {

constexpr int CE_WG = 256;                       // work items of a workgroup; truths of one pass of a pairs workgroup
constexpr int CE_TARGET_BLOCKS = 1024;           // pairs launch: about this many workgroups (four a CU) when the truths allow
constexpr int CE_CELLS = 12;                     // [3 classes][FP FN TP TN] of one sample
constexpr unsigned CE_OWN = 1u, CE_COUNTED = 2u;
constexpr int CE_FP = 0, CE_FN = 1, CE_TP = 2, CE_TN = 3;
constexpr int CE_SMALL = 20000, CE_MEDIUM = 100000;

struct CeJob {
    const int64_t* cnv_off;                      // [n_samples + 1]
    const int64_t* key;                          // [n_cnvs] chromosome rank << 32 | running maximum of the ends
    const int32_t* c_start;                      // [n_cnvs], sorted by (chromosome rank, start) within a sample
    const int32_t* c_end;
    const int32_t* c_cn;
    unsigned* flags;                             // [n_cnvs] CE_OWN | CE_COUNTED, zero before the first kernel
    const int32_t* t_chrom;                      // [n_truths]
    const int32_t* t_start;
    const int32_t* t_end;
    const int32_t* t_cn;
    int64_t n_truths;
    const int32_t* active;                       // [grid.x] the samples that have calls
    const int64_t* st_off;                       // [n_samples + 1] the entries that name a sample ...
    const int32_t* st_truth;                     // ... as truth indexes, one per naming
    unsigned* member;                            // [ceil(n_samples / 32)][n_truths] bit s % 32: the truth names sample s
    double po;
    unsigned long long* stats;                   // [n_samples][3][4]
};

__device__ __forceinline__ int ce_class(int start, int end)
{
    const int64_t l = (int64_t)end - start;
    return l < CE_SMALL ? 0 : l < CE_MEDIUM ? 1 : 2;
}

// poverlap(c, t) >= po && sameCN, both on one chromosome (cnveval.go:354-389): one IEEE float64 division; a zero-length
// interval gives 0 / 0 = NaN, which is not >= po
__device__ __forceinline__ bool ce_match(int cs, int ce, int ccn, int ts, int te, int tcn, double po)
{
    const int64_t ovl = (int64_t)(ce < te ? ce : te) - (int64_t)(cs > ts ? cs : ts);
    const double lc = (double)((int64_t)ce - cs), lt = (double)((int64_t)te - ts);
    const double total = lc < lt ? lc : lt;
    const double p = ovl < 0 ? 0.0 : (double)ovl / total;
    return p >= po && (ccn > 2 ? 3 : ccn) == (tcn > 2 ? 3 : tcn);
}

// the first call of [b, e) whose key is above `probe`
__device__ __forceinline__ int64_t ce_first_above(const int64_t* __restrict__ key, int64_t b, int64_t e, int64_t probe)
{
    while (b < e) {
        const int64_t m = b + ((e - b) >> 1);
        if (key[m] > probe) e = m;
        else b = m + 1;
    }
    return b;
}

__device__ __forceinline__ long long ce_wave_sum(long long v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// every work item of the workgroup calls this for every slot; acc[] is zero before the first call
__device__ __forceinline__ void ce_meet(unsigned long long* acc, int slot, long long v)
{
    v = ce_wave_sum(v);
    if ((threadIdx.x & 63) == 0 && v != 0) atomicAdd(&acc[slot], (unsigned long long)v);
}

__device__ __forceinline__ void ce_flush(const CeJob& j, int64_t s, unsigned long long* acc)
{
    __syncthreads();
    if (threadIdx.x < CE_CELLS) {
        const unsigned long long v = acc[threadIdx.x];
        if (v != 0) atomicAdd(&j.stats[s * CE_CELLS + threadIdx.x], v);
    }
}

__global__ __launch_bounds__(CE_WG) void gd_cnveval_positive_kernel(const CeJob j)
{
    __shared__ unsigned long long acc[CE_CELLS];
    if (threadIdx.x < CE_CELLS) acc[threadIdx.x] = 0;
    __syncthreads();
    const int64_t s = j.active[blockIdx.x];
    const int64_t b = j.cnv_off[s], e = j.cnv_off[s + 1];
    unsigned* const word = j.member + (s >> 5) * j.n_truths;
    const unsigned bit = 1u << (s & 31);
    long long tp0 = 0, tp1 = 0, tp2 = 0, fn0 = 0, fn1 = 0, fn2 = 0, fp0 = 0, fp1 = 0, fp2 = 0;
    for (int64_t k = j.st_off[s] + threadIdx.x; k < j.st_off[s + 1]; k += CE_WG) {
        const int64_t t = j.st_truth[k];
        atomicOr(&word[t], bit);
        const int tc = j.t_chrom[t], ts = j.t_start[t], te = j.t_end[t], tcn = j.t_cn[t];
        bool found = false;
        for (int64_t c = ce_first_above(j.key, b, e, ((int64_t)tc << 32) | (int64_t)ts); c < e; ++c) {
            if ((int)(j.key[c] >> 32) != tc) break;
            const int cs = j.c_start[c];
            if (cs > te) break;
            const int ce = j.c_end[c];
            if (!ce_match(cs, ce, j.c_cn[c], ts, te, tcn, j.po)) continue;
            if (found) {
                atomicOr(&j.flags[c], CE_OWN);
                continue;
            }
            found = true;
            // the first work item to count this call takes it out of the sample's uncounted ones
            if (!(atomicOr(&j.flags[c], CE_OWN | CE_COUNTED) & CE_COUNTED)) {
                const int cc = ce_class(cs, ce);
                fp0 -= cc == 0; fp1 -= cc == 1; fp2 -= cc == 2;
            }
        }
        const int cls = ce_class(ts, te);
        tp0 += found && cls == 0; tp1 += found && cls == 1; tp2 += found && cls == 2;
        fn0 += !found && cls == 0; fn1 += !found && cls == 1; fn2 += !found && cls == 2;
    }
    for (int64_t c = b + threadIdx.x; c < e; c += CE_WG) {
        const int cc = ce_class(j.c_start[c], j.c_end[c]);
        fp0 += cc == 0; fp1 += cc == 1; fp2 += cc == 2;
    }
    ce_meet(acc, 0 * 4 + CE_FP, fp0); ce_meet(acc, 0 * 4 + CE_FN, fn0); ce_meet(acc, 0 * 4 + CE_TP, tp0);
    ce_meet(acc, 1 * 4 + CE_FP, fp1); ce_meet(acc, 1 * 4 + CE_FN, fn1); ce_meet(acc, 1 * 4 + CE_TP, tp1);
    ce_meet(acc, 2 * 4 + CE_FP, fp2); ce_meet(acc, 2 * 4 + CE_FN, fn2); ce_meet(acc, 2 * 4 + CE_TP, tp2);
    ce_flush(j, s, acc);
}

__global__ __launch_bounds__(CE_WG) void gd_cnveval_pairs_kernel(const CeJob j)
{
    __shared__ unsigned long long acc[CE_CELLS];
    if (threadIdx.x < CE_CELLS) acc[threadIdx.x] = 0;
    __syncthreads();
    const int64_t s = j.active[blockIdx.x];
    const int64_t b = j.cnv_off[s], e = j.cnv_off[s + 1];
    const unsigned* const word = j.member + (s >> 5) * j.n_truths;
    const int shift = (int)(s & 31);
    long long fp0 = 0, fp1 = 0, fp2 = 0, tn0 = 0, tn1 = 0, tn2 = 0;
    for (int64_t t = (int64_t)blockIdx.y * CE_WG + threadIdx.x; t < j.n_truths; t += (int64_t)gridDim.y * CE_WG) {
        if ((word[t] >> shift) & 1u) continue;                       // the truth names the sample: step 2 had it
        const int tc = j.t_chrom[t], ts = j.t_start[t], te = j.t_end[t], tcn = j.t_cn[t];
        bool started = false;
        long long run = 0;
        for (int64_t c = ce_first_above(j.key, b, e, ((int64_t)tc << 32) | (int64_t)ts); c < e; ++c) {
            if ((int)(j.key[c] >> 32) != tc) break;
            const int cs = j.c_start[c];
            if (cs > te) break;
            const bool m = ce_match(cs, j.c_end[c], j.c_cn[c], ts, te, tcn, j.po);
            if (m && (j.flags[c] & CE_OWN)) { started = true; break; }       // (a first match that is OWN: neither FP nor TN)
            started = started || m;
            run += started;
        }
        const int cls = ce_class(ts, te);
        fp0 += cls == 0 ? run : 0; fp1 += cls == 1 ? run : 0; fp2 += cls == 2 ? run : 0;
        tn0 += !started && cls == 0; tn1 += !started && cls == 1; tn2 += !started && cls == 2;
    }
    ce_meet(acc, 0 * 4 + CE_FP, fp0); ce_meet(acc, 0 * 4 + CE_TN, tn0);
    ce_meet(acc, 1 * 4 + CE_FP, fp1); ce_meet(acc, 1 * 4 + CE_TN, tn1);
    ce_meet(acc, 2 * 4 + CE_FP, fp2); ce_meet(acc, 2 * 4 + CE_TN, tn2);
    ce_flush(j, s, acc);
}

}  // namespace gd
