// gd_indexsplit.hpp -- the cohort sum of `goleft indexsplit` (indexsplit/indexsplit.go:89-114 of the reference;
// DESIGN.md section 3.8): for every reference r and tile i, s[r][i] += float64(size[sample][r][i]) / 1e9 over the
// samples in argument order, in float64.  A sample with fewer tiles, or without the reference, adds nothing there.
//
//   gd_is_sum_kernel        a thread owns one cell and walks the samples of the batch in order, starting from the
//                           cell's value after the batches before: the additions of a cell happen in the reference's
//                           order whatever the batching, so the result is defined bit for bit
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gd {

constexpr int IS_WG = 256;

struct IsJob {
    int32_t n_samples, n_refs;
    const int64_t* sizes;                        // the tiles of the batch's samples, sample after sample
    const int64_t* tile_off;                     // [n_samples * n_refs] into sizes
    const int32_t* tile_cnt;                     // [n_samples * n_refs], <= longest[r]
    const int32_t* longest;                      // [n_refs]
    const int64_t* cell_off;                     // [n_refs] into sums
    double* sums;                                // longest[r] cells per reference, concatenated
};

// grid (blocks of tiles, references).  Offset and count of (sample, reference) depend on the loop counter and the block
// alone: scalar loads.  The 64 loads of a wavefront are consecutive tiles of one sample.  The quotient is the IEEE
// double division and the sum its own rounding (there is no product to contract).
__global__ __launch_bounds__(IS_WG) void gd_is_sum_kernel(IsJob j)
{
    for (int r = blockIdx.y; r < j.n_refs; r += gridDim.y) {
        const int L = j.longest[r];
        double* __restrict__ out = j.sums + j.cell_off[r];
        for (int i = blockIdx.x * IS_WG + threadIdx.x; i < L; i += gridDim.x * IS_WG) {
            double acc = out[i];
            for (int s = 0; s < j.n_samples; ++s) {
                const size_t k = (size_t)s * (size_t)j.n_refs + (size_t)r;
                const int n = j.tile_cnt[k];
                if (i < n) acc += (double)j.sizes[j.tile_off[k] + i] / 1e9;
            }
            out[i] = acc;
        }
    }
}

}  // namespace gd
