// gd_svdlog2.hpp -- dcnv's Log2 scaler (dcnv/scalers/scalers.go:134-164 of the reference, through ColCentered{gmean},
// :63-100 and :126-132) around the SVD debiaser of gd_svddebias.hpp: l = log2(1 + a), every SAMPLE
// centred on its upper median over all rows, c_j = sorted(l_.j)[rows / 2], zeros included; the cut and the projection of
// section 3.16 on z = l - c; out = max(0, 2^(z' + c) - 1), one rounding to float32.
//
// Two definitions of this project's, where the reference's own test and its code disagree:
//   the "- 1"   the reference's UnScale returns 2^x, so a round trip gives depth + 1 and its TestLog2RoundTrip
//               (scalers_test.go:49-79), which wants the input back within 0.001, fails.  The test's contract is served.
//   the clamp   a zero cell can leave the projection with a negative exponent: max(0, .), as ZScore.UnScale has it.
//
// log2 is monotone, so c_j = log2(1 + m_j) with m_j the rows / 2-th smallest raw cell of the column: gd_colselect.hpp's
// radix select finds m_j on the float32 bits (gd_colmid_pick_kernel), and nothing is sorted.
//
//   gd_svl_centre_kernel        centre[j] = sl_log(m_j), float64, from the select's keys: the same routine the cells go
//                               through, so a cell that IS its column's centre gives z = 0 exactly.
//   SvLog2                      the scaler policy of gd_svddebias.hpp's gd_svd_gram_kernel<P> and
//                               gd_svd_project_kernel<P, NV>: no state for a row, centre[column] for a column,
//                               z = sl_log(a) - centre, and back = (float)max(0, exp2(z' + centre) - 1).  The kernels are
//                               the linear scalers' own text, so tiles, slabs, chunks, LDS and the order of additions are
//                               theirs; gd_svd_gram_sum_kernel sums the partials in slab order.  The projection loads
//                               centre[column] where it uses it, going in and coming back: NV centres more a lane have no
//                               room beside 3 x NV float64 at NV = 16.
//
// z is never stored: log2 in float64 is a software routine of a few dozen instructions, and the Gram kernel converts a cell
// once per pair of tiles its column is in.  A form that staged l once as float64 (8 bytes a cell) was measured beside this
// one: its kernels were faster and its call slower, by the allocation of twice the matrix; DESIGN.md section 3.17 has the
// table.  No scratch, no atomics; LDS in the Gram kernel only.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gd_svddebias.hpp"

namespace gd {

__device__ __forceinline__ double sl_log(float a) { return log2(1.0 + (double)a); }

// the Log2 scaler's policy; back() holds the two definitions above, the "- 1" and the clamp
struct SvLog2 {
    struct Row {};
    struct Col { double ce; };
    static __device__ __forceinline__ Row row(const SvJob&, int64_t, bool) { return Row{}; }
    static __device__ __forceinline__ Col col(const SvJob& j, int c, bool ok) { return Col{ok ? j.centre[c] : 0.0}; }
    static __device__ __forceinline__ double z(float a, const Row&, const Col& c) { return sl_log(a) - c.ce; }
    static __device__ __forceinline__ float back(const SvJob&, double zp, const Row&, const Col& c)
    {
        const double r = exp2(zp + c.ce) - 1.0;
        return (float)(r > 0.0 ? r : 0.0);
    }
};

__global__ __launch_bounds__(SV_WG) void gd_svl_centre_kernel(SvJob j)
{
    const int i = (int)blockIdx.x * SV_WG + (int)threadIdx.x;
    if (i < j.n) j.centre[i] = sl_log(__uint_as_float((uint32_t)j.keys[i]));
}

}  // namespace gd
