// gd_eigh.hpp -- the eigenpairs of a real symmetric matrix on the host, for the two callers that factorise a small Gram
// matrix the device built: indexcov's principal components (host/indexcov_host.cpp) and the SVD
// debiaser's right singular vectors (gd_api_svddebias.inc, section 3.16).  Plain C++17 without a HIP include or a context,
// so tests/test_eigh_host.py runs it on the CPU (tests/emul/eigh_emul.cpp).  O(N^3) on one thread: the callers bound N.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <vector>

namespace gde {

// Householder reduction to tridiagonal form, then QL with implicit shifts (EISPACK tred2 / tql2 as restated in JAMA,
// public domain).  V (N x N, N >= 1) holds the matrix on entry and is stored COLUMN-major -- the matrix is symmetric, so
// it reads the same -- which makes every O(N^3) loop below (columns of V over k) contiguous; on return eigenvector c is at
// &V[c * N] (unit length) and its eigenvalue is d[c], in no particular order.  0, or -2 when an eigenvalue has not
// converged after 300 sweeps.
inline int sym_eigen(size_t N, std::vector<double>& V, std::vector<double>& d)
{
    std::vector<double> e(N);
    d.assign(N, 0.0);
#define VV(r, c) V[(size_t)(c) * N + (size_t)(r)]
    for (size_t j = 0; j < N; ++j) d[j] = VV(N - 1, j);
    for (size_t i = N - 1; i > 0; --i) {
        double scale = 0, h = 0;
        for (size_t kk = 0; kk < i; ++kk) scale += std::fabs(d[kk]);
        if (scale == 0.0) {
            e[i] = d[i - 1];
            for (size_t j = 0; j < i; ++j) { d[j] = VV(i - 1, j); VV(i, j) = 0; VV(j, i) = 0; }
        } else {
            for (size_t kk = 0; kk < i; ++kk) { d[kk] /= scale; h += d[kk] * d[kk]; }
            double f = d[i - 1], gg = std::sqrt(h);
            if (f > 0) gg = -gg;
            e[i] = scale * gg;
            h -= f * gg;
            d[i - 1] = f - gg;
            for (size_t j = 0; j < i; ++j) e[j] = 0;
            for (size_t j = 0; j < i; ++j) {
                f = d[j];
                VV(j, i) = f;
                gg = e[j] + VV(j, j) * f;
                const double* __restrict__ col = &VV(0, j);
                for (size_t kk = j + 1; kk < i; ++kk) { gg += col[kk] * d[kk]; e[kk] += col[kk] * f; }
                e[j] = gg;
            }
            f = 0;
            for (size_t j = 0; j < i; ++j) { e[j] /= h; f += e[j] * d[j]; }
            const double hh = f / (h + h);
            for (size_t j = 0; j < i; ++j) e[j] -= hh * d[j];
            for (size_t j = 0; j < i; ++j) {
                f = d[j];
                gg = e[j];
                double* __restrict__ col = &VV(0, j);
                for (size_t kk = j; kk < i; ++kk) col[kk] -= f * e[kk] + gg * d[kk];
                d[j] = VV(i - 1, j);
                VV(i, j) = 0;
            }
        }
        d[i] = h;
    }
    for (size_t i = 0; i + 1 < N; ++i) {                                       // accumulate the transformations
        VV(N - 1, i) = VV(i, i);
        VV(i, i) = 1.0;
        const double h = d[i + 1];
        if (h != 0.0) {
            const double* __restrict__ w = &VV(0, i + 1);
            for (size_t kk = 0; kk <= i; ++kk) d[kk] = w[kk] / h;
            for (size_t j = 0; j <= i; ++j) {
                double* __restrict__ col = &VV(0, j);
                double gg = 0;
                for (size_t kk = 0; kk <= i; ++kk) gg += w[kk] * col[kk];
                for (size_t kk = 0; kk <= i; ++kk) col[kk] -= gg * d[kk];
            }
        }
        for (size_t kk = 0; kk <= i; ++kk) VV(kk, i + 1) = 0;
    }
    for (size_t j = 0; j < N; ++j) { d[j] = VV(N - 1, j); VV(N - 1, j) = 0; }
    VV(N - 1, N - 1) = 1.0;
    e[0] = 0;
    // tql2
    for (size_t i = 1; i < N; ++i) e[i - 1] = e[i];
    e[N - 1] = 0;
    {
        double f = 0, tst1 = 0;
        const double eps = 2.220446049250313e-16;
        for (size_t l = 0; l < N; ++l) {
            tst1 = std::max(tst1, std::fabs(d[l]) + std::fabs(e[l]));
            size_t m = l;
            while (m < N) { if (std::fabs(e[m]) <= eps * tst1) break; ++m; }
            if (m >= N) m = N - 1;                                             // (e[N - 1] == 0 stops the scan before this)
            if (m > l) {
                int iter = 0;
                do {
                    if (++iter > 300) return -2;
                    double gg = d[l], p = (d[l + 1] - gg) / (2.0 * e[l]), r = std::hypot(p, 1.0);
                    if (p < 0) r = -r;
                    d[l] = e[l] / (p + r);
                    d[l + 1] = e[l] * (p + r);
                    const double dl1 = d[l + 1];
                    double h = gg - d[l];
                    for (size_t i = l + 2; i < N; ++i) d[i] -= h;
                    f += h;
                    p = d[m];
                    double c = 1, c2 = 1, c3 = 1, s1 = 0, s2 = 0;
                    const double el1 = e[l + 1];
                    for (size_t i = m; i-- > l;) {
                        c3 = c2; c2 = c; s2 = s1;
                        gg = c * e[i];
                        h = c * p;
                        r = std::hypot(p, e[i]);
                        e[i + 1] = s1 * r;
                        s1 = e[i] / r;
                        c = p / r;
                        p = c * d[i] - s1 * gg;
                        d[i + 1] = h + s1 * (c * gg + s1 * d[i]);
                        double* __restrict__ vi = &VV(0, i);
                        double* __restrict__ vj = &VV(0, i + 1);
                        for (size_t kk = 0; kk < N; ++kk) {
                            const double t = vj[kk];
                            vj[kk] = s1 * vi[kk] + c * t;
                            vi[kk] = c * vi[kk] - s1 * t;
                        }
                    }
                    p = -s1 * s2 * c3 * el1 * e[l] / dl1;
                    e[l] = s1 * p;
                    d[l] = c * p;
                } while (std::fabs(e[l]) > eps * tst1);
            }
            d[l] += f;
            e[l] = 0;
        }
    }
#undef VV
    return 0;
}

}  // namespace gde
