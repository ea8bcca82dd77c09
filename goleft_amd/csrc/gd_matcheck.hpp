// gd_matcheck.hpp -- what the entry points that take a [rows][samples] depth matrix decide on the host before anything
// reaches the device: which cell is not a depth, whether the matrix fits an allocation, whether two buffers share a byte,
// the order of the rows by their covariate and ChunkDebiaser's chunks over that order.  Plain C++17 without a HIP include
// or a context, so tests/test_matcheck_host.py runs it on the CPU (tests/emul/matcheck_emul.cpp); the messages and status
// codes are the callers' (gd_api_devmat.inc).
#pragma once

#include <algorithm>
#include <cfloat>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace gdm {

constexpr size_t kNone = ~(size_t)0;

// The first of v[0 .. n) that is not a finite number >= 0 (-0.0 is one, a negative denormal is not), or kNone.  For the
// cells of a matrix -- row i / samples, sample i % samples -- and for a vector of per-sample scales.  Two ordered compares
// say it: both are false for a NaN, the first for everything below zero, the second for +inf.
inline size_t first_bad(const float* v, size_t n)
{
    for (size_t i = 0; i < n; ++i)
        if (!(v[i] >= 0.0f && v[i] <= FLT_MAX)) return i;
    return kNone;
}

// Whether n_rows x max(n_samples, min_cols) float64 values -- the largest array a call makes of the matrix -- have a size.
inline bool fits(size_t n_rows, size_t n_samples, size_t min_cols)
{
    return n_rows <= (SIZE_MAX / sizeof(double)) / std::max(n_samples, min_cols);
}

// whether [a, a + na) and [b, b + nb) share a byte
inline bool overlap(const void* a, size_t na, const void* b, size_t nb)
{
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

// The rows in ascending order of their covariate (debiaser.go:56-76), equal values (-0.0 and 0.0 are) by row: the order
// tests/debias_ref.py and tests/movdebias_ref.py state, bit for bit.  Every value is finite; fewer than 2^32 rows.
inline std::vector<uint32_t> argsort(const double* vals, size_t n_rows)
{
    std::vector<uint32_t> order(n_rows);
    for (size_t r = 0; r < n_rows; ++r) order[r] = (uint32_t)r;
    std::sort(order.begin(), order.end(), [vals](uint32_t a, uint32_t b) { return vals[a] < vals[b] || (vals[a] == vals[b] && a < b); });
    return order;
}

// ChunkDebiaser's chunks (debiaser.go:140-148): chunk k is order[slices[k] .. slices[k + 1]).
struct Chunks {
    std::vector<uint32_t> slices;            // count() + 1 offsets into the order
    std::vector<uint32_t> chunk_of_row;      // by row, not by rank
    size_t largest = 0;                      // rows of the largest chunk
    size_t count() const { return slices.size() - 1; }
};

// The walk over the sorted values: a row opens the next chunk when its value, in float64, is more than `window` above the
// value that opened the current one (a difference equal to the window does not).  A boundary never parts equal values, so
// the order among them is immaterial to the chunks.  n_rows >= 1.
inline Chunks chunk_walk(const double* vals, const std::vector<uint32_t>& order, double window)
{
    const size_t n_rows = order.size();
    Chunks ch;
    ch.chunk_of_row.resize(n_rows);
    ch.slices.push_back(0);
    double v0 = vals[order[0]];
    for (size_t i = 0; i < n_rows; ++i) {
        const double v = vals[order[i]];
        if (v - v0 > window) {
            v0 = v;
            ch.largest = std::max(ch.largest, i - (size_t)ch.slices.back());
            ch.slices.push_back((uint32_t)i);
        }
        ch.chunk_of_row[order[i]] = (uint32_t)(ch.slices.size() - 1);
    }
    ch.largest = std::max(ch.largest, n_rows - (size_t)ch.slices.back());
    ch.slices.push_back((uint32_t)n_rows);
    return ch;
}

}  // namespace gdm
