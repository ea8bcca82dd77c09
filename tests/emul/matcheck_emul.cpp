// matcheck_emul.cpp -- goleft_amd/csrc/gd_matcheck.hpp behind a C ABI, for tests/test_matcheck_host.py (plain C++: the header
// has no HIP in it).
#include "../../goleft_amd/csrc/gd_matcheck.hpp"

#include <cstring>

extern "C" {

// the index of the first value that is not a depth, or -1
long long mc_first_bad(const float* v, size_t n)
{
    const size_t i = gdm::first_bad(v, n);
    return i == gdm::kNone ? -1 : (long long)i;
}

int mc_fits(size_t n_rows, size_t n_samples, size_t min_cols) { return gdm::fits(n_rows, n_samples, min_cols); }

// (addresses as integers: nothing is read)
int mc_overlap(size_t a, size_t na, size_t b, size_t nb)
{
    return gdm::overlap(reinterpret_cast<const void*>(a), na, reinterpret_cast<const void*>(b), nb);
}

// order [n_rows], slices [n_rows + 1] (the first chunks + 1 are written), chunk_of_row [n_rows]; *largest: rows of the largest
// chunk.  Returns the number of chunks.
size_t mc_chunks(const double* vals, size_t n_rows, double window, uint32_t* order, uint32_t* slices, uint32_t* chunk_of_row,
                 size_t* largest)
{
    const std::vector<uint32_t> o = gdm::argsort(vals, n_rows);
    const gdm::Chunks ch = gdm::chunk_walk(vals, o, window);
    memcpy(order, o.data(), n_rows * sizeof(uint32_t));
    memcpy(slices, ch.slices.data(), ch.slices.size() * sizeof(uint32_t));
    memcpy(chunk_of_row, ch.chunk_of_row.data(), n_rows * sizeof(uint32_t));
    *largest = ch.largest;
    return ch.count();
}

}  // extern "C"
