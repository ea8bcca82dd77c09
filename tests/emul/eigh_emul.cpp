// eigh_emul.cpp -- goleft_amd/csrc/gd_eigh.hpp as a stand-alone program, for tests/test_eigh_host.py (plain C++: the header
// has no HIP in it).
//
//   eigh_emul IN OUT
//
// IN: any number of matrices, each an int64 N and N * N float64 values (symmetric, either major).  OUT gets, per matrix,
// an int64 status (gde::sym_eigen's), then N eigenvalues and N * N values, eigenvector c at [c * N], in the solver's order.
#include "../../goleft_amd/csrc/gd_eigh.hpp"

#include <cstdint>
#include <cstdio>

int main(int argc, char** argv)
{
    if (argc != 3) { fprintf(stderr, "usage: eigh_emul IN OUT\n"); return 2; }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) { fprintf(stderr, "eigh_emul: cannot open the files\n"); return 2; }
    int64_t n = 0;
    while (fread(&n, sizeof n, 1, in) == 1) {
        if (n < 1 || n > 4096) { fprintf(stderr, "eigh_emul: a matrix of %lld\n", (long long)n); return 2; }
        const size_t N = (size_t)n;
        std::vector<double> V(N * N), d;
        if (fread(V.data(), sizeof(double), N * N, in) != N * N) { fprintf(stderr, "eigh_emul: short matrix\n"); return 2; }
        const int64_t rc = gde::sym_eigen(N, V, d);
        if (fwrite(&rc, sizeof rc, 1, out) != 1 || fwrite(d.data(), sizeof(double), N, out) != N ||
            fwrite(V.data(), sizeof(double), N * N, out) != N * N) { fprintf(stderr, "eigh_emul: short write\n"); return 2; }
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 2;
}
