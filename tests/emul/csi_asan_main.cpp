// csi_asan_main.cpp -- TEST INFRASTRUCTURE (tests/test_csi_ref.py): the .csi reader (goleft_amd/csrc/host/csi_reader.hpp)
// built with -fsanitize=address,undefined and run over every input of the file given ([u32 size, bytes] each): whole
// indexes as files and as payloads, payloads cut at and inside every field, counts that the bytes do not hold, damaged and
// truncated gzip bytes.  Each input is copied to a heap block of exactly its size, so that a read past it is seen.  One line
// per input: "<min_shift> <depth> <references> <anchors> <checksum of the anchors>" or "refused", then "ok".
#include "csi_reader.hpp"
#include <cstdio>
#include <memory>
int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    for (;;) {
        uint8_t h[4];
        if (fread(h, 1, 4, f) != 4) break;
        const size_t n = (size_t)h[0] | ((size_t)h[1] << 8) | ((size_t)h[2] << 16) | ((size_t)h[3] << 24);
        std::unique_ptr<uint8_t[]> d(new uint8_t[n ? n : 1]);
        if (n && fread(d.get(), 1, n, f) != n) return 2;
        std::unique_ptr<uint8_t[]> exact(new uint8_t[n]);                    // (n == 0: a block of no bytes)
        if (n) memcpy(exact.get(), d.get(), n);
        gdh::CsiIndex x; std::string why;
        if (!gdh::read_csi_bytes(exact.get(), n, &x, &why)) { printf("refused\n"); continue; }
        size_t count = 0; uint64_t sum = 0;
        for (const auto& v : x.anchors) {
            uint64_t s = 0;
            for (uint64_t a : v) s += a;
            count += v.size(); sum = (sum + s % 1000003) % 1000003;
        }
        printf("%d %d %zu %zu %llu\n", x.min_shift, x.depth, x.anchors.size(), count, (unsigned long long)sum);
    }
    fclose(f);
    printf("ok\n");
}
