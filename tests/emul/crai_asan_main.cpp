// crai_asan_main.cpp -- TEST INFRASTRUCTURE (tests/test_crai_reader_asan.py): the .crai reader
// (goleft_amd/csrc/host/crai_reader.hpp) built with -fsanitize=address,undefined and run over every file given: the
// reference's fixture, written files with every kind of bad line, damaged and truncated gzip bytes.  One line per file:
// "<references> <slices> <sum of alnStart + alnSpan + sliceLen>" or "refused <line>", then "ok".
#include "crai_reader.hpp"
#include <cinttypes>
#include <cstdio>
int main(int argc, char** argv) {
    for (int a = 1; a < argc; ++a) {
        gdh::CraiSlices c; int64_t line = 0; std::string why;
        if (!gdh::read_crai(argv[a], &c, &line, &why)) { printf("refused %" PRId64 "\n", line); continue; }
        int64_t sum = 0;
        for (size_t i = 0; i < c.start.size(); ++i) sum += c.start[i] + c.span[i] + c.len[i];
        printf("%zu %zu %" PRId64 "\n", c.ref_off.size() - 1, c.start.size(), sum);
    }
    printf("ok\n");
}
