// samplename_host.cpp -- host twin of `goleft samplename` (goleft's samplename/samplename.go:39-68).
//
//   goleft-depth samplename [-e] a.bam
//
// The SM values of the header's @RG lines (Names, sample_names.hpp), joined by newlines; an empty line when there is
// none.  -e: anything but exactly one name is the reference's panic.  No device is opened.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../../include/goleft_depth_host.h"
#include "bam_reader.hpp"
#include "sample_names.hpp"

namespace {

void usage(FILE* f)
{
    fputs("usage: samplename [--errormulti] BAM\n"
          "  -e  return an error if there is not exactly 1 sample in the bam\n", f);
}

}  // namespace

extern "C" int gdh_samplename_main(int argc, const char* const* argv)
{
    bool error_multi = false;
    std::vector<std::string> bams;
    for (int i = 1; i < argc; ++i) {
        const std::string arg = argv[i];
        if (arg == "-h" || arg == "--help") { usage(stdout); return 0; }
        if (arg == "-e" || arg == "--errormulti") { error_multi = true; continue; }
        if (arg == "--") { for (++i; i < argc; ++i) bams.push_back(argv[i]); break; }
        if (arg.size() > 1 && arg[0] == '-') { fprintf(stderr, "error: unknown argument %s\n", arg.c_str()); usage(stderr); return 255; }
        bams.push_back(arg);
    }
    if (bams.empty()) { fprintf(stderr, "error: bam is required\n"); usage(stderr); return 255; }
    if (bams.size() > 1) { fprintf(stderr, "error: too many positional arguments at '%s'\n", bams[1].c_str()); usage(stderr); return 255; }
    const std::string& bam = bams[0];
    gdh::BamReader br;
    std::string err;
    if (!br.open(bam, 1, &err)) { fprintf(stderr, "samplename: %s: %s\n", bam.c_str(), err.c_str()); return 1; }
    std::string text = br.header_text();
    const size_t nul = text.find('\0');
    if (nul != std::string::npos) text.resize(nul);
    const std::vector<std::string> names = gdh::sample_name_list(text);
    if (error_multi && names.size() != 1) {
        fprintf(stderr, "panic: goleft/samplename: found multiple samples in %s\n", bam.c_str());   // :64-66; a Go panic exits 2
        return 2;
    }
    std::string o;
    for (size_t i = 0; i < names.size(); ++i) { if (i) o += '\n'; o += names[i]; }
    o += '\n';
    fwrite(o.data(), 1, o.size(), stdout);
    return fflush(stdout) == 0 ? 0 : 1;
}
