// index_build.hpp -- a BAM's .bai made on the device, in memory (host/index_host.cpp): what `goleft-depth index` writes and
// what `goleft depth` parses when GOLEFT_GPU_INDEX=1 meets a BAM without an index.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "../../../include/goleft_depth.h"

namespace gdh {

struct IndexStats { int64_t records = 0; int rounds = 0, ranges = 0; };

// The index of `bam` on the context's device -> its bytes.  GD_OK, or the status with the message in *err; nothing is pending
// on the context afterwards either way.
int build_bai(gd_ctx* ctx, const std::string& bam, std::vector<uint8_t>* out, std::string* err, IndexStats* stats = nullptr);

}  // namespace gdh
