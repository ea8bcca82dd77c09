// index_build.hpp -- a BAM's .bai or .csi made on the device, in memory (host/index_host.cpp): what `goleft-depth index`
// writes and what `goleft depth` parses when GOLEFT_GPU_INDEX=1 meets a BAM without an index.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "../../../include/goleft_depth.h"

namespace gdh {

struct IndexStats { int64_t records = 0; int rounds = 0, ranges = 0, min_shift = 14, depth = 5; };
enum class IndexFormat { Bai, Csi };

// The depth of a .csi for these reference lengths: the smallest d with longest + 256 <= 2^(min_shift + 3 d).
int csi_depth(const std::vector<int64_t>& lengths, int min_shift);

// The index of `bam` on the context's device -> its bytes.  GD_OK, or the status with the message in *err; nothing is pending
// on the context afterwards either way.
int build_bai(gd_ctx* ctx, const std::string& bam, std::vector<uint8_t>* out, std::string* err, IndexStats* stats = nullptr);
// ... in either format: Bai is build_bai (min_shift is not consulted); Csi gives the file's bytes, BGZF, with min_shift (8 to
// 24) and the depth csi_depth gives.
int build_index(gd_ctx* ctx, const std::string& bam, IndexFormat format, int min_shift, std::vector<uint8_t>* out, std::string* err,
                IndexStats* stats = nullptr);

}  // namespace gdh
