// indexsplit_host.cpp -- host twin of `goleft indexsplit` (goleft's indexsplit/indexsplit.go).
//
//   goleft-depth indexsplit -n N [--fai ref.fai] [-p problematic.bed] a.bam b.bam ... | a.bai ... | a.crai ...
//
// N regions that hold about the same amount of data across a cohort, from the .bai linear indexes -- or the .crai slices,
// tiled on the device (gd_crai_sizes) -- alone: the tile sizes of every index are summed cell by
// cell on the device (gd_indexsplit_*, float64, the samples in argument
// order); chop, getPercents and the walk over the tiles carry state from cell to cell and run here, in plain
// sequential float64 (this library is built without fused multiply-adds).  Rows: chrom, start, end, %.2f sum, splits.
#include <algorithm>
#include <atomic>
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../../../include/goleft_depth.h"
#include "../../../include/goleft_depth_host.h"
#include "bam_reader.hpp"
#include "cli.hpp"
#include "index_sizes.hpp"

namespace {

using gdh::ends_with;

constexpr int kThreads = 8;                      // index readers, as indexcov's; never sized by the machine
constexpr int64_t kTile = 16384;                 // indexcov.TileWidth
constexpr size_t kBatch = 256;                   // samples of one gd_indexsplit_add: the device holds one batch at a time

struct SArgs {
    int64_t n = 0;
    bool has_n = false;
    std::string fai, problematic;
    std::vector<std::string> inputs;
};

void usage(FILE* f)
{
    fputs("usage: indexsplit --n N [--fai FAI] [--problematic PROBLEMATIC] INDEXES [INDEXES ...]\n"
          "  -n  number of regions to split to (at least 1)\n"
          "  --fai  fasta index file, required when the first input is a bare .bai or a .crai\n"
          "  -p  BED file of regions to split small (one path; it is not split at '|')\n"
          "  inputs: .bam files (index x.bam.bai, else x.bai), .bai files or .crai files, in any mix; for a .cram pass its\n"
          "          .crai.\n", f);
}

int parse_args(int argc, const char* const* argv, SArgs* a)
{
    using gdh::cli::Args;
    Args c(argc, argv, usage);
    for (;;) {
        const Args::Kind kind = c.next();
        if (kind == Args::End) break;
        if (kind == Args::Help) return 1;
        if (kind == Args::Positional) { a->inputs.push_back(c.arg); continue; }
        std::string* const text = c.key == "--fai" ? &a->fai : c.key == "-p" || c.key == "--problematic" ? &a->problematic : nullptr;
        if (!text && c.key != "-n" && c.key != "--n") return c.fail("unknown argument %s", c.arg.c_str());
        if (!c.value()) return -1;
        if (text) { *text = c.val; continue; }
        char* end = nullptr;
        const long long v = strtoll(c.val.c_str(), &end, 10);
        if (c.val.empty() || *end || v < 1 || v > INT32_MAX)
            return c.fail("%s %s: the number of regions is an integer from 1 to 2147483647", c.key.c_str(), c.val.c_str());
        a->n = v; a->has_n = true;
    }
    if (!a->has_n) return c.fail("--n is required");
    if (a->inputs.empty()) return c.fail("indexes is required");
    return 0;
}

using gdh::cli::now_s;

struct Sample : gdh::IndexSizes { std::string err; };

// chop (:38-49): cells above mean + 3 sd of their reference become 8 x mean.  gonum's stat.MeanStdDev restated (DESIGN.md
// section 5): the mean is the sequential sum over n, the variance the corrected two-pass form.
void chop(double* x, size_t n)
{
    double sum = 0;
    for (size_t i = 0; i < n; ++i) sum += x[i];
    const double m = sum / (double)n;
    double ss = 0, c = 0;
    for (size_t i = 0; i < n; ++i) { const double d = x[i] - m; ss += d * d; c += d; }
    const double var = (ss - c * c / (double)n) / (double)(n - 1);     // (n == 1: 0 / 0, nothing compares above NaN)
    const double mx = m + 3 * std::sqrt(var);
    for (size_t i = 0; i < n; ++i)
        if (x[i] > mx) x[i] = 8 * m;
}

void put_row(std::string* o, const std::string& chrom, int64_t start, int64_t end, double sum, int splits)
{
    char buf[96];
    snprintf(buf, sizeof buf, "\t%" PRId64 "\t%" PRId64 "\t%.2f\t%d\n", start, end, sum, splits);
    *o += chrom;
    *o += buf;
}

#define IS_CHECK(call)                                                                                  \
    do {                                                                                                \
        const int rc_ = (call);                                                                         \
        if (rc_ != GD_OK) {                                                                             \
            fprintf(stderr, "indexsplit: %s: %s (%s)\n", #call, gd_strerror(rc_), gd_last_error(ctx));  \
            return 1;                                                                                   \
        }                                                                                               \
    } while (0)

int run(const SArgs& a, FILE* out)
{
    const bool timing = getenv("GOLEFT_INDEXSPLIT_TIMING") != nullptr;
    const double t_start = now_s();
    for (const std::string& b : a.inputs)
        if (ends_with(b, ".cram")) {
            fprintf(stderr, "indexsplit: %s: CRAM alignment files are not read: pass the .crai index instead\n", b.c_str());
            return 1;
        }
    gdh_intervals* probs = nullptr;
    struct Free { gdh_intervals*& p; ~Free() { gdh_intervals_free(p); } } free_probs{probs};
    if (!a.problematic.empty() && gdh_intervals_read_lines(a.problematic.c_str(), &probs) != 0) {
        fprintf(stderr, "indexsplit: %s: cannot read the problematic regions (a BED file)\n", a.problematic.c_str());
        return 1;
    }
    // Main (:207-212): the references of the first argument as given
    std::vector<gdh::FaiRef> refs;
    {
        const std::string& first = a.inputs[0];
        std::string err;
        if (ends_with(first, ".bam")) {
            gdh::BamReader br;
            if (!br.open(first, 1, &err)) { fprintf(stderr, "indexsplit: %s: %s\n", first.c_str(), err.c_str()); return 1; }
            for (const auto& c : br.contigs()) refs.push_back(gdh::FaiRef{c.name, c.length});
        } else if (!a.fai.empty()) {
            if (!gdh::read_fai(a.fai, &refs)) { fprintf(stderr, "indexsplit: error opening fai: %s\n", a.fai.c_str()); return 1; }
        } else {
            fprintf(stderr, "indexsplit: %s: since no .fai was specified (--fai), expected the first input to be a bam\n", first.c_str());
            return 1;
        }
    }
    if (refs.empty()) { fprintf(stderr, "indexsplit: %s has no references\n", a.inputs[0].c_str()); return 1; }
    const size_t N = a.inputs.size(), R = refs.size();
    std::vector<Sample> smp(N);
    {
        std::atomic<size_t> next{0};
        auto work = [&] { for (;;) { const size_t i = next.fetch_add(1); if (i >= N) break; gdh::read_index_sizes(a.inputs[i], &smp[i], &smp[i].err); } };
        std::vector<std::thread> th;
        for (int t = 1; t < kThreads && (size_t)t < N; ++t) th.emplace_back(work);
        work();
        for (auto& t : th) t.join();
    }
    for (const Sample& s : smp)
        if (!s.err.empty()) { fprintf(stderr, "indexsplit: %s\n", s.err.c_str()); return 1; }
    const double t_read = now_s() - t_start;
    gdh::cli::Device ctx;
    if (!ctx.open("indexsplit")) return 1;
    double t_crai_read = 0, t_crai_tile = 0;
    {
        // the slices of the .crai indexes become tile sizes: one device call for all of them
        std::vector<gdh::IndexSizes*> all(N);
        for (size_t s = 0; s < N; ++s) { all[s] = &smp[s]; t_crai_read += smp[s].crai_read_s; }
        std::string err;
        if (!gdh::tile_crai_indexes(ctx, all, a.inputs, &err, &t_crai_tile)) {
            fprintf(stderr, "indexsplit: %s\n", err.c_str());
            return 1;
        }
    }
    // Split (:92-114): reference i of the list is reference i of every index; an index with fewer has nothing there
    auto count = [&](const Sample& s, size_t r) -> int64_t { return r + 1 < s.ref_off.size() ? s.ref_off[r + 1] - s.ref_off[r] : 0; };
    std::vector<int32_t> longest(R, 0);
    std::vector<int64_t> cell_off(R + 1, 0);
    for (size_t r = 0; r < R; ++r) {
        for (const Sample& s : smp) longest[r] = (int32_t)std::max<int64_t>(longest[r], count(s, r));
        cell_off[r + 1] = cell_off[r] + longest[r];
    }
    IS_CHECK(gd_indexsplit_begin(ctx, (int32_t)R, longest.data()));
    for (size_t s0 = 0; s0 < N; s0 += kBatch) {
        const size_t nb = std::min(kBatch, N - s0);
        std::vector<int64_t> sample_off(nb + 1, 0), tile_off(nb * R);
        std::vector<int32_t> tile_cnt(nb * R);
        for (size_t k = 0; k < nb; ++k) sample_off[k + 1] = sample_off[k] + (int64_t)smp[s0 + k].sizes.size();
        std::vector<int64_t> sizes((size_t)sample_off[nb]);
        for (size_t k = 0; k < nb; ++k) {
            Sample& s = smp[s0 + k];
            std::copy(s.sizes.begin(), s.sizes.end(), sizes.begin() + sample_off[k]);
            for (size_t r = 0; r < R; ++r) {
                const int64_t n = count(s, r);
                tile_off[k * R + r] = sample_off[k] + (n ? s.ref_off[r] : 0);
                tile_cnt[k * R + r] = (int32_t)n;
            }
            std::vector<int64_t>().swap(s.sizes);
            std::vector<std::vector<uint64_t>>().swap(s.raw);
        }
        IS_CHECK(gd_indexsplit_add(ctx, (int32_t)nb, sample_off.data(), sizes.data(), tile_off.data(), tile_cnt.data()));
    }
    std::vector<double> cells((size_t)cell_off[R]);
    IS_CHECK(gd_indexsplit_sums(ctx, cells.data(), cells.size()));
    double lib[3] = {0, 0, 0};
    (void)gd_indexsplit_timing(ctx, lib, 3);
    ctx.reset();
    const double t_scan0 = now_s();
    // getPercents (:52-66); floats.Sum is the sequential loop of gonum's portable build
    std::vector<double> sums(R, 0.0);
    double tot = 0;
    for (size_t r = 0; r < R; ++r) {
        double* x = cells.data() + cell_off[r];
        const size_t n = (size_t)longest[r];
        if (n) chop(x, n);
        double s = 0;
        for (size_t i = 0; i < n; ++i) s += x[i];
        sums[r] = s;
        tot += s;
    }
    if (!(tot > 0)) {
        // (the reference goes on with int(NaN * N), which Go leaves to the platform)
        fprintf(stderr, "indexsplit: the indexes hold no data on any of the %zu references (the first input is %s)\n", R, a.inputs[0].c_str());
        return 1;
    }
    std::string o;
    const double fN = (double)a.n;
    for (size_t ri = 0; ri < R; ++ri) {
        const gdh::FaiRef& ref = refs[ri];
        const int64_t len = longest[ri];
        if (len == 0) { put_row(&o, ref.name, 0, ref.length, 0, 0); continue; }
        const double pct = sums[ri] / tot;
        int64_t n = (int64_t)(pct * fN);
        if (n == 0 && pct > 0) n = 1;
        else if (n == 0) { put_row(&o, ref.name, 0, ref.length, 0, 0); continue; }
        const double chunk = sums[ri] / (double)n;
        const double* size = cells.data() + cell_off[ri];
        double sum = 0;
        int64_t lasti = 0;
        // the walk (:145-188): a region is written as soon as it holds chunk
        for (int64_t i = 0; i < len; ++i) {
            const bool ovl = gdh_intervals_overlaps(probs, ref.name.c_str(), i * kTile, (i + 1) * kTile) != 0;
            if (size[i] > chunk || (size[i] >= 0.05 * chunk && ovl)) {
                if (i > lasti) put_row(&o, ref.name, lasti * kTile, i * kTile, sum, 1);
                sum = size[i];
                int nsplits = (int)std::min<int64_t>((int64_t)(0.5 + (sum / (chunk / 2))), 9);   // (above 8 is 8)
                if (nsplits > 8) {
                    nsplits = 8;
                } else if (nsplits < 1) {
                    nsplits = 1;
                    if (ovl) nsplits = 3;
                }
                int64_t start = i * kTile;
                const int64_t l = (int64_t)((double)kTile / (double)nsplits + 1);
                for (int k = 0; k < nsplits; ++k) {
                    if (i + k == len + 1) put_row(&o, ref.name, start, ref.length, sum / (double)nsplits, nsplits);
                    else put_row(&o, ref.name, start, std::min(start + l, (i + 1) * kTile), sum / (double)nsplits, nsplits);
                    start += l;
                }
                lasti = i + 1; sum = 0;
                continue;
            }
            sum += size[i];
            if (sum >= chunk || i == len - 1 || (sum >= 0.2 * chunk && ovl)) {
                if (i == len - 1) put_row(&o, ref.name, lasti * kTile, ref.length, sum, 1);
                else put_row(&o, ref.name, lasti * kTile, (i + 1) * kTile, sum, 1);
                lasti = i + 1;
                sum = 0;
            }
        }
    }
    const double t_scan = now_s() - t_scan0;
    if (fwrite(o.data(), 1, o.size(), out) != o.size() || fflush(out) != 0) { fprintf(stderr, "indexsplit: error writing the regions\n"); return 1; }
    if (timing)
        fprintf(stderr, "{\"samples\": %zu, \"references\": %zu, \"cells\": %" PRId64 ", \"total_s\": %.4f, \"index_read_s\": %.4f, "
                        "\"crai_read_s\": %.4f, \"crai_tile_s\": %.4f, \"upload_s\": %.4f, \"kernel_s\": %.4f, \"readback_s\": %.4f, \"scan_s\": %.4f}\n",
                N, R, cell_off[R], now_s() - t_start, t_read, t_crai_read, t_crai_tile, lib[0], lib[1], lib[2], t_scan);
    return 0;
}

}  // namespace

extern "C" int gdh_indexsplit_run(int argc, const char* const* argv, const char* out_path)
{
    SArgs a;
    const int p = parse_args(argc, argv, &a);
    if (p > 0) return 0;
    if (p < 0) return 255;
    return gdh::cli::run_to_output("indexsplit", out_path, [&](FILE* out) { return run(a, out); });
}

extern "C" int gdh_indexsplit_main(int argc, const char* const* argv) { return gdh_indexsplit_run(argc, argv, nullptr); }
