// indexcov_host.cpp -- host twin of `goleft indexcov` (goleft's indexcov/indexcov.go, types.go).
//
//   goleft-depth indexcov -d DIR [-X X,Y] [-p REGEX] [-e] [-n] [-f ref.fai] a.bam b.bam ... | a.bai ... | a.crai ...
//
// Coverage of a cohort from the .bai linear indexes -- or the .crai slices, tiled on the device (gd_crai_sizes; DESIGN.md
// section 3.9) -- alone: DIR/<DIR>-indexcov.bed.gz (one row per 16 384-base tile, one %.3g column per sample), .roc (coverage ROC per reference) and .ped (inferred sex, copy number of the sex references,
// bin counts, slopes, five principal components).  The host reads the indexes (eight reader threads), runs the
// reference's sequential -n pass, solves the N x N eigenproblem and writes text and BGZF; medians, depths, cells, slots,
// counters, copy numbers, the pca8 bytes and their exact Gram matrix come from the device (gd_indexcov_*).
// No HTML, PNG or chart output (plot.go, template.go): out of scope.
#include <glob.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

#include <algorithm>
#include <atomic>
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <regex>
#include <string>
#include <thread>
#include <vector>

#include "../../../include/goleft_depth.h"
#include "../../../include/goleft_depth_host.h"
#include "../gd_eigh.hpp"
#include "../gd_round3g.hpp"
#include "bam_reader.hpp"
#include "cli.hpp"
#include "index_sizes.hpp"

namespace {

const char* const kDefaultExclude = "^chrEBV$|^NC|_random$|Un_|^HLA\\-|_alt$|hap\\d$";
constexpr int kSlots = 70;
constexpr int kThreads = 8;                      // the reference's eight index readers (:417-429); never sized by the machine

struct IArgs {
    std::string dir, sex = "X,Y", exclude = kDefaultExclude, fai;
    bool include_gl = false, extra_norm = false;
    std::vector<std::string> inputs;
};

void usage(FILE* f)
{
    fputs("usage: indexcov --directory DIRECTORY [--includegl] [--excludepatt EXCLUDEPATT] [--sex SEX] [--fai FAI]\n"
          "                [--extranormalize] BAM [BAM ...]\n"
          "  -d  directory for output files: DIR/<DIR>-indexcov.bed.gz, .roc and .ped\n"
          "  -e  accepted (it selects plotted chromosomes; GL* references then also weigh into the slope)\n"
          "  -p  regular expression of chromosome names to exclude (ECMAScript syntax; the reference uses RE2)\n"
          "  -X  comma delimited names of the sex chromosome(s), '' if there are none (default X,Y)\n"
          "  -f  fasta index file, required when the first input is a bare .bai or a .crai\n"
          "  -n  normalize across samples and smooth within a sample\n"
          "  inputs: .bam files (index x.bam.bai, else x.bai), .bai files or .crai files, in any mix; for a .cram pass its\n"
          "          .crai; -c/--chrom is refused.\n"
          "  No HTML, PNG or chart output is written (index.html, *-roc-*.html, *.png of the reference are out of scope).\n", f);
}

using gdh::ends_with;

int parse_args(int argc, const char* const* argv, IArgs* a)
{
    using gdh::cli::Args;
    Args c(argc, argv, usage);
    for (;;) {
        const Args::Kind kind = c.next();
        if (kind == Args::End) break;
        if (kind == Args::Help) return 1;
        if (kind == Args::Positional) { a->inputs.push_back(c.arg); continue; }
        const std::string& key = c.key;
        if (key == "-e" || key == "--includegl") { a->include_gl = true; continue; }
        if (key == "-n" || key == "--extranormalize") { a->extra_norm = true; continue; }
        const bool chrom = key == "-c" || key == "--chrom";
        std::string* const text = key == "-d" || key == "--directory" ? &a->dir : key == "-p" || key == "--excludepatt" ? &a->exclude
                                : key == "-X" || key == "--sex" ? &a->sex : key == "-f" || key == "--fai" ? &a->fai : nullptr;
        if (!text && !chrom) return c.fail("unknown argument %s", c.arg.c_str());
        if (!c.value()) return -1;
        if (chrom) {
            fprintf(stderr, "indexcov: %s %s is not supported: the reference appends the chosen chromosome to the full list "
                            "instead of filtering by it\n", key.c_str(), c.val.c_str());
            return -2;
        }
        *text = c.val;
    }
    if (a->dir.empty()) return c.fail("--directory is required");
    if (a->inputs.empty()) return c.fail("bam is required");
    return 0;
}

using gdh::cli::now_s;

bool mkdir_p(const std::string& path)
{
    struct stat st;
    if (stat(path.c_str(), &st) == 0) return S_ISDIR(st.st_mode);
    for (size_t p = 1; p <= path.size(); ++p)
        if (p == path.size() || path[p] == '/') {
            const std::string part = path.substr(0, p);
            if (mkdir(part.c_str(), 0755) != 0 && errno != EEXIST) return false;
        }
    return true;
}

// filepath.Base
std::string base_name(std::string p)
{
    while (p.size() > 1 && p.back() == '/') p.pop_back();
    const size_t s = p.find_last_of('/');
    if (s != std::string::npos && p.size() > 1) p = p.substr(s + 1);
    return p.empty() ? "." : p;
}

using Ref = gdh::FaiRef;
using gdh::read_fai;

struct Sample : gdh::IndexSizes {
    std::string path, name, err;
};

// readIndex (:471-525) + getSizes (types.go:45-82)
void read_sample(Sample* s)
{
    const std::string& b = s->path;
    std::string err;
    if (!gdh::read_index_sizes(b, s, &s->err)) return;
    if (ends_with(b, ".bai") || ends_with(b, ".crai")) {
        gdh::short_name(b, "", &s->name);
    } else {
        gdh::BamReader br;
        if (!br.open(b, 1, &err)) { s->err = b + ": " + err; return; }
        if (!gdh::short_name(b, br.header_text(), &s->name)) { s->err = "bam reagroup: more than one RG for " + b; return; }
    }
}

bool same_chrom(const std::vector<std::string>& as, const std::string& b)       // :530-547
{
    for (const std::string& a : as) {
        if (a == b) return true;
        std::string na = a;
        if (a.compare(0, 3, "chr") == 0) na = a.substr(3);
        else if (b.compare(0, 3, "chr") == 0) na = "chr" + a;
        if (na == b) return true;
    }
    return false;
}

// fmt's %.Nf of a float64, NaN and the infinities as Go prints them
void put_f(std::string* o, const char* fmt, double v)
{
    if (std::isnan(v)) { *o += "NaN"; return; }
    if (std::isinf(v)) { *o += v > 0 ? "+Inf" : "-Inf"; return; }
    char buf[64];
    snprintf(buf, sizeof buf, fmt, v);
    *o += buf;
}

// normalizeAcrossSamples (:549-597): sequential in the tile index, in the reference's order.  d[k] / len[k]: the
// depths of sample k on this reference.
void normalize_across(std::vector<float*>& d, const std::vector<int>& len)
{
    const size_t N = d.size();
    if (N < 5) return;
    int max_len = 0;
    for (int l : len) max_len = std::max(max_len, l);
    for (int j = 0; j < max_len; ++j) {
        double m = 0, n = 0;
        for (size_t i = 0; i < N; ++i)
            if (len[i] > j) {
                m += (double)d[i][j]; n += 1;
                if (j > 0) { m += (double)d[i][j - 1]; n += 1; }
                if (j < len[i] - 1) { m += (double)d[i][j + 1]; n += 1; }
            }
        if ((int)n < 3 * (int)N - 4) continue;
        m /= n;
        if (m < 0.1) continue;
        const float fm = (float)m;
        for (size_t i = 0; i < N; ++i)
            if (len[i] > j) {
                float* x = d[i];
                x[j] /= fm;
                if (j > 2 && j < len[i] - 3) {
                    float t = x[j - 3] + x[j - 2];
                    t = t + x[j - 1];
                    t = t + x[j];
                    t = t + x[j + 1] / fm;
                    t = t + x[j + 2] / fm;
                    t = t + x[j + 3] / fm;
                    x[j] = (float)(1.0 / 7.0) * t;
                }
            }
    }
}

// ---- BGZF (level 1, mtime 0, OS 0xff as the reference sets) -----------------------------------------------------
bool bgzf_block(const uint8_t* src, size_t n, std::vector<uint8_t>* out)
{
    z_stream zs{};
    if (deflateInit2(&zs, 1, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) != Z_OK) return false;
    std::vector<uint8_t> buf(deflateBound(&zs, (uLong)n) + 64);
    zs.next_in = const_cast<Bytef*>(src); zs.avail_in = (uInt)n;
    zs.next_out = buf.data(); zs.avail_out = (uInt)buf.size();
    const int rc = deflate(&zs, Z_FINISH);
    const size_t clen = zs.total_out;
    deflateEnd(&zs);
    if (rc != Z_STREAM_END || clen + 26 > 65536) return false;
    const uint8_t hdr[18] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0,
                             (uint8_t)((clen + 25) & 0xff), (uint8_t)((clen + 25) >> 8)};
    out->insert(out->end(), hdr, hdr + 18);
    out->insert(out->end(), buf.data(), buf.data() + clen);
    const uint32_t crc = (uint32_t)crc32(crc32(0, nullptr, 0), src, (uInt)n), isz = (uint32_t)n;
    for (int k = 0; k < 4; ++k) out->push_back((uint8_t)(crc >> (8 * k)));
    for (int k = 0; k < 4; ++k) out->push_back((uint8_t)(isz >> (8 * k)));
    return true;
}

// Compresses text as BGZF members of at most 0xff00 bytes on kThreads threads and appends them to f.
bool bgzf_write(FILE* f, const std::string& text)
{
    const size_t blk = 0xff00, nb = (text.size() + blk - 1) / blk;
    std::vector<std::vector<uint8_t>> parts(nb);
    std::atomic<size_t> next{0};
    std::atomic<bool> ok{true};
    auto work = [&] {
        for (;;) {
            const size_t i = next.fetch_add(1);
            if (i >= nb) break;
            const size_t a = i * blk, n = std::min(blk, text.size() - a);
            if (!bgzf_block(reinterpret_cast<const uint8_t*>(text.data()) + a, n, &parts[i])) ok.store(false);
        }
    };
    std::vector<std::thread> th;
    for (int t = 1; t < kThreads && (size_t)t < nb; ++t) th.emplace_back(work);
    work();
    for (auto& t : th) t.join();
    if (!ok.load()) return false;
    for (const auto& p : parts)
        if (fwrite(p.data(), 1, p.size(), f) != p.size()) return false;
    return true;
}

const uint8_t kBgzfEof[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};

#define IC_CHECK(call)                                                                                \
    do {                                                                                              \
        const int rc_ = (call);                                                                       \
        if (rc_ != GD_OK) {                                                                           \
            fprintf(stderr, "indexcov: %s: %s (%s)\n", #call, gd_strerror(rc_), gd_last_error(ctx));  \
            return 1;                                                                                 \
        }                                                                                             \
    } while (0)

int run(const IArgs& a)
{
    const bool timing = getenv("GOLEFT_INDEXCOV_TIMING") != nullptr;
    double t_read = 0, t_norm = 0, t_eig = 0, t_text = 0, t_bgzf = 0, t_back = 0;
    const double t_start = now_s();
    for (const std::string& b : a.inputs) {
        if (ends_with(b, ".cram")) {
            fprintf(stderr, "indexcov: %s: CRAM alignment files are not read: pass the .crai index instead\n", b.c_str());
            return 1;
        }
        // (expandGlobs below drops what matches nothing; a .crai that is not there is named instead)
        if (ends_with(b, ".crai") && b.find_first_of("*?[") == std::string::npos && access(b.c_str(), F_OK) != 0) {
            fprintf(stderr, "indexcov: %s: no such .crai index\n", b.c_str());
            return 1;
        }
    }
    std::vector<std::string> sex;
    if (!a.sex.empty()) {                                                      // strings.Split(strings.TrimSpace(Sex), ",")
        std::string t = a.sex;
        while (!t.empty() && isspace((unsigned char)t.back())) t.pop_back();
        while (!t.empty() && isspace((unsigned char)t.front())) t.erase(t.begin());
        size_t p = 0;
        for (;;) {
            const size_t q = t.find(',', p);
            sex.push_back(t.substr(p, q == std::string::npos ? std::string::npos : q - p));
            if (q == std::string::npos) break;
            p = q + 1;
        }
    }
    std::regex exclude;
    const bool has_exclude = !a.exclude.empty();
    if (has_exclude) {
        try { exclude = std::regex(a.exclude, std::regex::ECMAScript); }
        catch (const std::regex_error&) { fprintf(stderr, "indexcov: bad exclude pattern %s\n", a.exclude.c_str()); return 1; }
    }
    if (!mkdir_p(a.dir)) { fprintf(stderr, "indexcov: error creating specified directory: %s\n", a.dir.c_str()); return 1; }
    // getReferences (:344-374): the first argument as given
    std::vector<Ref> refs;
    {
        const std::string& first = a.inputs[0];
        std::string err;
        if (ends_with(first, ".bam")) {
            gdh::BamReader br;
            if (!br.open(first, 1, &err)) { fprintf(stderr, "indexcov: %s: %s\n", first.c_str(), err.c_str()); return 1; }
            for (const auto& c : br.contigs()) refs.push_back(Ref{c.name, c.length});
        } else if (!a.fai.empty()) {
            if (!read_fai(a.fai, &refs)) { fprintf(stderr, "indexcov: error opening fai: %s\n", a.fai.c_str()); return 1; }
        } else {
            fprintf(stderr, "indexcov: %s: since no .fai was specified (-f), expected input to be a list of bams\n", first.c_str());
            return 1;
        }
    }
    // expandGlobs (:376-389)
    std::vector<std::string> paths;
    for (const std::string& p : a.inputs) {
        glob_t g{};
        if (glob(p.c_str(), 0, nullptr, &g) == 0)
            for (size_t i = 0; i < g.gl_pathc; ++i) paths.push_back(g.gl_pathv[i]);
        globfree(&g);
    }
    if (paths.empty()) { fprintf(stderr, "indexcov: expected at least 1 bam/bai: none of the inputs exists (%s)\n", a.inputs[0].c_str()); return 1; }
    if (paths.size() > 65535) { fprintf(stderr, "indexcov: at most 65535 samples\n"); return 1; }
    const size_t N = paths.size();
    std::vector<Sample> smp(N);
    {
        std::atomic<size_t> next{0};
        auto work = [&] { for (;;) { const size_t i = next.fetch_add(1); if (i >= N) break; smp[i].path = paths[i]; read_sample(&smp[i]); } };
        std::vector<std::thread> th;
        for (int t = 1; t < kThreads && (size_t)t < N; ++t) th.emplace_back(work);
        work();
        for (auto& t : th) t.join();
    }
    for (const Sample& s : smp)
        if (!s.err.empty()) { fprintf(stderr, "indexcov: %s\n", s.err.c_str()); return 1; }
    t_read = now_s() - t_start;
    gdh::cli::Device ctx;                        // opened where the first device call is
    auto open_device = [&]() -> bool { return ctx || ctx.open("indexcov"); };
    double t_crai_read = 0, t_crai_tile = 0;
    {
        // the slices of the .crai indexes become tile sizes: one device call for all of them
        std::vector<gdh::IndexSizes*> all(N);
        bool any = false;
        for (size_t s = 0; s < N; ++s) { all[s] = &smp[s]; any = any || smp[s].is_crai; t_crai_read += smp[s].crai_read_s; }
        if (any) {
            if (!open_device()) return 1;
            std::string err;
            if (!gdh::tile_crai_indexes(ctx, all, paths, &err, &t_crai_tile)) {
                fprintf(stderr, "indexcov: %s\n", err.c_str());
                return 1;
            }
        }
    }
    fprintf(stderr, "indexcov: running on %zu indexes\n", N);
    // the references that are reported
    std::vector<size_t> kept;
    for (size_t r = 0; r < refs.size(); ++r) {
        if (has_exclude && std::regex_search(refs[r].name, exclude)) continue;
        kept.push_back(r);
    }
    if (kept.empty()) { fprintf(stderr, "(FATAL) indexcov: every reference is excluded by %s\n", a.exclude.c_str()); return 1; }
    const size_t R = kept.size();
    std::vector<uint8_t> is_sex(R);
    for (size_t k = 0; k < R; ++k) is_sex[k] = same_chrom(sex, refs[kept[k]].name) ? 1 : 0;
    std::vector<int64_t> sample_off(N + 1, 0), tile_off(N * R);
    std::vector<int32_t> tile_cnt(N * R);
    for (size_t s = 0; s < N; ++s) sample_off[s + 1] = sample_off[s] + (int64_t)smp[s].sizes.size();
    std::vector<int64_t> sizes((size_t)sample_off[N]);
    for (size_t s = 0; s < N; ++s) {
        std::copy(smp[s].sizes.begin(), smp[s].sizes.end(), sizes.begin() + sample_off[s]);
        for (size_t k = 0; k < R; ++k) {
            const size_t r = kept[k];
            const bool has = r + 1 < smp[s].ref_off.size();
            tile_off[s * R + k] = sample_off[s] + (has ? smp[s].ref_off[r] : 0);
            tile_cnt[s * R + k] = has ? (int32_t)(smp[s].ref_off[r + 1] - smp[s].ref_off[r]) : 0;
        }
        std::vector<int64_t>().swap(smp[s].sizes);
        std::vector<std::vector<uint64_t>>().swap(smp[s].raw);
    }
    if (!open_device()) return 1;
    IC_CHECK(gd_indexcov_upload(ctx, (int32_t)N, (int32_t)R, sample_off.data(), sizes.data(), tile_off.data(), tile_cnt.data(), is_sex.data()));
    std::vector<int64_t>().swap(sizes);
    gd_indexcov_dims dims{};
    std::vector<int32_t> longest(R);
    std::vector<int64_t> cell_off(R), col_off(R), median(N);
    IC_CHECK(gd_indexcov_get_dims(ctx, &dims, longest.data(), cell_off.data(), col_off.data()));
    IC_CHECK(gd_indexcov_medians(ctx, median.data()));
    if (dims.m == 0) {                                                         // (the reference panics in mat.NewDense)
        fprintf(stderr, "(FATAL) indexcov: no reference that is not a sex chromosome is left: nothing for the principal components\n");
        return 1;
    }
    for (size_t s = 0; s < N; ++s)
        if (median[s] == 0)
            for (size_t k = 0; k < R; ++k) tile_cnt[s * R + k] = 0;            // (as the device library does)
    if (a.extra_norm) {
        const double t0 = now_s();
        std::vector<float> dep((size_t)dims.n_tiles);
        IC_CHECK(gd_indexcov_depths(ctx, dep.data(), dep.size()));
        for (size_t k = 0; k < R; ++k) {
            if (is_sex[k]) continue;
            std::vector<float*> d(N);
            std::vector<int> len(N);
            for (size_t s = 0; s < N; ++s) { d[s] = dep.data() + tile_off[s * R + k]; len[s] = tile_cnt[s * R + k]; }
            normalize_across(d, len);
        }
        IC_CHECK(gd_indexcov_set_depths(ctx, dep.data(), dep.size()));
        t_norm = now_s() - t0;
    }
    const int n_pc = (int)std::min<int64_t>(5, std::min<int64_t>((int64_t)N, dims.m));
    IC_CHECK(gd_indexcov_compute(ctx, n_pc >= 3 ? 1 : 0));
    double t0 = now_s();
    std::vector<int32_t> slots(R * N * kSlots);
    std::vector<int64_t> counters(N * 4);
    std::vector<double> cn(R * N);
    IC_CHECK(gd_indexcov_slots(ctx, slots.data()));
    IC_CHECK(gd_indexcov_counters(ctx, counters.data()));
    IC_CHECK(gd_indexcov_cn(ctx, cn.data()));
    std::vector<int64_t> G;
    if (n_pc >= 3) { G.resize(N * N); IC_CHECK(gd_indexcov_gram(ctx, G.data())); }
    t_back += now_s() - t0;

    std::vector<std::string> names(N);
    for (size_t s = 0; s < N; ++s) names[s] = smp[s].name;
    std::string joined;
    for (size_t s = 0; s < N; ++s) { if (s) joined += '\t'; joined += names[s]; }
    const std::string base = a.dir + "/" + base_name(a.dir) + "-indexcov";
    FILE* fb = fopen((base + ".bed.gz").c_str(), "wb");
    FILE* fr = fopen((base + ".roc").c_str(), "w");
    if (!fb || !fr) { fprintf(stderr, "indexcov: cannot create %s.bed.gz / .roc\n", base.c_str()); return 1; }
    bool io_ok = bgzf_write(fb, "#chrom\tstart\tend\t" + joined + "\n");
    std::map<std::string, std::vector<double>> sexes;
    std::vector<float> slopes(N, 0.f);
    int n_slopes = 0;
    std::vector<uint32_t> cells;
    const size_t rows_per_piece = std::max<size_t>(1, (64u << 20) / (N * 8 + 64));
    for (size_t k = 0; k < R && io_ok; ++k) {
        const Ref& ref = refs[kept[k]];
        const int L = longest[k];
        // the BED rows of this reference, a piece of rows at a time
        for (size_t row0 = 0; row0 < (size_t)L && io_ok; row0 += rows_per_piece) {
            const size_t nrows = std::min(rows_per_piece, (size_t)L - row0);
            t0 = now_s();
            cells.resize(nrows * N);
            IC_CHECK(gd_indexcov_cells(ctx, cell_off[k] + (int64_t)(row0 * N), (int64_t)(nrows * N), cells.data()));
            const double t1 = now_s();
            t_back += t1 - t0;
            std::vector<std::string> part((size_t)kThreads);
            auto work = [&](int t) {
                const size_t a0 = nrows * (size_t)t / kThreads, a1 = nrows * (size_t)(t + 1) / kThreads;
                std::string& o = part[(size_t)t];
                o.reserve((a1 - a0) * (N * 6 + ref.name.size() + 24));
                char buf[16];
                for (size_t i = a0; i < a1; ++i) {
                    o += ref.name;
                    o += '\t'; o += std::to_string((row0 + i) * 16384);
                    o += '\t'; o += std::to_string((row0 + i + 1) * 16384);
                    const uint32_t* c = cells.data() + i * N;
                    for (size_t s = 0; s < N; ++s) { o += '\t'; o.append(buf, (size_t)gd_fmt3g(c[s], buf)); }
                    o += '\n';
                }
            };
            std::vector<std::thread> th;
            for (int t = 1; t < kThreads; ++t) th.emplace_back(work, t);
            work(0);
            for (auto& t : th) t.join();
            std::string text;
            for (auto& p : part) text += p;
            const double t2 = now_s();
            t_text += t2 - t1;
            io_ok = bgzf_write(fb, text);
            t_bgzf += now_s() - t2;
        }
        if (is_sex[k] && L > 0) sexes[ref.name] = std::vector<double>(cn.begin() + k * N, cn.begin() + (k + 1) * N);
        if (L > 0) {
            // writeROCs (:1018-1036), CountsROC (:181-193)
            t0 = now_s();
            std::vector<std::vector<float>> rocs(N, std::vector<float>(kSlots));
            for (size_t s = 0; s < N; ++s) {
                const int32_t* cnt = slots.data() + (k * N + s) * kSlots;
                int64_t tot[kSlots];
                tot[kSlots - 1] = cnt[kSlots - 1];
                for (int i = kSlots - 2; i >= 0; --i) tot[i] = tot[i + 1] + cnt[i];
                const float mx = (float)tot[0];
                for (int i = 0; i < kSlots; ++i) rocs[s][(size_t)i] = (float)tot[i] / mx;
            }
            std::string o = "#chrom\tcov\t" + joined + "\n";
            for (int i = 0; i < kSlots; ++i) {
                o += ref.name; o += '\t';
                put_f(&o, "%.2f", (double)i / (70 * (2.0 / 3.0)));
                for (size_t s = 0; s < N; ++s) { o += '\t'; put_f(&o, "%.2f", (double)rocs[s][(size_t)i]); }
                o += '\n';
            }
            io_ok = io_ok && fwrite(o.data(), 1, o.size(), fr) == o.size();
            if ((a.include_gl || ref.name.compare(0, 2, "GL") != 0) && L > 2 && !is_sex[k] && L > 100) {
                const float scalar = (float)ref.length / 1e6f;                 // updateSlopes (:739-750): slots 40 and 54
                for (size_t s = 0; s < N; ++s) slopes[s] += (float)(rocs[s][40] - rocs[s][54]) * scalar;
                ++n_slopes;
            }
            t_text += now_s() - t0;
        }
    }
    io_ok = io_ok && fwrite(kBgzfEof, 1, sizeof kBgzfEof, fb) == sizeof kBgzfEof;
    io_ok = (fclose(fb) == 0) && io_ok;
    io_ok = (fclose(fr) == 0) && io_ok;
    if (!io_ok) { fprintf(stderr, "indexcov: error writing %s.bed.gz / .roc\n", base.c_str()); return 1; }
    for (float& s : slopes) s = s / (float)n_slopes;
    // checkSexes (:760-771)
    if (sexes.size() != sex.size()) {
        std::string keys;
        for (const auto& kv : sexes) { if (!keys.empty()) keys += ','; keys += kv.first; }
        const bool fatal = sexes.empty() && !(sex.size() == 2 && sex[0] == "X" && sex[1] == "Y");
        fprintf(stderr, "%s indexcov: expected %zu sex chromosomes, found: %zu.\nyou can set the expected with --sex '%s'\n",
                fatal ? "(FATAL)" : "(WARNING)", sex.size(), sexes.size(), keys.c_str());
        if (fatal) { return 1; }
    }
    if (sexes.empty()) fprintf(stderr, "sex chromosomes not found.\n");
    double lib[5] = {0, 0, 0, 0, 0};
    (void)gd_indexcov_timing(ctx, lib, 5);
    ctx.reset();
    // the principal components (pca :773-807) from the exact Gram matrix
    std::vector<double> pcs;
    if (n_pc >= 3) {
        t0 = now_s();
        pcs.resize(N * (size_t)n_pc);
        if (gdh_indexcov_pcs(G.data(), (int)N, n_pc, pcs.data(), nullptr) != 0) { fprintf(stderr, "indexcov: error with principal components\n"); return 1; }
        t_eig = now_s() - t0;
    } else {
        fprintf(stderr, "indexcov: %d principal components, not plotting\n", n_pc);
    }
    // writeIndex (:815-893): the .ped
    t0 = now_s();
    bool anygt = false;
    for (const Sample& s : smp) anygt = anygt || s.mapped > 0 || s.unmapped > 0;
    std::string o = "#family_id\tsample_id\tpaternal_id\tmaternal_id\tsex\tphenotype";
    for (const auto& kv : sexes) o += "\tCN" + kv.first;                       // (std::map: the keys sorted, as sort.Strings)
    o += "\tbins.out\tbins.lo\tbins.hi\tbins.in\tslope\tp.out";
    for (int c = 0; c < n_pc && n_pc >= 3; ++c) o += "\tPC" + std::to_string(c + 1);
    if (anygt) o += "\tmapped\tunmapped";
    o += '\n';
    for (size_t s = 0; s < N; ++s) {
        const int inferred = sexes.empty() ? -9 : (int)(0.5 + sexes.begin()->second[s]);
        o += "unknown\t" + names[s] + "\t-9\t-9\t" + std::to_string(inferred) + "\t-9";
        for (const auto& kv : sexes) { o += '\t'; put_f(&o, "%.2f", kv.second[s]); }
        const int64_t* c = counters.data() + s * 4;                            // out, low, hi, in
        o += '\t' + std::to_string(c[0]) + '\t' + std::to_string(c[1]) + '\t' + std::to_string(c[2]) + '\t' + std::to_string(c[3]);
        o += '\t'; put_f(&o, "%.3f", (double)slopes[s]);
        o += '\t'; put_f(&o, "%.2f", (double)c[0] / (double)c[3]);
        for (int k = 0; k < n_pc && n_pc >= 3; ++k) { o += '\t'; put_f(&o, "%.2f", pcs[s * (size_t)n_pc + (size_t)k]); }
        if (anygt) o += '\t' + std::to_string(smp[s].mapped) + '\t' + std::to_string(smp[s].unmapped);
        o += '\n';
    }
    FILE* fp = fopen((base + ".ped").c_str(), "w");
    if (!fp || fwrite(o.data(), 1, o.size(), fp) != o.size() || fclose(fp) != 0) {
        fprintf(stderr, "indexcov: cannot write %s.ped\n", base.c_str());
        return 1;
    }
    t_text += now_s() - t0;
    if (timing)
        fprintf(stderr, "{\"samples\": %zu, \"tiles\": %" PRId64 ", \"m\": %" PRId64 ", \"total_s\": %.4f, \"index_read_s\": %.4f, "
                        "\"crai_read_s\": %.4f, \"crai_tile_s\": %.4f, \"upload_s\": %.4f, \"median_depth_s\": %.4f, \"pass_s\": %.4f, \"cn_s\": %.4f, \"gram_s\": %.4f, "
                        "\"readback_s\": %.4f, \"normalize_s\": %.4f, \"eigen_s\": %.4f, \"text_s\": %.4f, \"bgzf_s\": %.4f}\n",
                N, dims.n_tiles, dims.m, now_s() - t_start, t_read, t_crai_read, t_crai_tile, lib[0], lib[1], lib[2], lib[3], lib[4], t_back, t_norm, t_eig,
                t_text, t_bgzf);
    fprintf(stderr, "indexcov finished: see %s.ped for overview of output\n", base.c_str());
    return 0;
}

}  // namespace

// The first k principal-component projections of the rows of X from G = X * X^T alone:
// C = G - g 1^T - 1 g^T + (1^T G 1 / N^2) 1 1^T with g = G 1 / N is the Gram matrix of the column-centred X; its
// eigenpairs (s_k^2, u_k) are the left singular pairs, and X v_k = (G - g 1^T) u_k / s_k.  fp64 throughout.
extern "C" int gdh_indexcov_pcs(const int64_t* G, int n, int k, double* out, double* sigma)
{
    if (!G || !out || n < 1 || k < 1 || k > n) return -1;
    const size_t N = (size_t)n;
    std::vector<double> g(N, 0.0);
    long double all = 0;
    for (size_t i = 0; i < N; ++i) {
        long double t = 0;
        for (size_t j = 0; j < N; ++j) t += (long double)G[i * N + j];
        all += t;
        g[i] = (double)(t / (long double)n);
    }
    const double mean = (double)(all / ((long double)n * (long double)n));
    // gd_eigh.hpp's solver: V is column-major, eigenvector c ends up at &V[c * N]
    std::vector<double> V(N * N), d(N);
#define VV(r, c) V[(size_t)(c) * N + (size_t)(r)]
    for (size_t i = 0; i < N; ++i)
        for (size_t j = 0; j <= i; ++j) {
            const double x = ((double)G[i * N + j] - g[i]) - g[j] + mean, y = ((double)G[j * N + i] - g[j]) - g[i] + mean;
            VV(i, j) = VV(j, i) = 0.5 * (x + y);                               // (exactly symmetric)
        }
#undef VV
    if (gde::sym_eigen(N, V, d) != 0) return -2;
    std::vector<size_t> order(N);
    for (size_t i = 0; i < N; ++i) order[i] = i;
    std::sort(order.begin(), order.end(), [&](size_t x, size_t y) { return d[x] > d[y]; });
    const double top = std::sqrt(std::max(0.0, d[order[0]]));
    for (int c = 0; c < k; ++c) {
        const size_t e = order[(size_t)c];
        const double sg = std::sqrt(std::max(0.0, d[e]));
        if (sigma) sigma[c] = sg;
        const double* u = &V[e * N];
        // a component whose singular value is 0 up to rounding has no defined vector: 0.00
        const bool null = !(sg > 1e-6 * top) || top == 0;   // (the Gram route resolves singular values down to about 1e-8 of the first)
        double usum = 0;
        for (size_t j = 0; j < N; ++j) usum += u[j];
        for (size_t i = 0; i < N; ++i) {
            double t = 0;
            for (size_t j = 0; j < N; ++j) t += (double)G[i * N + j] * u[j];
            out[i * (size_t)k + (size_t)c] = null ? 0.0 : (t - g[i] * usum) / sg;
        }
    }
    return 0;
}

extern "C" void gdh_round3g(const float* x, size_t n, uint32_t* out)
{
    for (size_t i = 0; i < n; ++i) out[i] = gd_round3g(x[i]);
}

extern "C" int gdh_fmt3g(uint32_t cell, char* out, size_t cap)
{
    char buf[16];
    const int n = gd_fmt3g(cell, buf);
    if ((size_t)n + 1 > cap) return -1;
    memcpy(out, buf, (size_t)n);
    out[n] = 0;
    return n;
}

extern "C" int gdh_crai_read(const char* path, size_t cap_refs, size_t cap_slices, int64_t* ref_off, int64_t* aln_start, int64_t* aln_span,
                             int32_t* slice_len, size_t* n_refs, size_t* n_slices, int64_t* line, char* msg, size_t cap_msg)
{
    if (!path || !n_refs || !n_slices || !line) return -1;
    gdh::CraiSlices c;
    std::string why;
    *n_refs = *n_slices = 0;
    if (!gdh::read_crai(path, &c, line, &why)) {
        if (msg && cap_msg) snprintf(msg, cap_msg, "%s", why.c_str());
        return -2;
    }
    *n_refs = c.ref_off.size() - 1;
    *n_slices = c.start.size();
    if (!ref_off || cap_refs < *n_refs || cap_slices < *n_slices) return -3;
    if (*n_slices && (!aln_start || !aln_span || !slice_len)) return -1;
    std::copy(c.ref_off.begin(), c.ref_off.end(), ref_off);
    std::copy(c.start.begin(), c.start.end(), aln_start);
    std::copy(c.span.begin(), c.span.end(), aln_span);
    std::copy(c.len.begin(), c.len.end(), slice_len);
    return 0;
}

extern "C" int gdh_indexcov_run(int argc, const char* const* argv)
{
    IArgs a;
    const int p = parse_args(argc, argv, &a);
    if (p > 0) return 0;
    if (p == -2) return 1;
    if (p < 0) return 255;
    return run(a);
}

extern "C" int gdh_indexcov_main(int argc, const char* const* argv) { return gdh_indexcov_run(argc, argv); }
