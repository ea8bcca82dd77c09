// cnveval_host.cpp -- host twin of the reference's cnveval command (cnveval/cmd/cnveval/cnveval.go).
//
//   goleft-depth cnveval [-m MINOVERLAP] [-s] truth.bed[.gz] test.bed[.gz]
//
// Precision and recall of a call set against a truth set, per size class.  This file reads the two files, gives the
// samples ids (the union of both sets), ranks the chromosomes by their names as byte strings (so 10 < 2), sorts every
// sample's calls by (rank, start) with a stable sort -- calls that tie keep their input order -- and prints the four
// lines; the counting is gd_cnveval's, on the device.  The reference's x.cpu.pprof is not written.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "../../../include/goleft_depth.h"
#include "../../../include/goleft_depth_host.h"
#include "cli.hpp"

namespace {

struct CArgs {
    double min_overlap = 0.4;
    bool limit_samples = false;
    std::vector<std::string> pos;
};

void usage(FILE* f)
{
    fputs("usage: cnveval [--minoverlap MINOVERLAP] [--limitsamples] TRUTH TEST\n"
          "  -m, --minoverlap    minimum overlap proportion for intervals to be considered as overlapping (default 0.4; above 0, at most 1)\n"
          "  -s, --limitsamples  only include sites of the truth-set that have matching samples in the test-set\n"
          "  TRUTH, TEST         bed files, plain or gzipped: chrom, start, end, copy number, samples (comma-separated)\n", f);
}

int parse_args(int argc, const char* const* argv, CArgs* a)
{
    using gdh::cli::Args;
    Args c(argc, argv, usage);
    for (;;) {
        const Args::Kind kind = c.next();
        if (kind == Args::End) break;
        if (kind == Args::Help) return 1;
        if (kind == Args::Positional) { a->pos.push_back(c.arg); continue; }
        if (c.key == "-s" || c.key == "--limitsamples") {
            if (c.has_val) return c.fail("%s takes no value", c.key.c_str());
            a->limit_samples = true;
            continue;
        }
        if (c.key != "-m" && c.key != "--minoverlap") return c.fail("unknown argument %s", c.arg.c_str());
        if (!c.value()) return -1;
        char* end = nullptr;
        const double v = strtod(c.val.c_str(), &end);
        if (c.val.empty() || *end || !(v > 0 && v <= 1)) return c.fail("%s %s: minoverlap must be between 0 and 1", c.key.c_str(), c.val.c_str());
        a->min_overlap = v;
    }
    if (a->pos.size() != 2) return c.fail("truth and test are required");
    return 0;
}

using gdh::cli::now_s;

struct Line {
    std::string chrom;
    int32_t start, end, cn;
    std::vector<std::string> samples;
};

// strconv.Atoi's syntax: an optional sign and decimal digits, nothing else
bool parse_int(const std::string& s, long long* out)
{
    size_t i = s.size() && (s[0] == '+' || s[0] == '-') ? 1 : 0;
    if (i == s.size()) return false;
    long long v = 0;
    for (; i < s.size(); ++i) {
        if (s[i] < '0' || s[i] > '9') return false;
        if (v < (1LL << 40)) v = v * 10 + (s[i] - '0');       // (beyond every range asked of it: it stays there)
    }
    *out = s[0] == '-' ? -v : v;
    return true;
}

// parseTruth (:65-107) without its filter: every line that ends in a newline and does not start with '#'
int read_bed(const std::string& path, std::vector<Line>* out)
{
    gdh::cli::Lines in;
    if (!in.open(path)) { fprintf(stderr, "cnveval: cannot open %s\n", path.c_str()); return 1; }
    std::string line;
    const long long& lineno = in.lineno;
    while (in.next(&line)) {
        if (!in.whole) {
            // ReadString returns such a line together with io.EOF, and the reference's loop leaves on io.EOF first
            fprintf(stderr, "cnveval: %s:%lld: the last line has no newline and is not read, as in the reference\n", path.c_str(), lineno);
            break;
        }
        if (line[0] == '#') continue;            // (an empty line has a NUL there)
        if (line.empty()) { fprintf(stderr, "cnveval: %s:%lld: an empty line\n", path.c_str(), lineno); return 1; }
        std::vector<std::string> tok;
        for (size_t b = 0;;) {
            const size_t e = line.find('\t', b);
            tok.push_back(line.substr(b, e == std::string::npos ? e : e - b));
            if (e == std::string::npos) break;
            b = e + 1;
        }
        if (tok.size() < 5) {
            fprintf(stderr, "cnveval: %s:%lld: expected five fields for CNVs (chrom, start, end, copy number, samples), found %zu\n", path.c_str(), lineno, tok.size());
            return 1;
        }
        long long v[3];
        static const char* const what[3] = {"start", "end", "copy number"};
        for (int k = 0; k < 3; ++k) {
            if (!parse_int(tok[1 + k], &v[k])) { fprintf(stderr, "cnveval: %s:%lld: the %s, %s, is not an integer\n", path.c_str(), lineno, what[k], tok[1 + k].c_str()); return 1; }
            if (v[k] > INT32_MAX || v[k] < INT32_MIN || (k < 2 && v[k] < 0)) {
                fprintf(stderr, "cnveval: %s:%lld: the %s, %s, is outside %s .. 2147483647\n", path.c_str(), lineno, what[k], tok[1 + k].c_str(), k < 2 ? "0" : "-2147483648");
                return 1;
            }
        }
        if (v[1] < v[0]) { fprintf(stderr, "cnveval: %s:%lld: the end, %lld, is before the start, %lld\n", path.c_str(), lineno, v[1], v[0]); return 1; }
        Line l;
        l.chrom = tok[0]; l.start = (int32_t)v[0]; l.end = (int32_t)v[1]; l.cn = (int32_t)v[2];
        for (size_t b = 0;;) {                   // strings.Split: an empty field is a name too
            const size_t e = tok[4].find(',', b);
            l.samples.push_back(tok[4].substr(b, e == std::string::npos ? e : e - b));
            if (e == std::string::npos) break;
            b = e + 1;
        }
        out->push_back(std::move(l));
    }
    return 0;
}

// Go's %.4f of float64(a) / float64(b)
std::string ratio(int64_t a, int64_t b)
{
    if (b == 0) return "NaN";
    char buf[64];
    snprintf(buf, sizeof buf, "%.4f", (double)a / (double)b);
    return buf;
}

int run(const CArgs& a, FILE* out)
{
    const double t_begin = now_s();
    std::vector<Line> test, all_truth, truth;
    if (read_bed(a.pos[1], &test)) return 1;
    fprintf(stderr, "cnveval: cnvs in test-set (%zu)\n", test.size());
    if (read_bed(a.pos[0], &all_truth)) return 1;
    if (a.limit_samples) {
        std::unordered_set<std::string> have;
        for (const Line& l : test) have.insert(l.samples[0]);
        for (Line& l : all_truth)
            if (std::any_of(l.samples.begin(), l.samples.end(), [&](const std::string& s) { return have.count(s) != 0; })) truth.push_back(std::move(l));
    } else {
        truth.swap(all_truth);
    }
    size_t n_named = 0;
    for (const Line& l : truth) n_named += l.samples.size();
    fprintf(stderr, "cnveval: %zu total cnvs in truth-set (%zu)\n", n_named, truth.size());
    // ids: the samples in order of first appearance, the test set first; ranks: the chromosome names as byte strings
    std::unordered_map<std::string, int32_t> sid;
    auto id_of = [&](const std::string& s) { return sid.emplace(s, (int32_t)sid.size()).first->second; };
    std::vector<std::string> chroms;
    for (const Line& l : test) { id_of(l.samples[0]); chroms.push_back(l.chrom); }
    for (const Line& l : truth) { for (const std::string& s : l.samples) id_of(s); chroms.push_back(l.chrom); }
    std::sort(chroms.begin(), chroms.end());
    chroms.erase(std::unique(chroms.begin(), chroms.end()), chroms.end());
    auto rank_of = [&](const std::string& c) { return (int32_t)(std::lower_bound(chroms.begin(), chroms.end(), c) - chroms.begin()); };
    if (sid.size() > (size_t)GD_CNVEVAL_MAX_SAMPLES) { fprintf(stderr, "cnveval: %zu samples, at most %d\n", sid.size(), GD_CNVEVAL_MAX_SAMPLES); return 1; }
    const size_t S = sid.size(), C = test.size(), T = truth.size();
    struct Call { int32_t sample, chrom, start, end, cn; };
    std::vector<Call> calls(C);
    for (size_t i = 0; i < C; ++i) calls[i] = Call{sid[test[i].samples[0]], rank_of(test[i].chrom), test[i].start, test[i].end, test[i].cn};
    std::stable_sort(calls.begin(), calls.end(), [](const Call& x, const Call& y) {
        return x.sample != y.sample ? x.sample < y.sample : x.chrom != y.chrom ? x.chrom < y.chrom : x.start < y.start;
    });
    std::vector<int64_t> cnv_off(S + 1, 0), t_off(T + 1, 0);
    std::vector<int32_t> c_chrom(C), c_start(C), c_end(C), c_cn(C), t_chrom(T), t_start(T), t_end(T), t_cn(T), t_samples;
    for (size_t i = 0; i < C; ++i) {
        ++cnv_off[(size_t)calls[i].sample + 1];
        c_chrom[i] = calls[i].chrom; c_start[i] = calls[i].start; c_end[i] = calls[i].end; c_cn[i] = calls[i].cn;
    }
    for (size_t s = 0; s < S; ++s) cnv_off[s + 1] += cnv_off[s];
    t_samples.reserve(n_named);
    for (size_t t = 0; t < T; ++t) {
        t_chrom[t] = rank_of(truth[t].chrom); t_start[t] = truth[t].start; t_end[t] = truth[t].end; t_cn[t] = truth[t].cn;
        for (const std::string& s : truth[t].samples) t_samples.push_back(sid[s]);
        t_off[t + 1] = (int64_t)t_samples.size();
    }
    const double t_read = now_s() - t_begin;
    gdh::cli::Device ctx;
    if (!ctx.open("cnveval")) return 1;
    std::vector<int64_t> stats(S * 12, 0);
    {
        const int rc = gd_cnveval(ctx, (int32_t)S, cnv_off.data(), c_chrom.data(), c_start.data(), c_end.data(), c_cn.data(), T, t_chrom.data(),
                                  t_start.data(), t_end.data(), t_cn.data(), t_off.data(), t_samples.data(), a.min_overlap, stats.data());
        if (rc != GD_OK) {
            fprintf(stderr, "cnveval: gd_cnveval: %s (%s)\n", gd_strerror(rc), gd_last_error(ctx));
            return 1;
        }
    }
    double lib[3] = {0, 0, 0};
    (void)gd_cnveval_timing(ctx, lib, 3);
    ctx.reset();
    // Tabulate (cnveval.go:118-133) and Stat.String (:93-96); '-' overrides '0' in %-04d: left-justified, space-padded
    int64_t tab[4][4] = {};
    for (size_t s = 0; s < S; ++s)
        for (int k = 0; k < 3; ++k)
            for (int f = 0; f < 4; ++f) { tab[k][f] += stats[(s * 3 + k) * 4 + f]; tab[3][f] += stats[(s * 3 + k) * 4 + f]; }
    static const char* const names[4] = {"0-20000", "20000-100000", ">=100000", "all"};
    for (int k = 0; k < 4; ++k) {
        const long long fp = tab[k][0], fn = tab[k][1], tp = tab[k][2];
        fprintf(out, "size-class: %-12s | precision: %s (%-4lld / (%-4lld + %-4lld)) recall: %s (%-4lld / (%-4lld + %-4lld))\n", names[k],
                ratio(tp, tp + fp).c_str(), tp, tp, fp, ratio(tp, tp + fn).c_str(), tp, tp, fn);
    }
    if (fflush(out) != 0) { fprintf(stderr, "cnveval: error writing the report\n"); return 1; }
    if (const char* e = getenv("GOLEFT_CNVEVAL_TIMING"); e && *e == '1')
        fprintf(stderr, "cnveval: %.4f s in all: reading %.4f, upload %.4f, kernels %.4f, read-back %.4f\n", now_s() - t_begin, t_read, lib[0], lib[1], lib[2]);
    return 0;
}

}  // namespace

extern "C" int gdh_cnveval_run(int argc, const char* const* argv, const char* out_path)
{
    CArgs a;
    const int p = parse_args(argc, argv, &a);
    if (p > 0) return 0;
    if (p < 0) return 255;
    return gdh::cli::run_to_output("cnveval", out_path, [&](FILE* out) { return run(a, out); });
}

extern "C" int gdh_cnveval_main(int argc, const char* const* argv) { return gdh_cnveval_run(argc, argv, nullptr); }
