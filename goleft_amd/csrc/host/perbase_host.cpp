// perbase_host.cpp -- `goleft-depth perbase`: the per-base depth of a BAM as runs of equal depth.
//
//   goleft-depth perbase [-Q Q] [-c CHROM] [-b regions.bed] [--quantize C1,C2,...] [-o OUT] in.bam
//
// A bedGraph -- `chrom start end depth`, what mosdepth calls per-base.bed and bedtools `genomecov -bga` --, or with
// --quantize `chrom start end lo:hi` for the stretches whose depths share a bin.  The BAM is read as `depth` reads it
// (host/bam_records.hpp), the contigs are computed with the per-base vector kept, and gd_perbase_runs encodes the runs on
// the device: only they cross the link.  Every wanted contig in header order, or with -b every BED line in file order, is
// walked in slices of GOLEFT_PERBASE_SLICE positions a device call; a run that continues across a slice boundary is joined
// here, so the output does not depend on the slice.  The text is formatted on several threads into buffers written in order.
#include <algorithm>
#include <atomic>
#include <cerrno>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <thread>
#include <vector>

#include "../../../include/goleft_depth.h"
#include "../../../include/goleft_depth_host.h"
#include "bam_reader.hpp"
#include "bam_records.hpp"
#include "cli.hpp"
#include "regions.hpp"

namespace {

using gdh::cli::now_s;
using gdh::regions::parse_cuts;
using gdh::regions::parse_int;
using gdh::regions::Region;

struct PArgs {
    int q = 1;                          // -Q, as depth's
    std::string chrom, bed, out, bam;
    std::vector<int32_t> cuts;          // --quantize
    bool quantize = false;
};

void usage(FILE* f)
{
    fputs("usage: perbase [-Q Q] [-c CHROM] [-b REGIONS.bed] [--quantize C1,C2,...] [-o OUT] BAM\n"
          "  -Q, --q         mapping quality cutoff (default 1)\n"
          "  -c, --chrom     only this chromosome\n"
          "  -b, --bed       only the regions of this BED file, in file order, clipped to their chromosome\n"
          "  --quantize      cut points: runs of equal depth BIN, labelled lo:hi (0:C1, C1:C2, ... Cn:inf); at most 32, increasing, from 1\n"
          "  -o, --out       write here instead of stdout\n"
          "  BAM             coordinate sorted; its .bai or .csi is used when there is one\n", f);
}

// 0 ok, 1 help shown, -1 error (message printed)
int parse_args(int argc, const char* const* argv, PArgs* a)
{
    using gdh::cli::Args;
    Args c(argc, argv, usage);
    std::vector<std::string> pos;
    for (;;) {
        const Args::Kind kind = c.next();
        if (kind == Args::End) break;
        if (kind == Args::Help) return 1;
        if (kind == Args::Positional) { pos.push_back(c.arg); continue; }
        const std::string k = c.key;
        if (k != "-Q" && k != "--q" && k != "-c" && k != "--chrom" && k != "-b" && k != "--bed" && k != "--quantize" && k != "-o" && k != "--out")
            return c.fail("unknown argument %s", c.arg.c_str());
        if (!c.value()) return -1;
        if (k == "-Q" || k == "--q") {
            if (!parse_int(c.val, &a->q)) return c.fail("%s %s: not an integer", k.c_str(), c.val.c_str());
        } else if (k == "-c" || k == "--chrom") a->chrom = c.val;
        else if (k == "-b" || k == "--bed") a->bed = c.val;
        else if (k == "-o" || k == "--out") a->out = c.val;
        else {
            std::string why;
            if (!parse_cuts(c.val, &a->cuts, &why)) return c.fail("--quantize %s: %s", c.val.c_str(), why.c_str());
            a->quantize = true;
        }
    }
    if (pos.empty()) return c.fail("bam is required");
    if (pos.size() > 1) return c.fail("too many positional arguments at '%s'", pos[1].c_str());
    a->bam = pos[0];
    return 0;
}

void append_int(std::string* out, int64_t v)
{
    char buf[24];
    char* p = buf + sizeof buf;
    const bool neg = v < 0;
    uint64_t u = neg ? 0 - (uint64_t)v : (uint64_t)v;
    do { *--p = (char)('0' + u % 10); u /= 10; } while (u);
    if (neg) *--p = '-';
    out->append(p, (size_t)(buf + sizeof buf - p));
}

// Lines of runs [k0, k1) of one region: run k ends where run k + 1 starts, the last of all at `last_end`.
void format_runs(std::string* out, const std::string& chrom, const uint32_t* starts, const int32_t* values, size_t k0, size_t k1, size_t n,
                 int64_t last_end, const std::vector<std::string>* labels)
{
    for (size_t k = k0; k < k1; ++k) {
        out->append(chrom);
        out->push_back('\t');
        append_int(out, starts[k]);
        out->push_back('\t');
        append_int(out, k + 1 < n ? (int64_t)starts[k + 1] : last_end);
        out->push_back('\t');
        if (labels) out->append((*labels)[(size_t)values[k]]);
        else append_int(out, values[k]);
        out->push_back('\n');
    }
}

struct Emitter {
    FILE* out;
    const std::vector<std::string>* labels;
    unsigned threads;
    bool io_ok = true;
    double text_s = 0;

    // the first n - 1 runs when `open` (the last one's end is not known yet), else all n with the last ending at region_end
    void write(const std::string& chrom, const std::vector<uint32_t>& s, const std::vector<int32_t>& v, bool open, int64_t region_end)
    {
        const double t0 = now_s();
        const size_t n = s.size(), m = open ? n - 1 : n;
        constexpr size_t kPiece = 1u << 16;                   // runs a buffer holds
        const size_t pieces = (m + kPiece - 1) / kPiece;
        std::vector<std::string> buf(pieces);
        std::atomic<size_t> next{0};
        auto work = [&]() {
            for (size_t p; (p = next.fetch_add(1)) < pieces;)
                format_runs(&buf[p], chrom, s.data(), v.data(), p * kPiece, std::min(m, (p + 1) * kPiece), n, region_end, labels);
        };
        const unsigned nt = (unsigned)std::min<size_t>(threads, std::max<size_t>(pieces, 1));
        std::vector<std::thread> th;
        for (unsigned t = 1; t < nt; ++t) th.emplace_back(work);
        work();
        for (auto& t : th) t.join();
        for (const std::string& b : buf)
            if (!b.empty()) io_ok = fwrite(b.data(), 1, b.size(), out) == b.size() && io_ok;
        text_s += now_s() - t0;
    }
};

int run(const PArgs& a, FILE* out)
{
    const double t_begin = now_s();
    std::string err;
    gdh::BamReader bam;
    if (!bam.open(a.bam, 0, &err)) { fprintf(stderr, "perbase: %s\n", err.empty() ? ("cannot open " + a.bam).c_str() : err.c_str()); return 1; }
    const auto& contigs = bam.contigs();
    std::map<std::string, int> tid_of;
    std::vector<int64_t> lens(contigs.size());
    for (size_t i = 0; i < contigs.size(); ++i) { tid_of.emplace(contigs[i].name, (int)i); lens[i] = contigs[i].length; }

    // ---- the regions, in output order ----------------------------------------------------------------------------------
    std::vector<Region> regions;
    if (!a.chrom.empty() && !tid_of.count(a.chrom)) { fprintf(stderr, "perbase: chromosome %s is not in the BAM header\n", a.chrom.c_str()); return 1; }
    if (!a.bed.empty()) {
        if (int rc = gdh::regions::read_bed("perbase", a.bed, tid_of, lens, &regions)) return rc;
        if (!a.chrom.empty()) {
            const int32_t only = tid_of[a.chrom];
            regions.erase(std::remove_if(regions.begin(), regions.end(), [&](const Region& r) { return r.tid != only; }), regions.end());
        }
    } else {
        for (size_t t = 0; t < contigs.size(); ++t)
            if (a.chrom.empty() || contigs[t].name == a.chrom) regions.push_back(Region{(int32_t)t, 0, lens[t]});
    }
    std::vector<int32_t> wanted;
    for (const Region& r : regions) wanted.push_back(r.tid);
    std::sort(wanted.begin(), wanted.end());
    wanted.erase(std::unique(wanted.begin(), wanted.end()), wanted.end());
    if (wanted.empty()) return 0;

    // ---- one device: records into HBM as depth reads them, then the per-base vector ------------------------------------
    gdh::rec::Shards S;
    S.v.resize(1);
    gdh::rec::Shard& sh = S.v[0];
    if (const char* e = getenv("GOLEFT_DEVICE")) sh.device = atoi(e);
    sh.wanted = wanted;
    {
        const int rc = gd_create(sh.device, &sh.ctx);
        if (rc != GD_OK) {
            sh.ctx = nullptr;
            fprintf(stderr, "perbase: no usable MI355X device (%s); this build has no CPU path\n", gd_strerror(rc));
            return 1;
        }
    }
    gd_ctx* const ctx = sh.ctx;
    gd_params P;
    gd_default_params(&P);
    P.min_mapq = a.q;
    if (int rc = gdh::rec::configure_context("perbase", ctx, P, lens, true, wanted)) return rc;
    const std::vector<int> shard_of(contigs.size(), 0);
    uint64_t n_gpu_records = 0;
    const auto t0 = std::chrono::steady_clock::now();
    gdh::rec::ReadTimes T{t0, t0, t0};
    if (int rc = gdh::rec::read_records("perbase", a.bam, bam, wanted, S, shard_of, &n_gpu_records, &T)) return rc;
    {
        const int rc = gd_compute(ctx);
        if (rc != GD_OK) { fprintf(stderr, "perbase: gd_compute failed: %s (%s)\n", gd_strerror(rc), gd_last_error(ctx)); return 1; }
    }
    const double t_computed = now_s();

    // ---- the runs ------------------------------------------------------------------------------------------------------
    int64_t slice = 1ll << 25;
    if (const char* e = getenv("GOLEFT_PERBASE_SLICE"); e && *e) slice = std::max<long long>(1, atoll(e));
    std::vector<std::string> labels;
    if (a.quantize)
        for (size_t b = 0; b <= a.cuts.size(); ++b)
            labels.push_back((b ? std::to_string(a.cuts[b - 1]) : std::string("0")) + ":" + (b < a.cuts.size() ? std::to_string(a.cuts[b]) : std::string("inf")));
    Emitter em{out, a.quantize ? &labels : nullptr, (unsigned)std::max(1, std::min(gdh::usable_cpus(), 16))};
    double lib[4] = {0, 0, 0, 0}, dev_s[4] = {0, 0, 0, 0};
    uint64_t n_runs = 0, n_calls = 0;
    std::vector<uint32_t> ts, fs;                             // a slice's runs; the region's joined runs not yet written
    std::vector<int32_t> tv, fv;
    constexpr size_t kFlush = 8u << 20;
    for (const Region& r : regions) {
        const std::string& chrom = contigs[(size_t)r.tid].name;
        fs.clear(); fv.clear();
        for (int64_t s0 = r.start; s0 < r.end; s0 += slice) {
            const int64_t s1 = std::min(r.end, s0 + slice);
            size_t n = 0;
            int rc = gd_perbase_runs(ctx, r.tid, s0, s1, (int)a.cuts.size(), a.cuts.data(), ts.data(), tv.data(), std::min(ts.size(), tv.size()), &n);
            if (rc == GD_E_CAPACITY) {
                ts.resize(n + n / 4); tv.resize(ts.size());
                rc = gd_perbase_runs(ctx, r.tid, s0, s1, (int)a.cuts.size(), a.cuts.data(), ts.data(), tv.data(), ts.size(), &n);
            }
            if (rc != GD_OK) { fprintf(stderr, "perbase: gd_perbase_runs failed: %s (%s)\n", gd_strerror(rc), gd_last_error(ctx)); return 1; }
            ++n_calls;
            (void)gd_perbase_runs_timing(ctx, lib, 4);
            for (int k = 0; k < 4; ++k) dev_s[k] += lib[k];
            // a slice's first run continues the run before it when their values are equal
            const size_t k0 = !fs.empty() && n && tv[0] == fv.back() ? 1 : 0;
            fs.insert(fs.end(), ts.begin() + (ptrdiff_t)k0, ts.begin() + (ptrdiff_t)n);
            fv.insert(fv.end(), tv.begin() + (ptrdiff_t)k0, tv.begin() + (ptrdiff_t)n);
            if (fs.size() > kFlush) {                          // all but the last: it may go on
                em.write(chrom, fs, fv, true, r.end);
                n_runs += fs.size() - 1;
                fs.erase(fs.begin(), fs.end() - 1);
                fv.erase(fv.begin(), fv.end() - 1);
            }
        }
        if (!fs.empty()) { em.write(chrom, fs, fv, false, r.end); n_runs += fs.size(); }
    }
    if (fflush(out) != 0) em.io_ok = false;
    if (!em.io_ok) { fprintf(stderr, "perbase: write error\n"); return 1; }
    if (const char* e = getenv("GOLEFT_PERBASE_TIMING"); e && *e == '1')
        fprintf(stderr, "perbase: %.4f s in all: reading + compute %.4f, count %.4f, scan %.4f, emit %.4f, read-back %.4f, text %.4f; %llu runs, %llu device calls, %s decoder\n",
                now_s() - t_begin, t_computed - t_begin, dev_s[0], dev_s[1], dev_s[2], dev_s[3], em.text_s, (unsigned long long)n_runs,
                (unsigned long long)n_calls, n_gpu_records ? "device" : "host");
    return 0;
}

}  // namespace

extern "C" int gdh_perbase_run(int argc, const char* const* argv, const char* out_path)
{
    PArgs a;
    const int p = parse_args(argc, argv, &a);
    if (p > 0) return 0;
    if (p < 0) return 1;
    if (out_path) a.out = out_path;
    if (a.bam.size() >= 5 && a.bam.compare(a.bam.size() - 5, 5, ".cram") == 0) {
        fprintf(stderr, "perbase: %s: a CRAM is not served, only a BAM\n", a.bam.c_str());
        return 1;
    }
    if (access(a.bam.c_str(), R_OK) != 0) { fprintf(stderr, "perbase: cannot open %s: %s\n", a.bam.c_str(), strerror(errno)); return 1; }
    return gdh::cli::run_to_output("perbase", a.out.empty() ? nullptr : a.out.c_str(), [&](FILE* out) { return run(a, out); });
}

extern "C" int gdh_perbase_main(int argc, const char* const* argv) { return gdh_perbase_run(argc, argv, nullptr); }
