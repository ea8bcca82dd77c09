// bam_records.hpp -- the records of a BAM into engine contexts that are ready to compute: what `depth` and `perbase` share
// between the BAM header and gd_compute.  An engine context per device ("shard") configured for the job (parameters, how the
// file's bytes reach the device, the contig table, the outputs, the contigs it computes), and the read itself: on the device
// through a .bai or .csi (GOLEFT_GPU_INDEX=1: through an index made on the device when the file has none), or with the host
// decoder through the pinned ring (GOLEFT_GPU_DECODE=0, no usable index, or a file the device read gives up on).
// `prog` is the name the messages carry.  Header-only; included by depth_host.cpp and perbase_host.cpp.
#pragma once
#include <unistd.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <thread>
#include <vector>

#include "../../../include/goleft_depth_host.h"
#include "bam_reader.hpp"
#include "gpu_ingest.hpp"
#include "index_build.hpp"

namespace gdh {
namespace rec {

// One engine context per device ("shard"): the reference parallelises over tiles inside one process
// (`-p`, depth/depth.go:392-394) and merges in :394-421; here the unit is a contig, assigned to a device.
struct Shard {
    gd_ctx* ctx = nullptr;
    int device = 0;
    std::vector<int32_t> wanted;        // the references this shard computes (ascending)
    uint64_t n_gpu_records = 0;
    int rc = GD_OK;                     // result of the shard's worker thread
    bool io_ok = true;
    std::string what;                   // the failing call
};

struct Shards {
    std::vector<Shard> v;
    ~Shards()
    {
        if (gdh_get_fast_exit()) return;                     // the process is about to exit (main.cpp)
        for (Shard& s : v) if (s.ctx) gd_destroy(s.ctx);
    }
};

#define GDH_REC_CHK(prog_, cx_, call)                                                  \
    do {                                                                               \
        int rc_ = (call);                                                              \
        if (rc_ != GD_OK) {                                                            \
            fprintf(stderr, "%s: %s failed: %s (%s)\n", (prog_), #call, gd_strerror(rc_), \
                    (cx_) ? gd_last_error(cx_) : "");                                  \
            return 1;                                                                  \
        }                                                                              \
    } while (0)

// measurement switches of the CLI (README): an integer from the environment, or the default
inline int env_int(const char* name, int dflt)
{
    const char* e = getenv(name);
    return e && *e ? atoi(e) : dflt;
}

// fn on every shard that has contigs, each on its own OS thread (every gd_* entry point re-issues hipSetDevice); false
// (after a message) when one failed.
inline bool run_on_every_shard(const char* prog, Shards& S, const char* what, const std::function<int(Shard&)>& fn)
{
    std::vector<std::thread> th;
    for (size_t k = 1; k < S.v.size(); ++k)
        th.emplace_back([&, k]() { S.v[k].rc = S.v[k].wanted.empty() ? GD_OK : fn(S.v[k]); });
    S.v[0].rc = S.v[0].wanted.empty() ? GD_OK : fn(S.v[0]);
    for (auto& t : th) t.join();
    for (Shard& sh : S.v)
        if (sh.rc != GD_OK) {
            fprintf(stderr, "%s: %s failed on device %d: %s (%s)\n", prog, what, sh.device, gd_strerror(sh.rc),
                    gd_last_error(sh.ctx));
            return false;
        }
    return true;
}

struct ReadTimes { std::chrono::steady_clock::time_point indexed, mapped, read; };

// Is there a file where the index of `bam` is looked for (x.bam.bai, x.bai, x.bam.csi, x.csi)?
inline bool index_file_exists(const std::string& bam)
{
    const bool is_bam = bam.size() > 4 && bam.compare(bam.size() - 4, 4, ".bam") == 0;
    for (const char* suffix : {".bai", ".csi"}) {
        if (access((bam + suffix).c_str(), F_OK) == 0) return true;
        if (is_bam && access((bam.substr(0, bam.size() - 4) + suffix).c_str(), F_OK) == 0) return true;
    }
    return false;
}

// One context configured for a job: parameters, how the BAM's bytes reach the device, the contig table, the outputs the
// caller needs, and the contigs it computes.  0, or 1 after the failed call has been reported.
inline int configure_context(const char* prog, gd_ctx* ctx, const gd_params& P, const std::vector<int64_t>& lens, bool need_perbase,
                             const std::vector<int32_t>& wanted)
{
    GDH_REC_CHK(prog, ctx, gd_set_params(ctx, &P));
    GDH_REC_CHK(prog, ctx, gd_set_option(ctx, GD_OPT_COPY_THREADS, env_int("GOLEFT_COPY_THREADS", 4)));   // staging copies of the device BAM read
    // How the BAM's bytes reach the device: a copy KERNEL on CUs of its own (every 8th), the inflate launches on the
    // others (CU-masked streams).  One copy engine moves 21-22 GB/s next to the inflate kernels (and its reads of host
    // memory slow the pread into the staging buffers down: 0.8-2.1 s per genome by box against 0.65 s); the kernel on 32
    // dedicated CUs moves 35 GB/s.  GOLEFT_INGEST_DMA=1 brings the copy engine back, GOLEFT_INGEST_CU_SPLIT=0 the
    // unmasked streams (profiles/r11d_, r11e_scope3_genome.json).
    GDH_REC_CHK(prog, ctx, gd_set_option(ctx, GD_OPT_INGEST_DMA, env_int("GOLEFT_INGEST_DMA", 0)));
    if (!getenv("GOLEFT_INGEST_CU_SPLIT") && env_int("GOLEFT_INGEST_DMA", 0) == 0)
        GDH_REC_CHK(prog, ctx, gd_set_option(ctx, GD_OPT_INGEST_CU_SPLIT, 8));
    if (getenv("GOLEFT_INGEST_CU_SPLIT")) GDH_REC_CHK(prog, ctx, gd_set_option(ctx, GD_OPT_INGEST_CU_SPLIT, env_int("GOLEFT_INGEST_CU_SPLIT", 0)));
    if (getenv("GOLEFT_INGEST_COPY_GRID")) GDH_REC_CHK(prog, ctx, gd_set_option(ctx, GD_OPT_INGEST_COPY_GRID, env_int("GOLEFT_INGEST_COPY_GRID", 16)));   // workgroups of the copy kernel
    if (getenv("GOLEFT_INFLATE_KERNEL")) GDH_REC_CHK(prog, ctx, gd_set_option(ctx, GD_OPT_INFLATE_KERNEL, env_int("GOLEFT_INFLATE_KERNEL", 0)));
    if (env_int("GOLEFT_TRUST_BGZF", 0)) GDH_REC_CHK(prog, ctx, gd_set_option(ctx, GD_OPT_INGEST_CRC, 0));
    // the context's worker threads (they pread the file's pieces into the staging buffers): 16 unless the container grants
    // few CPUs -- under a 16-CPU quota sixteen of them and the member lister's threads together ran into the quota (the
    // kernel then stops EVERY thread until the period ends: 6 - 13 throttled periods per genome, the file's pieces read at
    // half the rate); ten of them still read faster than the link takes the bytes
    {
        const int cpus = gdh::usable_cpus();
        const int pt = env_int("GOLEFT_PUSH_THREADS", cpus <= 16 ? std::max(4, cpus * 5 / 8) : 0);
        if (pt) GDH_REC_CHK(prog, ctx, gd_set_option(ctx, GD_OPT_PUSH_THREADS, pt));
    }
    GDH_REC_CHK(prog, ctx, gd_set_contigs(ctx, (int)lens.size(), lens.data()));
    GDH_REC_CHK(prog, ctx, gd_set_option(ctx, GD_OPT_BAM_REFS, (int64_t)lens.size()));   // engine contigs = the BAM's references
    if (!need_perbase) GDH_REC_CHK(prog, ctx, gd_set_outputs(ctx, 0));   // windows + class runs are all the rows need
    if (!lens.empty() && !wanted.empty())
        GDH_REC_CHK(prog, ctx, gd_select_contigs(ctx, (int)wanted.size(), wanted.data()));
    return 0;
}

// ---- records into HBM (replaces the samtools children) ---------------------------
// With a .bai next to the BAM (goleft depth needs one anyway: `samtools depth -r`), the whole
// read happens on the device: the contig's byte range goes to gd_ingest_bgzf, which inflates
// the BGZF members and decodes the records there (GOLEFT_GPU_DECODE=0 keeps the host decoder).
// Every shard reads its own contigs' byte ranges from the shared mapping.
// -> 0, or the process's exit code; *n_gpu_records: what the device decoder delivered (0: the host decoder ran).
inline int read_records(const char* prog, const std::string& bam_path, gdh::BamReader& bam, const std::vector<int32_t>& wanted, Shards& S,
                        const std::vector<int>& shard_of, uint64_t* n_gpu_records_out, ReadTimes* T)
{
    const auto& contigs = bam.contigs();
    std::string err;
    uint64_t n_gpu_records = 0;
    auto now = []() { return std::chrono::steady_clock::now(); };
    auto ctx_of = [&](int tid) -> gd_ctx* { return S.v[(size_t)shard_of[(size_t)tid]].ctx; };
    auto on_every_shard = [&](const char* what, const std::function<int(Shard&)>& fn) { return run_on_every_shard(prog, S, what, fn); };
    auto& t_indexed = T->indexed; auto& t_mapped = T->mapped; auto& t_read = T->read;
    {
        std::vector<std::vector<uint64_t>> lin;
        std::vector<char> has_chunks;
        std::vector<uint64_t> chunk_end;
        const char* gd_env = getenv("GOLEFT_GPU_DECODE");
        bool gpu_decode = !(gd_env && gd_env[0] == '0') && gdh::BamReader::linear_index(bam_path, &lin, &err, &has_chunks, &chunk_end) &&
                          lin.size() == contigs.size();
        // GOLEFT_GPU_INDEX=1: a BAM whose index is NOT FOUND gets one made on the device, in memory (host/index_host.cpp; it is
        // not written), and the read below takes the device path with it.  An index that is there but unusable stays what it was.
        const char* gi_env = getenv("GOLEFT_GPU_INDEX");
        if (!gpu_decode && gi_env && gi_env[0] == '1' && !(gd_env && gd_env[0] == '0') && !index_file_exists(bam_path)) {
            std::vector<uint8_t> bai;
            std::string ierr;
            // (a reference no .bai can hold -- longer than 2^29 - 256 --: the same index as a .csi)
            int64_t longest = 0;
            for (const auto& ct : contigs) longest = std::max<int64_t>(longest, ct.length);
            const int rc = gdh::build_index(S.v[0].ctx, bam_path, longest + 256 > (1ll << 29) ? gdh::IndexFormat::Csi : gdh::IndexFormat::Bai,
                                            14, &bai, &ierr);
            if (rc != GD_OK) {
                fprintf(stderr, "%s: %s: cannot index on the device: %s\n", prog, bam_path.c_str(), ierr.c_str());
                return 1;
            }
            gpu_decode = gdh::BamReader::linear_index_bytes(bai, &lin, &err, &has_chunks, &chunk_end) && lin.size() == contigs.size();
        }
        // a reference whose bins hold chunks but whose linear index is empty (a non-htslib indexer):
        // the anchors cannot be trusted to mean "no records" -> host decoder
        for (size_t r = 0; gpu_decode && r < lin.size(); ++r)
            if (lin[r].empty() && r < has_chunks.size() && has_chunks[r]) gpu_decode = false;
        t_indexed = now();
        if (gpu_decode) {
            gdh::FileMap fm;
            if (!fm.open(bam_path)) gpu_decode = false;
            fm.keep = gdh_get_fast_exit() != 0;
            t_mapped = now();
            if (gpu_decode) {
                if (!on_every_shard("the device BAM read", [&](Shard& sh) {
                        return gdh::ingest_references_on_device(sh.ctx, fm, lin, sh.wanted, sh.wanted, &sh.n_gpu_records, &sh.io_ok,
                                                                (uint64_t)env_int("GOLEFT_INGEST_GROUP_MB", 512) << 20, &chunk_end,
                                                                // a reference larger than this is read in parts cut at .bai anchors
                                                                // (0: never; _KB: tests cut small files)
                                                                getenv("GOLEFT_INGEST_PART_KB") ? (uint64_t)env_int("GOLEFT_INGEST_PART_KB", 0) << 10
                                                                                                : (uint64_t)env_int("GOLEFT_INGEST_PART_MB", 2048) << 20);
                    }))
                    return 1;
                for (Shard& sh : S.v) {
                    if (!sh.io_ok) gpu_decode = false;
                    n_gpu_records += sh.n_gpu_records;
                }
                if (!gpu_decode) n_gpu_records = 0;
                t_read = now();
            }
            if (!gpu_decode)
                for (Shard& sh : S.v) GDH_REC_CHK(prog, sh.ctx, gd_reset(sh.ctx));   // fall back to the host decoder below
        }
        if (!gpu_decode) {
        if (wanted.size() == 1) bam.seek_contig(wanted[0], &err);   // .bai shortcut for --chrom
        std::vector<char> want(contigs.size(), 0);
        for (int32_t t : wanted) want[(size_t)t] = 1;
        const int32_t last_wanted = wanted.back();
        gdh::RecordBlock blk;
        for (;;) {
            const int rc = bam.next_block(blk, 1u << 21, &err);
            if (rc < 0) {
                fprintf(stderr, "%s: %s\n", prog, err.c_str());
                return 1;
            }
            if (rc == 0) break;
            if (blk.tid > last_wanted) break;                       // coordinate sorted: done
            if (blk.tid >= (int32_t)contigs.size() || !want[(size_t)blk.tid]) continue;
            gd_ctx* const ctx = ctx_of(blk.tid);
            gd_batch b;
            GDH_REC_CHK(prog, ctx, gd_acquire(ctx, blk.size(), blk.cigar.size(), &b));
            memcpy(b.pos, blk.pos.data(), blk.size() * sizeof(int32_t));
            memcpy(b.flag, blk.flag.data(), blk.size() * sizeof(uint16_t));
            memcpy(b.mapq, blk.mapq.data(), blk.size() * sizeof(uint8_t));
            memcpy(b.cigar_off, blk.cigar_off.data(), (blk.size() + 1) * sizeof(uint32_t));
            if (!blk.cigar.empty()) memcpy(b.cigar, blk.cigar.data(), blk.cigar.size() * sizeof(uint32_t));
            GDH_REC_CHK(prog, ctx, gd_commit(ctx, &b, blk.tid, blk.size(), blk.cigar.size()));
        }
        }
    }
    *n_gpu_records_out = n_gpu_records;
    return 0;
}

#undef GDH_REC_CHK

}  // namespace rec
}  // namespace gdh
