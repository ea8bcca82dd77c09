// gd_api_state.hpp -- what a gd_ctx holds and the helpers every part of the C ABI shares: per-contig
// record streams, the pinned staging ring, the device job state, what a gd_compute carries from launch to finish
// (ComputeState: the route and the profiling stages of the attempt in flight), the in-flight guard, the route rule
// (compute_route) and the launch helpers of the tile kernels that take its answer, the long-read structures
// (gd_chunk.hpp) and the state of a device BAM read.  Included by gd_api.hip only (one translation unit: the
// kernels of gd_kernels.hpp are not inline).
//
// Ownership: every device array, page-locked array, event and stream the context keeps is a member of one of
// gd_own.hpp's four owner types, here or in a state the context holds by unique_ptr, and goes when its holder goes:
// nothing is freed by name.  What grows goes through ensure_dev, reserve_records (a contig's records) or IngestBufs::fit /
// fit_host (the device BAM read); DevBuf and DevList are one call's scratch.  Raw pointers are aliases or the caller's.
#pragma once

#include "gd_own.hpp"

#include <memory>
#include <atomic>
#include <mutex>
#include <thread>

namespace {

using gd_own::DevArr, gd_own::PinArr, gd_own::Event, gd_own::Stream;

constexpr int kRingSlots = 4;
constexpr size_t kSpecBounds = 4096;     // boundaries copied to the host before their count is known (one synchronisation)
constexpr int kDefaultLookback = 512;
constexpr uint64_t kMaxReadsPerContig = 1ull << 30;
constexpr int kTileT = gd::shape::T;       // reference positions per tile (gd_kernels.hpp: the one shape that is built)
constexpr int kAutoLongSpan = 32768;      // GD_PATH_AUTO leaves the short-read tile path above this read span
constexpr int kMaxSpan = 1 << 27;   // tile-relative byte offsets of the tile kernel stay in 32 bits

// One device allocation shared by the derived arrays of a batch of contigs (long-read structures, position
// indexes, long-read structures): a batch is built with one hipMalloc and no per-contig host round trip; the
// block goes back to HBM when the last contig that points into it drops its share.
typedef std::shared_ptr<DevArr<uint8_t>> BlockRef;

struct ContigHost {
    int64_t length = 0;
    // device record stream (owned; adopted: borrowed from the caller, who frees it).  reserve_records grows pos, flag,
    // mapq and off (one element more) together, off last: its capacity is the group's
    DevArr<int32_t>  pos;
    DevArr<uint16_t> flag;
    DevArr<uint8_t>  mapq;
    DevArr<uint32_t> off;
    DevArr<uint32_t> cigar;
    size_t n_reads = 0, n_ops = 0;
    size_t cap_reads() const { return off.cap() ? off.cap() - 1 : 0; }
    bool adopted = false;
    int32_t last_pos = -0x7fffffff;
    // long-read path (gd_chunk.hpp): deletion lists, read records and tile indexes, built straight from the records
    // (slices of ck_blk)
    BlockRef ck_blk;
    uint4*    lrec = nullptr;          // n_reads + 2 long-read records {pos, end, list offset, deletions}; [n_reads + 1].x = the largest span
    uint32_t* lfq = nullptr;           // n_reads: flag << 8 | MAPQ
    uint2*    dl = nullptr;            // (ops >> 1) + n_reads + 1 deletions {start, length}
    uint32_t* pck = nullptr;           // tile indexes (filled by gd_dels_raw_kernel)
    uint32_t* ndel = nullptr;          // deletions per read
    int32_t   max_span = 0;
    uint64_t  n_dels = 0;              // deletions in dl
    bool ck_ok = false;                // lrec / lfq / dl / pck describe the current records
    // built as the records arrive (gd_index_records_kernel): the position index, ridx[k] = first read with pos >= 64 k
    DevArr<uint32_t> ridx;             // (length >> 6) + 2 entries; valid up to entry pos[ridx_reads - 1] >> 6
    size_t ridx_reads = 0;             // records it covers (== n_reads: gd_prep_kernel uses it)
    bool ing_left = false;             // device BAM read in parts: a record of another reference has ended this one's records
    // layout in the result arrays of the last compute (-1 = not computed)
    int64_t base_off = -1;
    int64_t win_off = -1;
    int64_t n_win = 0;
    size_t run_beg = 0, run_end = 0;   // slice of ctx->bounds
};

struct RingSlot {
    gd_batch b{};            // what gd_acquire hands out: its pointers and capacities mirror the owners below
    PinArr<int32_t> pos;
    PinArr<uint16_t> flag;
    PinArr<uint8_t> mapq;
    PinArr<uint32_t> cigar_off, cigar;
    Event done;
    bool busy = false;       // its copy may still be in flight (`done`)
    bool held = false;       // handed out by gd_acquire, not committed yet
};

}  // namespace

// State of a device BAM read between gd_ingest_begin and gd_ingest_finish.
struct IngestState;
namespace { struct FillPool; struct CovState; struct IdxState; struct IcState; struct IsState; struct EcState; }

// Device buffers of one pending range (compressed bytes, inflated bytes, member tables): grow-only and
// kept by the context between ranges -- allocating and freeing gigabytes per range cost 0.1-0.2 s.
struct IngestBufs {
    gd_own::DevArr<uint8_t> in, out;
    gd_own::PinArr<uint8_t> tab;
    bool busy = false;
    static bool fit(gd_own::DevArr<uint8_t>& a, size_t need)
    {
        if (need <= a.cap() && a) return true;
        // (a quarter more than asked for when it has to GROW: ranges of about one size -- a reference read in parts --
        // would otherwise free and allocate again for every range a little larger than the last, and a hipFree waits for
        // the whole device, the other range's inflate kernels included)
        const size_t want = a ? need + need / 4 : (need ? need : 1);
        a.reset();
        return a.alloc(want) == hipSuccess;
    }
    // The member tables live in PAGE-LOCKED HOST memory that the kernels read (and write: the status words) over the
    // link: a few bytes per member, once.  As device arrays they were five blocking uploads per range -- each of which
    // queued on the copy engine behind the 64 MB pieces of the read in progress (20 ms per gd_ingest_begin measured).
    static bool fit_host(gd_own::PinArr<uint8_t>& a, size_t need)
    {
        if (need <= a.cap() && a) return true;
        a.reset();
        // generously: freeing page-locked memory waits for the device like hipFree does -- ranges of slightly different
        // member counts (a reference read in parts) must not do that between every two of them (measured: 50 ms per
        // gd_ingest_begin, 1.4 s per genome)
        const size_t want = std::max<size_t>(2 * need + 4096, 8u << 20);
        return a.alloc(want) == hipSuccess;
    }
    void drop() { in.reset(); out.reset(); }
};


// What gd_compute carries from its launch to its finish (gd_api_compute.inc).
struct ComputeState {
    std::vector<int32_t> tids;          // contigs of the job
    uint64_t n_reads = 0, n_ops = 0, n_units = 0, n_groups = 0;
    int64_t tile_beg = 0, base_off = 0, win_off = 0, bases = 0;
    bool raw_aligned = true;            // ... arrays aligned for the raw straight-line kernel's vector loads
    int32_t route = GD_TK_NONE;         // compute_route's answer for the attempt in flight (GD_TK_NONE: a job without tiles)
    // profiling: stage k is the interval ev[k] .. ev[k + 1] and belongs to kernel_ms[stage_id[k]]; the last record
    // only closes the stage before it (scatter has the most: four stages, five records)
    int8_t stage_id[6] = {};
    int n_stages = 0;
    int reruns = 0, used_lookback = 0;
    int32_t chunk_span = 0;
    size_t spec = 0;                    // boundaries copied speculatively with the counters
    bool pending = false;               // launched, not finished
    bool nothing = false;               // ... a job without tiles
};

struct GdUniqueId { char internal[128]; };   // ncclUniqueId's layout (rccl.h: NCCL_UNIQUE_ID_BYTES = 128)

struct gd_ctx {
    __attribute__((visibility("hidden"))) gd_ctx();     // (both defined at the end of gd_api.hip, where the kept states
    __attribute__((visibility("hidden"))) ~gd_ctx();    // are complete types)
    int device = 0;
    // the two streams are declared first: they are destroyed last, after everything that may have work on them
    Stream stream;                      // compute stream: the context's own, or the caller's (gd_set_stream), borrowed
    Stream copy_stream;
    Event copy_done;
    gd_params params{};
    std::vector<ContigHost> contigs;
    std::vector<int32_t> selected;      // empty = all
    RingSlot ring[kRingSlots];
    int ring_next = 0;
    bool commit_check_device = false;   // GD_OPT_COMMIT_CHECK
    bool commit_checks_pending = false; // blocks whose verdict (d_ingest[3]) nobody has read yet
    int32_t commit_tid_lo = 0, commit_tid_hi = 0;   // ... the contigs they belong to
    std::string err;

    // tuning knobs (gd_set_option; defaults are what the measurements of DESIGN.md section 4 chose)
    bool fast_kernel = true;            // GD_OPT_FAST_KERNEL: the straight-line tile kernel (gd_tile_fast.hpp) for
                                        // ordinary tiles, the generic one for the rest; 0 = generic for every tile
    std::vector<uint8_t> batch_tab_ck;  // host copy of the job table of the last ck batch
    PinArr<uint32_t> h_batch;           // pinned: per-contig totals / status words coming back
    int tile_opt = 1;                   // bit 0: non-temporal per-base stores (2 % faster: the vector is
                                        // never re-read by the kernel)
    bool lookback_pinned = false;       // max_span_hint given: never shrink below it
    int path = GD_PATH_AUTO;            // gd_set_path
    bool keep_perbase = true;           // gd_set_outputs(GD_OUT_PERBASE)
    bool sums_only = false;             // gd_set_outputs(GD_OUT_SUMS_ONLY): window sums, nothing else
    bool ran_sums_only = false;         // what the last gd_compute produced
    bool span_forces_long = false;      // AUTO: the tile path met a read too long for it
    DevArr<unsigned long long> d_status;   // scatter path look-back words
    int lookback = kDefaultLookback;
    // gd_index_records_kernel's words: [0] check flags, [1] the largest reference span of any record that has arrived
    // since gd_reset / gd_set_contigs (INT_MAX: a record it did not walk), [2] the last position of the last launch
    DevArr<uint32_t> d_ingest;
    bool ingest_span_dirty = false;     // [1] may have grown since the host last read it
    int32_t ingest_span = 0;            // the host's copy (0: nothing measured)
    bool ingest_index = true;           // GD_OPT_INGEST_INDEX
    double alloc_in_enqueue = 0;        // seconds of device allocation inside the last enqueue (the long-read block): counted as `prepare`
    double timing[4] = {0, 0, 0, 0};    // gd_compute_timing: allocations + contig table, enqueue, wait, total of the last gd_compute

    // device job state
    DevArr<gd::ContigDev> d_ctgs;
    std::vector<gd::ContigDev> h_ctgs;
    std::vector<gd::ContigDev> up_ctgs;   // what d_ctgs holds
    gd::ContigDev* up_ctgs_dev = nullptr;
    uint32_t slow_grid = 64;             // workgroups of gd_tile_slow_kernel
    std::vector<int32_t> job_tids;      // contig table index -> tid
    DevArr<gd::TileInfo> d_tiles;         // d_tiles, d_tile_cnt, d_tile_off (and d_super_cnt, a SUPER-th of them) grow together
    DevArr<gd::TileFast> d_ftiles;
    DevArr<int32_t> d_perbase;
    DevArr<int64_t> d_wsum;               // d_wsum and d_wmin grow together
    DevArr<int32_t> d_wmin;
    DevArr<int2> d_chunks;                // d_chunks and d_ordered grow together, d_ordered last: its capacity is
    DevArr<int2> d_ordered;               // Job::run_cap (never above d_chunks')
    DevArr<uint32_t> d_tile_cnt;
    DevArr<uint32_t> d_tile_off;
    DevArr<uint32_t> d_super_cnt;
    DevArr<gd::Counters> d_counters;
    PinArr<gd::Counters> h_counters;
    PinArr<int2> h_bounds;                // the first kSpecBounds ordered boundaries travel with the counters
    uint32_t parity = 0;                  // Counters::n_slow in use (alternates per compute)
    bool slow_counter_clean = false;      // the last enqueue ran gd_prep_kernel, which zeroed the other counter
    DevArr<uint32_t> d_region_cursor;

    DevArr<int64_t> d_wed;                             // gd_depthwed: tables + the sites x samples matrix
    DevArr<uint32_t> d_md_bits;                        // gd_md_flags: `any` words then `suf` words
    DevArr<uint16_t> d_md_cnt;                         // gd_md_begin .. gd_md_finish: samples >= min_cov per position
    int64_t md_acc_len = -1;                           // gd_md_begin's length (-1: not begun)
    int64_t md_acc_samples = 0;
    int64_t md_len = -1;                               // positions the bitmaps cover (-1: none yet)
    std::vector<int32_t> md_tids;                      // the samples they were built from
    // gd_ingest_begin .. gd_ingest_finish.  Two ranges may be pending: ing_q[0] is the oldest (the one
    // gd_ingest_decode / _finish / _release act on), the last one is being fed -- so the inflate tail of
    // one range overlaps the upload of the next.
    // ranges that may be pending: one being decoded, one inflating, one being fed (include/goleft_depth.h: a fourth
    // gd_ingest_begin is refused).  Four were measured -- 2.42 against 2.44 s per genome read, profiles/r12u_... -- and not kept.
    static constexpr int kIngestDepth = 3;
    IngestState* ing_q[kIngestDepth] = {};
    int ing_n = 0;
    double ing_secs[7] = {0, 0, 0, 0, 0, 0, 0};         // gd_ingest_timing
    std::thread ing_feeder;                             // gd_ingest_feed_fd: the read of the newest range in progress
    int ing_feeder_rc = 0;
    std::string ing_feeder_err;                         // what the feeder thread's failure said (published by ingest_join)
    double ing_feeder_secs[2] = {0, 0};                 // its share of gd_ingest_timing [0], [1] (merged by ingest_join)
    bool ing_stage_used[2] = {false, false};
    int ing_cur = 0;                                   // the staging buffer the next piece goes through
    IngestBufs ing_bufs[kIngestDepth];
    // staging of the device BAM read, created by the first gd_ingest_begin and kept until gd_destroy
    // (page-locking 128 MB per contig would cost more than many contigs' whole decode)
    Stream ing_hp;                                     // GD_OPT_INGEST_DMA 0: the copy kernel's stream, high priority or (GD_OPT_INGEST_CU_SPLIT) CU-masked
    Stream ing_stream[8];                              // inflate launches rotate over these (two pending ranges x 4)
    PinArr<uint8_t> ing_stage[2];                      // page-locked staging buffers: one is filled while the other's piece leaves
    Event ing_staged[2];                               // ... recorded on the copy stream: the buffer's piece has arrived
    int ing_cu_split = 0;                              // GD_OPT_INGEST_CU_SPLIT: every n-th CU for the copy kernel, the rest for the inflate launches
    bool ing_copy_engine = true;                       // GD_OPT_INGEST_DMA: a staged piece leaves with a copy command (1) or with a copy kernel on ing_hp (0)
    unsigned ing_copy_grid = 16;                        // GD_OPT_INGEST_COPY_GRID: workgroups of the copy kernel that pulls a staged piece over the link
    Event ing_hp_done[2];                               // ing_hp: the copy stream waits for these before it records ing_staged[k]
    unsigned ing_launch_seq = 0;
    int ing_copy_threads = 1;                          // GD_OPT_COPY_THREADS: threads filling the staging buffer
    bool h2d_kernel = true;                            // GD_OPT_H2D_KERNEL: staging blocks reach HBM through gd_h2d_kernel
    unsigned h2d_grid = 512;                           // ... its workgroups
    bool ingest_crc = true;                            // GD_OPT_INGEST_CRC
    uint64_t ing_range_hint = 0;                       // GD_OPT_INGEST_RANGE_HINT: bytes of the largest range the caller will feed
    int inflate_kernel = 0;                            // GD_OPT_INFLATE_KERNEL
    int32_t bam_n_ref = 0;                             // GD_OPT_BAM_REFS: references of the BAM being read (0: unknown)
    int push_threads = 16;
    FillPool* pool = nullptr; int pool_workers = 0;    // host worker threads (gd_push fills, gd_commit validates), created on first use
    size_t push_chunk = 1u << 20;                      // GD_OPT_PUSH_CHUNK: records per staging block of gd_push                             // GD_OPT_PUSH_THREADS: threads of gd_push filling a ring block
    DevArr<uint32_t> d_scan_tmp;                               // launch_scan: block totals
    DevArr<uint8_t> d_rectab;                                  // ... and the record table the counting walk leaves for the extraction (device, grow-only)
    std::unique_ptr<CovState> cov;                             // gd_covstats_*: the sampling state and its buffers (gd_api_covstats.inc)
    std::unique_ptr<IdxState> idx;                             // gd_index_*: the runs, linear index and counts of the file so far (gd_api_index.inc)
    int64_t idx_slice = 65536;                                 // GD_OPT_INDEX_SLICE
    int idx_checks = 3;                                        // GD_OPT_INDEX_GUESS_CHECKS
    int idx_repair_rounds = 4;                                 // GD_OPT_INDEX_REPAIR_ROUNDS
    double idx_secs[5] = {0, 0, 0, 0, 0};                      // gd_index_timing
    std::unique_ptr<IcState> ic;                               // gd_indexcov_*: the cohort's tile sizes and results (gd_api_indexcov.inc)
    std::unique_ptr<IsState> isp;                              // gd_indexsplit_*: the cohort's cell sums (gd_api_indexsplit.inc)
    std::unique_ptr<EcState> ec;                               // gd_emcnv_*: the positions, member bits and member values of the rows so far (gd_api_emcnv.inc)
    double sm_secs[3] = {0, 0, 0};                             // gd_sample_medians*: upload, kernels, read-back of the last call (gd_api_colselect.inc)
    int sm_passes = 0;                                         // ... and the passes over the matrix it ran
    double cd_secs[7] = {0, 0, 0, 0, 0, 0, 0};                 // gd_chunk_debias: sort + chunking, upload, kernels, read-back of the last call; its chunks, its largest chunk;
                                                               // the median kernel alone when GOLEFT_CHUNKDEBIAS_SPLIT is set (gd_api_chunkdebias.inc)
    double md_secs[4] = {0, 0, 0, 0};                          // gd_moving_debias*: sort, upload, kernel, read-back of the last call (gd_api_movdebias.inc)
    int64_t md_segment = 0;                                    // GD_OPT_MOVDEBIAS_SEGMENT: sorted rows a workgroup owns (0: by the window)
    double sv_secs[5] = {0, 0, 0, 0, 0};                       // gd_svd_debias*: upload, statistics + Gram, eigenpairs (host), projection, read-back of the last call (gd_api_svddebias.inc)
    double ce_secs[4] = {0, 0, 0, 0};                          // gd_cnveval: preparation + upload, kernels, read-back of the last call, and the first kernel's part of the second (gd_api_cnveval.inc)
    DevArr<uint32_t> d_pb_cnt, d_pb_base;                      // gd_perbase_runs: run starts per chunk and their exclusive scan (grow-only; gd_api_perbase.inc)
    DevArr<uint32_t> d_pb_start;                               // ... the runs of the last call: d_pb_start and d_pb_value grow together, d_pb_value last:
    DevArr<int32_t> d_pb_value;                                // its capacity is PbJob::cap
    double pb_secs[4] = {0, 0, 0, 0};                          // gd_perbase_runs: count, scan, emit, read-back of the last call
    DevArr<uint8_t> d_dist;                                    // gd_depth_hist, gd_region_bins: the region and chunk tables and the counts of the last call (grow-only; gd_api_dist.inc)
    double dist_secs[3] = {0, 0, 0};                           // ... its upload, kernel and read-back
    double em_secs[3] = {0, 0, 0};                             // gd_emdepth*: upload, kernel, read-back of the last call (gd_api_emdepth.inc)
    PinArr<uint8_t> h_walk;                                    // gd_ingest_decode, gd_covstats_decode: per-segment tables of the record walk (page-locked host memory
                                                               // the walk kernels read and write over the link: no copy command)
    PinArr<uint32_t> h_ingest;                                 // page-locked: d_ingest's words as the host reads them (gd_copy_words_kernel)
    DevArr<uint8_t> d_seq;                             // gd_seq_load: one contig's bases, zero padded
    int64_t seq_len = -1;
    uint32_t seq_padded = 0;

    int64_t* export_buf = nullptr;     // gd_set_export: caller-owned device buffer, written by every gd_compute
    int64_t export_max_w = 0, export_cap_b = 0;

    // gd_comm_init: one RCCL communicator per context (gd_api_comm.inc)
    void* comm = nullptr;
    int comm_rank = 0, comm_world = 0;
    Event comm_ev[3];                                      // [0], [1]: the last two gathers; [2]: "computed so far"
    unsigned comm_seq = 0;
    const int64_t* comm_last_send = nullptr;   // the buffer the last gd_gather_export reads (it may still be reading it)
    unsigned comm_last_ev = 0;                 // ... and which of comm_ev[0 / 1] is recorded behind it

    ComputeState cs;
    bool computed = false;
    int64_t n_tiles = 0, n_win_total = 0, n_bases = 0;
    std::vector<int2> bounds;             // ordered run boundaries of the last compute
    gd_stats stats{};

    bool profiling = false;
    Event ev[GD_K_COUNT + 1];
    float kernel_ms[GD_K_COUNT] = {};
};

namespace {

thread_local bool tl_ingest_feeder = false;              // this thread is a context's reader thread (gd_ingest_feed_fd)

int fail(gd_ctx* c, int code, const char* fmt, ...)
{
    if (c) {
        char buf[512];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof buf, fmt, ap);
        va_end(ap);
        // the read of a pending range runs on a thread of the context (gd_ingest_feed_fd) beside the caller's own
        // calls: its failures are kept apart and published when the read is joined (ingest_join)
        if (tl_ingest_feeder) c->ing_feeder_err = buf;
        else c->err = buf;
    }
    return code;
}

// Whatever changes what a launched compute reads (records, contigs, parameters, path, outputs, options) is refused
// until gd_compute_finish.  A null context passes: the caller's own argument check answers that.
int in_flight(gd_ctx* c)
{
    return c && c->cs.pending ? fail(c, GD_E_STATE, "a compute is in flight: gd_compute_finish first") : GD_OK;
}

#define HIPCHK(ctx, call)                                                              \
    do {                                                                               \
        hipError_t e_ = (call);                                                        \
        if (e_ != hipSuccess)                                                          \
            return fail((ctx), e_ == hipErrorOutOfMemory ? GD_E_NOMEM : GD_E_HIP,      \
                        "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_),         \
                        __FILE__, __LINE__);                                           \
    } while (0)

// One device buffer of one call, freed when the call returns however it returns.  Never allocated: as() is null.
// (A DevArr of bytes whose alloc reports through the context, as every per-call buffer's did: it stays for that.)
struct DevBuf : DevArr<uint8_t> {
    int alloc(gd_ctx* c, size_t bytes) { HIPCHK(c, DevArr<uint8_t>::alloc(bytes)); return GD_OK; }
};

// Its companion for a call whose number of buffers is only known as it runs: all freed on return.
struct DevList {
    std::vector<DevBuf> v;
    // *out = count elements (at least one), zeroed on the context's stream when asked for
    template <typename T>
    int alloc(gd_ctx* c, T** out, size_t count, bool zero = false)
    {
        const size_t bytes = (count ? count : 1) * sizeof(T);
        v.emplace_back();
        if (int r = v.back().alloc(c, bytes)) return r;
        *out = v.back().template as<T>();
        if (zero) HIPCHK(c, hipMemsetAsync(*out, 0, bytes, c->stream));
        return GD_OK;
    }
};

// Exactly `ncap` elements for a device array the context keeps; with keep, the first `used` stay.  The new block first,
// then the copy on the copy stream, then a wait for both of the context's streams, then the old block goes.
template <typename Tp>
int regrow_dev(gd_ctx* c, DevArr<Tp>& a, size_t ncap, bool keep, size_t used)
{
    DevArr<Tp> nb;                               // (freed again when the copy or a synchronisation fails)
    HIPCHK(c, nb.alloc(ncap));
    if (a) {
        if (keep && used)
            HIPCHK(c, hipMemcpyAsync(nb.get(), a.get(), used * sizeof(Tp), hipMemcpyDeviceToDevice, c->copy_stream));
        HIPCHK(c, hipStreamSynchronize(c->copy_stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, a.reset_checked());
    }
    a = std::move(nb);                           // (onto an empty owner: no second free)
    return GD_OK;
}

// Room for `need` elements in such an array: grow-only, by half at least.
template <typename Tp>
int ensure_dev(gd_ctx* c, DevArr<Tp>& a, size_t need, bool keep = false, size_t used = 0)
{
    if (need <= a.cap() && a) return GD_OK;
    return regrow_dev(c, a, std::max(need, a.cap() + a.cap() / 2), keep, used);
}

// A state kept across calls (gd_ctx::cov, ic, isp, ec) goes: not before the kernels that read its arrays have ended.
template <class S>
void drop_state(gd_ctx* c, std::unique_ptr<S>& s)
{
    if (s) (void)hipStreamSynchronize(c->stream);
    s.reset();
}

void drop_ck(ContigHost& h)
{
    h.ck_blk.reset();                  // (hipFree of the block, when this was its last user, waits for the device)
    h.lrec = nullptr; h.lfq = nullptr; h.dl = nullptr; h.pck = nullptr; h.ndel = nullptr;
    h.max_span = 0;
    h.n_dels = 0;
    h.ck_ok = false;
}

// Everything but the length starts over; what the contig owns is freed (adopted records are borrowed: they are not).
void free_contig(ContigHost& h)
{
    const int64_t length = h.length;
    h = ContigHost();
    h.length = length;
}

int64_t derive_step(const gd_params& p)
{
    if (p.step > 0) return p.step;
    // depth/depth.go:48,:132
    int64_t s = 10000000 / p.window_size;
    if (s < 1) s = 1;
    return s * p.window_size;
}

// (m, s) with floor(x / d) == (x * m) >> s for every x < 2^31 (1 <= d < 2^31):
// s = 31 + ceil(log2 d), m = ceil(2^s / d) < 2^32  (Granlund & Montgomery 1994, N = 31).
void magic_u31(uint32_t d, uint32_t* m, uint32_t* s)
{
    if (d == 0) d = 1;
    uint32_t l = 0;
    while (l < 31 && (1u << l) < d) ++l;
    const unsigned __int128 num = (unsigned __int128)1 << (31 + l);
    *m = (uint32_t)((num + d - 1) / d);
    *s = 31 + l;
}

int set_device(gd_ctx* c)
{
    HIPCHK(c, hipSetDevice(c->device));
    return GD_OK;
}

// The records are gone (gd_set_contigs, gd_reset): so are the blocks handed out before, the verdicts pending on committed
// ones, and what the context learnt from the records -- the look-back, the spans the index pass measured.
int forget_records_state(gd_ctx* c)
{
    for (auto& s : c->ring) s.held = false;
    c->commit_checks_pending = false;                      // (d_ingest is cleared below)
    c->computed = false;
    c->lookback = c->params.max_span_hint > 0 ? c->params.max_span_hint : kDefaultLookback;
    c->span_forces_long = false;
    HIPCHK(c, hipMemsetAsync(c->d_ingest, 0, 4 * sizeof(uint32_t), c->stream));   // spans of records that are gone
    HIPCHK(c, hipStreamSynchronize(c->stream));            // (the next block's index pass runs on the copy stream: not before this)
    c->ingest_span = 0;
    c->ingest_span_dirty = false;
    return GD_OK;
}

void launch_prep(gd_ctx* c, const gd::Job& job)
{
    // one thread per tile; the same threads grid-stride over the window arrays (a thread per window made a 30x
    // genome's launch six rounds of workgroups, five of them doing 12 bytes of work per thread)
    int64_t work = std::max<int64_t>(job.n_tiles, std::min<int64_t>(job.n_win_total / 8, 1 << 20));
    int blocks = (int)((work + 255) / 256);
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(gd::gd_prep_kernel, dim3(blocks), dim3(256), 0, c->stream, job);
}

// The per-base store mode of a tile kernel (its OPT / ST template parameter), chosen at launch: f gets it as a
// compile-time constant -- 2: no per-base output, 1: non-temporal stores (GD_OPT_NT_STORES), 0: plain stores.
template <class F>
void with_store_mode(const gd_ctx* c, F&& f)
{
    if (!c->keep_perbase) f(std::integral_constant<int, 2>{});
    else if (c->tile_opt & 1) f(std::integral_constant<int, 1>{});
    else f(std::integral_constant<int, 0>{});
}

void launch_tile(gd_ctx* c, const gd::Job& job, int route)
{
    // 8 XCDs: the grid is 8 equal slices of the tile list (see the kernel)
    const unsigned grid = (unsigned)(((job.n_tiles + 7) / 8) * 8);
    const dim3 block(gd::shape::NT);
    if (route == GD_TK_TILE_SUMS) {
        hipLaunchKernelGGL(gd::gd_tile_sums_kernel, dim3(grid), block, 0, c->stream, job);
        return;
    }
    with_store_mode(c, [&](auto m) {
        constexpr int M = decltype(m)::value;
        if (route == GD_TK_GENERIC) {
            hipLaunchKernelGGL(gd::gd_tile_kernel<M>, dim3(grid), block, 0, c->stream, job);
            return;
        }
        // GD_TK_FAST_RAW.  Ordinary tiles: the straight-line kernel; the tiles gd_prep_kernel listed as `slow` (clipped
        // at a contig end, deeper than one batch of reads, more ops than the staging area): the generic one
        // The slow list (a few dozen workgroups of a large, cold kernel) goes FIRST: launched after the
        // straight-line kernel it took ~0.1 ms -- as long as all of chr20's ordinary tiles -- behind the
        // write-back of that kernel's per-base stores; in front of it, it costs a few microseconds
        // (profiles/r02d_slow_first.txt; a side stream next to the straight-line kernel bought nothing).
        const unsigned sgrid = c->slow_grid;                 // strides over the slow list (usually one tile per contig)
        hipLaunchKernelGGL(gd::gd_tile_slow_kernel<M>, dim3(sgrid), block, 0, c->stream, job);
        hipLaunchKernelGGL(gd::fast::gd_tile_fast_kernel<M>, dim3(grid), block, 0, c->stream, job);
    });
}

void launch_ltile(gd_ctx* c, const gd::Job& job)
{
    const unsigned grid = (unsigned)(((job.n_tiles + 7) / 8) * 8);
    with_store_mode(c, [&](auto m) {
        constexpr int M = decltype(m)::value == 1 ? 0 : decltype(m)::value;   // (built with plain stores and with none)
        hipLaunchKernelGGL(gd::gd_ltile2_kernel<M>, dim3(grid), dim3(gd::shape::NT), 0, c->stream, job);
    });
}

// The class runs of every tile, in genome order (every route but the sums-only ones ends with it).
void launch_runs_order(gd_ctx* c, const gd::Job& job)
{
    hipLaunchKernelGGL(gd::gd_runs_order_kernel, dim3((unsigned)((c->n_tiles + gd::SUPER - 1) / gd::SUPER)), dim3(gd::SUPER), 0,
                       c->stream, c->d_chunks, job.run_cap, c->d_tile_cnt, c->d_tile_off, c->d_super_cnt, c->d_ordered,
                       (int)c->n_tiles);
}

// In-place exclusive scan of v[0..n) on the compute stream, v[n] = total (v has n + 1 elements).
int launch_scan(gd_ctx* c, uint32_t* v, uint32_t n)
{
    if (n <= 4u * gd::SCAN_BLOCK) {
        hipLaunchKernelGGL(gd::gd_unit_scan_kernel, dim3(1), dim3(1024), 0, c->stream, v, n);
        return GD_OK;
    }
    const uint32_t nb = (n + gd::SCAN_BLOCK - 1u) / gd::SCAN_BLOCK;
    if (int r = ensure_dev(c, c->d_scan_tmp, (size_t)nb + 1)) return r;
    hipLaunchKernelGGL(gd::gd_scan_totals_kernel, dim3(nb), dim3(256), 0, c->stream, v, n, c->d_scan_tmp);
    hipLaunchKernelGGL(gd::gd_unit_scan_kernel, dim3(1), dim3(1024), 0, c->stream, c->d_scan_tmp, nb);
    hipLaunchKernelGGL(gd::gd_scan_apply_kernel, dim3(nb), dim3(256), 0, c->stream, v, n, c->d_scan_tmp, nb);
    return GD_OK;
}

// ---- derived record arrays, built per BATCH of contigs ----------------------------------------------------
// Bump allocation inside one block: every array starts on a 256-byte boundary.
struct Carve {
    size_t at = 0;
    size_t take(size_t bytes) { const size_t o = at; at += (bytes + 255) & ~(size_t)255; return o; }
};

// A block of at least `need` bytes: `keep` (what the batch's contigs held before) when nobody else uses it and it
// is large enough -- a re-normalisation of the same contigs allocates nothing -- else a new allocation.
int batch_block(gd_ctx* c, BlockRef keep, size_t need, BlockRef* out)
{
    if (keep && keep.use_count() == 1 && keep->cap() >= need) { *out = std::move(keep); return GD_OK; }
    keep.reset();
    BlockRef b = std::make_shared<DevArr<uint8_t>>();
    const auto ta = std::chrono::steady_clock::now();
    HIPCHK(c, b->alloc(need));
    // (a first large allocation can wait for the driver to clear memory another process -- or this one -- just released:
    // 0.4 ms on one box, half a second on another; gd_compute_timing reports it with the other device allocations)
    c->alloc_in_enqueue += std::chrono::duration<double>(std::chrono::steady_clock::now() - ta).count();
    *out = std::move(b);
    return GD_OK;
}

int batch_host(gd_ctx* c, size_t words)
{
    if (words <= c->h_batch.cap() && c->h_batch) return GD_OK;
    c->h_batch.reset();
    HIPCHK(c, c->h_batch.alloc(std::max<size_t>(words, 256)));
    return GD_OK;
}

// Long-read path: deletion lists, read records and tile indexes (gd_chunk.hpp) of a batch of contigs, straight from the
// records as they arrived: ONE allocation sized from the record counts alone (deletion lists: half the ops + a slot per
// read; tile indexes: an entry per 64 ops + three per read -- gd_chunk.hpp pt_slot), ONE pass (gd_dels_raw_kernel fills the
// index as it walks), one small kernel that puts every contig's deletion total and largest span into page-locked memory.
struct CkPending {
    std::vector<ContigHost*> hs;
    BlockRef blk;
    size_t o_jobs = 0, o_tot = 0;
    std::vector<size_t> o_lrec, o_lfq, o_dl, o_ndel, o_pck;
    uint32_t n_units = 0;
    gd::DelBatch B{};
};

int ck_enqueue(gd_ctx* c, const std::vector<ContigHost*>& hs, CkPending* P)
{
    P->hs = hs;
    const size_t nj = hs.size();
    if (nj == 0) return GD_OK;
    BlockRef keep = hs[0]->ck_blk;
    for (ContigHost* h : hs) drop_ck(*h);
    Carve cv;
    uint64_t units = 0;
    P->o_lrec.resize(nj); P->o_lfq.resize(nj); P->o_dl.resize(nj); P->o_ndel.resize(nj); P->o_pck.resize(nj);
    for (size_t k = 0; k < nj; ++k) {
        const ContigHost& h = *hs[k];
        const size_t n = h.n_reads;
        const size_t n_dl = (h.n_ops >> 1) + n + 1;
        const size_t n_pck = (h.n_ops >> 6) + 3 * n + 4;      // (< 2^32: at most 2^30 reads and 2^32 ops per contig)
        if (n_dl > 0xffffffffull) return fail(c, GD_E_RANGE, "too many deletions on one contig");
        P->o_lrec[k] = cv.take((n + 2) * sizeof(uint4));
        P->o_lfq[k] = cv.take((n + 1) * sizeof(uint32_t));
        P->o_ndel[k] = cv.take((n + 1) * sizeof(uint32_t));
        P->o_dl[k] = cv.take(n_dl * sizeof(uint2));
        P->o_pck[k] = cv.take(n_pck * sizeof(uint32_t));
        units += (n + 63) / 64;
    }
    if (units > (1ull << 26) - 64) return fail(c, GD_E_RANGE, "too many records in one batch (internal error)");
    P->n_units = (uint32_t)units;
    P->o_jobs = cv.take(nj * sizeof(gd::DelJob) + (nj + 1) * sizeof(uint32_t));   // the jobs, then ubeg
    P->o_tot = cv.take(2 * nj * sizeof(uint32_t));               // [deletions x n][largest spans x n]
    if (int r = batch_block(c, std::move(keep), cv.at, &P->blk)) return r;
    char* const base = P->blk->as<char>();
    // job table (host copy kept in the context until the next batch)
    c->batch_tab_ck.assign(nj * sizeof(gd::DelJob) + (nj + 1) * sizeof(uint32_t), 0);
    gd::DelJob* jobs = reinterpret_cast<gd::DelJob*>(c->batch_tab_ck.data());
    uint32_t* ubeg = reinterpret_cast<uint32_t*>(c->batch_tab_ck.data() + nj * sizeof(gd::DelJob));
    uint32_t u = 0;
    for (size_t k = 0; k < nj; ++k) {
        ContigHost& h = *hs[k];
        const uint32_t n = (uint32_t)h.n_reads, nu = (n + 63u) / 64u;
        gd::DelJob& j = jobs[k];
        j.pos = h.pos; j.flag = h.flag; j.mapq = h.mapq;
        j.off = h.off;
        j.cigar = h.cigar;
        j.n_reads = n; j.n_units = nu;
        j.lrec = reinterpret_cast<uint4*>(base + P->o_lrec[k]);
        j.lfq = reinterpret_cast<uint32_t*>(base + P->o_lfq[k]);
        j.dl = reinterpret_cast<uint2*>(base + P->o_dl[k]);
        j.ndel = reinterpret_cast<uint32_t*>(base + P->o_ndel[k]);
        j.max_span = reinterpret_cast<int32_t*>(j.lrec + n + 1);
        j.pck = reinterpret_cast<uint32_t*>(base + P->o_pck[k]);
        j.total = reinterpret_cast<uint32_t*>(base + P->o_tot) + k;
        ubeg[k] = u;
        u += nu;
    }
    ubeg[nj] = u;
    HIPCHK(c, hipMemcpyAsync(base + P->o_jobs, c->batch_tab_ck.data(), c->batch_tab_ck.size(), hipMemcpyHostToDevice, c->stream));
    static_assert(sizeof(gd::DelJob) % 8 == 0, "the ubeg table follows the jobs");
    gd::DelBatch& B = P->B;
    B.jobs = reinterpret_cast<const gd::DelJob*>(base + P->o_jobs);
    B.ubeg = reinterpret_cast<const uint32_t*>(base + P->o_jobs + nj * sizeof(gd::DelJob));
    B.n_jobs = (uint32_t)nj; B.n_units = P->n_units;
    for (size_t k = 0; k < nj; ++k)                          // lrec[n], lrec[n + 1] (the span accumulator)
        HIPCHK(c, hipMemsetAsync(base + P->o_lrec[k] + hs[k]->n_reads * sizeof(uint4), 0, 2 * sizeof(uint4), c->stream));
    HIPCHK(c, hipMemsetAsync(base + P->o_tot, 0, nj * sizeof(uint32_t), c->stream));   // (gd_ptile_totals_kernel writes the spans)
    if (P->n_units)
        hipLaunchKernelGGL(gd::gd_dels_raw_kernel, dim3((P->n_units + 3u) / 4u), dim3(256), 0, c->stream, B);
    hipLaunchKernelGGL(gd::gd_ptile_totals_kernel, dim3((unsigned)((nj + 255) / 256)), dim3(256), 0, c->stream, B);
    HIPCHK(c, hipGetLastError());
    return GD_OK;
}

// host words the totals of a ck batch take in gd_ctx::h_batch: [n_jobs deletion counts][n_jobs spans]
int ck_readback(gd_ctx* c, const CkPending& P, uint32_t* dst)
{
    const size_t nj = P.hs.size();
    if (nj == 0) return GD_OK;
    char* const base = P.blk->as<char>();
    // (dst is page-locked: a one-wave kernel stores the 2 n words there -- no copy commands; there used to be 1 + n of them)
    hipLaunchKernelGGL(gd::gd_copy_words_kernel, dim3(1), dim3(64), 0, c->stream, reinterpret_cast<const uint32_t*>(base + P.o_tot), dst,
                       (uint32_t)(2 * nj));
    HIPCHK(c, hipGetLastError());
    return GD_OK;
}

// after the synchronisation: publish (the spans are the look-back of the tile table)
int ck_finish(gd_ctx* c, CkPending& P, const uint32_t* tot)
{
    const size_t nj = P.hs.size();
    if (nj == 0) return GD_OK;
    gd::DelJob* jobs = reinterpret_cast<gd::DelJob*>(c->batch_tab_ck.data());
    for (size_t k = 0; k < nj; ++k) {
        ContigHost& h = *P.hs[k];
        h.ck_blk = P.blk;
        h.lrec = jobs[k].lrec; h.lfq = jobs[k].lfq; h.dl = jobs[k].dl; h.pck = jobs[k].pck; h.ndel = jobs[k].ndel;
        h.max_span = (int32_t)tot[nj + k];
        h.n_dels = tot[k];
        h.ck_ok = true;
    }
    return GD_OK;
}

// Builds the long-read structures of a batch of contigs.
int ck_batch(gd_ctx* c, const std::vector<ContigHost*>& hs)
{
    if (hs.empty()) return GD_OK;
    HIPCHK(c, hipEventRecord(c->copy_done, c->copy_stream));
    HIPCHK(c, hipStreamWaitEvent(c->stream, c->copy_done, 0));
    if (c->profiling) HIPCHK(c, hipEventRecord(c->ev[6], c->stream));
    CkPending P;
    if (int r = ck_enqueue(c, hs, &P)) return r;
    if (int r = batch_host(c, 2 * hs.size())) return r;
    if (int r = ck_readback(c, P, c->h_batch)) return r;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (int r = ck_finish(c, P, c->h_batch)) return r;
    if (c->profiling) {
        HIPCHK(c, hipEventRecord(c->ev[7], c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        float ms = 0;
        HIPCHK(c, hipEventElapsedTime(&ms, c->ev[6], c->ev[7]));
        c->kernel_ms[GD_K_CKPT] += ms;
    }
    return GD_OK;
}

// ---- the route of a gd_compute ------------------------------------------------------------------------------
// Which device algorithm and which tile kernel a job runs: the GD_TK_* value gd_stats.tile_kernel reports, or
// GD_E_INVALID.  This is the one statement of the rule; everything else -- long-read or scatter
// launch sequence, sums-only, Job::fast, gd_stats.path, the kernel launch_tile launches -- is read off its answer.
// Under GD_PATH_AUTO the answer can change between two attempts of one compute (span_forces_long).

// May the straight-line tile kernel and the streaming sums kernel run at all?  (They still need aligned arrays;
// compute_prepare allocates the straight-line kernel's tile table on this.)
bool straight_line_allowed(const gd_ctx* c)
{
    return c->fast_kernel && (c->path == GD_PATH_TILE || c->path == GD_PATH_AUTO);
}

int compute_route(const gd_ctx* c, const ComputeState& S)
{
    if (c->path == GD_PATH_SCATTER) return c->keep_perbase ? GD_TK_SCATTER : GD_E_INVALID;
    if (c->path == GD_PATH_CHUNK || (c->path == GD_PATH_AUTO && (c->span_forces_long || S.n_ops > 6 * S.n_reads)))
        return GD_TK_LONG;                                   // (sums-only is ignored: minima and runs are produced)
    // The straight-line kernels read the records as they arrived (no pass over the records before the first -- usually
    // the only -- compute of an input); contig arrays their vector loads cannot take: the generic kernels.
    const bool straight = straight_line_allowed(c) && S.raw_aligned;
    // sums-only: built for the default tile shape; W < 32 (more windows per tile than the LDS accumulators hold) keeps
    // the regular windows-only kernels, as documented
    if (c->sums_only && c->params.window_size >= 32)         // one streaming pass over the records, no tiles, where it can
        return straight && S.n_groups <= 0xfffffff0ull ? GD_TK_SUMS_STREAM_RAW : GD_TK_TILE_SUMS;
    return straight ? GD_TK_FAST_RAW : GD_TK_GENERIC;
}

bool route_sums_only(int route) { return route == GD_TK_TILE_SUMS || route == GD_TK_SUMS_STREAM_RAW; }

int route_path(int route)
{
    return route == GD_TK_LONG ? GD_PATH_CHUNK : route == GD_TK_SCATTER ? GD_PATH_SCATTER : GD_PATH_TILE;
}

// The long-read structures of the listed contigs that lack them, straight from the records as they arrived.
int ck_tids(gd_ctx* c, const std::vector<int32_t>& tids)
{
    // A launch holds fewer than 2^32 work-items (the dispatch packet's grid size is 32 bits; a larger grid wraps
    // silently): at one wave per 64-read unit that is 2^26 units, so a very large job is several batches.
    constexpr uint64_t kMaxUnits = 48u << 20;
    std::vector<ContigHost*> part;
    uint64_t units = 0;
    auto flush = [&]() -> int {
        if (part.empty()) return GD_OK;
        const int r = ck_batch(c, part);
        part.clear(); units = 0;
        return r;
    };
    for (int32_t tid : tids) {
        ContigHost& h = c->contigs[tid];
        if (h.length <= 0 || h.ck_ok) continue;
        if (!part.empty() && units + (h.n_reads + 63) / 64 > kMaxUnits)
            if (int r = flush()) return r;
        units += (h.n_reads + 63) / 64;
        part.push_back(&h);
    }
    return flush();
}

}  // namespace

struct IngestState {
    static constexpr size_t kStage = 64u << 20;        // bytes per page-locked staging buffer
    uint64_t n_bytes = 0, fed = 0, total = 0;           // compressed bytes announced / received, inflated bytes
    uint64_t base = 0;                                  // file offset of the range
    size_t nm = 0, next = 0;                            // members, first member not yet handed to the inflate kernel
    std::vector<uint64_t> m_coff, m_end, out_off;       // file offset, end offset in the range, offset in the inflated bytes
    std::vector<uint32_t> out_len;
    IngestBufs* bufs = nullptr;                         // one of gd_ctx::ing_bufs
    uint8_t *d_in = nullptr, *d_out = nullptr;
    uint64_t *t_in_off = nullptr, *t_out_off = nullptr;
    uint32_t *t_in_len = nullptr, *t_out_len = nullptr, *t_status = nullptr, *t_crc = nullptr;
    // One lane inflates one member start to end (~0.04 s whatever the member count), so the members are
    // handed to the kernel in at most kBatches launches, each on its own stream: they overlap each other
    // and the upload of the bytes still to come.
    static constexpr int kBatches = 8;
    int n_launch = 0;
    std::vector<gd_own::Event> inf_done;                // one per inflate launch of THIS range
    bool inflated = false;                              // every member inflated and its status checked
    ~IngestState() { if (bufs) bufs->busy = false; }
};
