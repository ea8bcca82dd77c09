// gd_api.hip -- C ABI of the per-base depth engine (include/goleft_depth.h).
//
// Host-side runtime around the CDNA4 kernels of gd_kernels.hpp, one translation unit.  This file: status strings,
// gd_create, the setters (stream, parameters, path, outputs, contigs, selection), options, statistics and timing; then
// the gd_api_*.inc files with the rest of the ABI, in this order: records (pinned staging ring + copy stream, records
// host -> HBM, HBM-resident per-contig record streams), compute (route, launch sequencing, look-back), results
// (read-back), aux, ingest, covstats, index, indexcov, indexsplit, crai, devmat, emdepth, emcnv, colselect, chunkdebias,
// movdebias, svddebias, cnveval, perbase, dist, comm; and behind them, where every kept state is a complete type, gd_destroy.  What the
// context holds is owned by its members (gd_own.hpp, gd_api_state.hpp): gd_destroy is the order of the teardown, the
// context's destructor the inventory.
// Replaces gargs' process.Runner + the samtools child + the callback's parse loop of `goleft depth`
// (depth/depth.go:392-394, :45, :282-325).
#include "../../include/goleft_depth.h"
#include "gd_kernels.hpp"
#include "gd_matcheck.hpp"
#include "gd_eigh.hpp"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <condition_variable>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include <unistd.h>

#include "gd_api_state.hpp"

extern "C" {

const char* gd_strerror(int s)
{
    switch (s) {
    case GD_OK: return "ok";
    case GD_E_INVALID: return "invalid argument";
    case GD_E_NOMEM: return "out of memory";
    case GD_E_HIP: return "HIP runtime error";
    case GD_E_STATE: return "call out of order";
    case GD_E_RANGE: return "tid or coordinate out of range";
    case GD_E_NODEVICE: return "no usable HIP device";
    case GD_E_UNSORTED: return "records not coordinate sorted";
    case GD_E_CAPACITY: return "output buffer too small";
    }
    return "unknown status";
}

int gd_abi_version(void) { return GD_ABI_VERSION; }
int gd_abi_revision(void) { return GD_ABI_REVISION; }

int gd_device_count(int* n)
{
    if (!n) return GD_E_INVALID;
    int k = 0;
    hipError_t e = hipGetDeviceCount(&k);
    if (e != hipSuccess) { *n = 0; return GD_E_NODEVICE; }
    *n = k;
    return GD_OK;
}

int gd_default_params(gd_params* p)
{
    if (!p) return GD_E_INVALID;
    // depth/depth.go:164-167
    p->window_size = 250;
    p->min_mapq = 1;
    p->min_cov = 4;
    p->max_mean_depth = 0;
    p->flag_mask = GD_DEFAULT_FLAG_MASK;
    p->max_span_hint = 0;
    p->step = 0;
    return GD_OK;
}

int gd_create(int device_id, gd_ctx** out)
{
    if (!out) return GD_E_INVALID;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return GD_E_NODEVICE;
    if (device_id < 0 || device_id >= n) return GD_E_RANGE;
    gd_ctx* c = new (std::nothrow) gd_ctx();
    if (!c) return GD_E_NOMEM;
    c->device = device_id;
    gd_default_params(&c->params);
    auto bail = [&](hipError_t e) {
        (void)e;
        gd_destroy(c);
        return GD_E_HIP;
    };
    hipError_t e;
    if ((e = hipSetDevice(device_id)) != hipSuccess) return bail(e);
    if ((e = c->stream.create(hipStreamNonBlocking)) != hipSuccess) return bail(e);
    if ((e = c->copy_stream.create(hipStreamNonBlocking)) != hipSuccess) return bail(e);
    if ((e = c->copy_done.create(hipEventDisableTiming)) != hipSuccess) return bail(e);
    for (auto& s : c->ring)
        if ((e = s.done.create(hipEventDisableTiming)) != hipSuccess) return bail(e);
    for (auto& ev : c->ev)
        if ((e = ev.create(hipEventDefault)) != hipSuccess) return bail(e);
    if ((e = c->d_counters.alloc(1)) != hipSuccess) return bail(e);
    if ((e = c->d_region_cursor.alloc(1)) != hipSuccess) return bail(e);
    if ((e = c->h_counters.alloc(1)) != hipSuccess) return bail(e);
    if ((e = c->h_bounds.alloc(kSpecBounds)) != hipSuccess) return bail(e);
    if ((e = hipMemset(c->d_counters, 0, sizeof(gd::Counters))) != hipSuccess) return bail(e);
    if ((e = c->d_ingest.alloc(4)) != hipSuccess) return bail(e);
    if ((e = hipMemset(c->d_ingest, 0, 4 * sizeof(uint32_t))) != hipSuccess) return bail(e);
    if ((e = c->h_ingest.alloc(4)) != hipSuccess) return bail(e);
    // Warm-up: one compute of an EMPTY two-tile contig runs every kernel of the tile path once (prep, slow list, straight-
    // line tile kernel, run ordering, read-back) and makes the small fixed-size allocations -- the first launch of a kernel in
    // a process costs tens of microseconds that a job of chr20's size (0.14 ms a step) saw as 1.3 x in its first, usually
    // only, compute.  A context comes up on a thread of its own while the host reads the BAM header (0.2-0.3 s): the
    // millisecond belongs there.  Nothing of it stays: no contigs, no records, default look-back.
    // A warm-up that fails is a device that fails: the context is not handed out in a state the caller did not ask for (ADVICE
    // r5: a phantom contig, a cleared error).  GOLEFT_NO_WARMUP=1 skips it (tests that create contexts by the hundred).
    if (const char* nw = getenv("GOLEFT_NO_WARMUP"); !(nw && *nw == '1')) {
        const int64_t len = 2 * 4096;
        int rc = gd_set_contigs(c, 1, &len);
        if (rc == GD_OK) rc = gd_compute(c);
        const int rc2 = gd_set_contigs(c, 0, nullptr);
        if (rc != GD_OK || rc2 != GD_OK) {
            fprintf(stderr, "gd_create: the warm-up compute failed (%d / %d): %s\n", rc, rc2, c->err.c_str());
            gd_destroy(c);
            return rc != GD_OK ? rc : rc2;
        }
        c->stats = gd_stats{};
        for (double& t : c->timing) t = 0;
    }
    *out = c;
    return GD_OK;
}

const char* gd_last_error(const gd_ctx* c) { return c ? c->err.c_str() : "null context"; }

int gd_set_stream(gd_ctx* c, void* s)
{
    if (!c) return GD_E_INVALID;
    if (int r = set_device(c)) return r;
    if (c->stream.owned() && c->stream) HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, c->stream.reset_checked());                // (a caller's stream is let go of, never destroyed)
    if (s) c->stream.borrow(static_cast<hipStream_t>(s));
    else HIPCHK(c, c->stream.create(hipStreamNonBlocking));
    return GD_OK;
}

int gd_set_params(gd_ctx* c, const gd_params* p)
{
    if (int r = in_flight(c)) return r;
    if (!c || !p) return GD_E_INVALID;
    if (p->window_size < 1) return fail(c, GD_E_INVALID, "window_size must be >= 1");
    if (p->step < 0) return fail(c, GD_E_INVALID, "step must be >= 0");
    if (p->step > 0 && p->step % p->window_size != 0)
        return fail(c, GD_E_INVALID, "step must be a multiple of window_size");
    c->params = *p;
    if (p->max_span_hint > 0) { c->lookback = p->max_span_hint; c->lookback_pinned = true; }
    else c->lookback_pinned = false;
    c->computed = false;
    return GD_OK;
}

int gd_set_path(gd_ctx* c, int path)
{
    if (int r = in_flight(c)) return r;
    if (!c) return GD_E_INVALID;
    if (path != GD_PATH_AUTO && path != GD_PATH_TILE && path != GD_PATH_SCATTER && path != GD_PATH_CHUNK)
        return fail(c, GD_E_INVALID, "unknown path %d", path);
    c->path = path;
    c->computed = false;
    return GD_OK;
}

int gd_set_outputs(gd_ctx* c, unsigned flags)
{
    if (int r = in_flight(c)) return r;
    if (!c) return GD_E_INVALID;
    if (flags & ~(unsigned)(GD_OUT_PERBASE | GD_OUT_SUMS_ONLY)) return fail(c, GD_E_INVALID, "unknown output flags 0x%x", flags);
    if ((flags & GD_OUT_PERBASE) && (flags & GD_OUT_SUMS_ONLY))
        return fail(c, GD_E_INVALID, "GD_OUT_SUMS_ONLY excludes GD_OUT_PERBASE");
    c->keep_perbase = (flags & GD_OUT_PERBASE) != 0;
    c->sums_only = (flags & GD_OUT_SUMS_ONLY) != 0;
    c->computed = false;
    return GD_OK;
}

int gd_set_contigs(gd_ctx* c, int n, const int64_t* lengths)
{
    if (int r = in_flight(c)) return r;
    if (!c || n < 0 || (n > 0 && !lengths)) return GD_E_INVALID;
    if (int r = set_device(c)) return r;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipStreamSynchronize(c->copy_stream));
    c->contigs.clear();                                    // (frees what the contigs own)
    c->contigs.resize(n);
    for (int i = 0; i < n; ++i) {
        if (lengths[i] < 0 || lengths[i] > GD_MAX_CONTIG_LENGTH)
            return fail(c, GD_E_RANGE, "contig %d length %lld out of range", i, (long long)lengths[i]);
        c->contigs[i].length = lengths[i];
    }
    c->selected.clear();
    return forget_records_state(c);                        // a new data set
}

int gd_select_contigs(gd_ctx* c, int n, const int32_t* tids)
{
    if (int r = in_flight(c)) return r;
    if (!c || n < 0 || (n > 0 && !tids)) return GD_E_INVALID;
    std::vector<int32_t> s(tids, tids + n);
    for (int32_t t : s)
        if (t < 0 || (size_t)t >= c->contigs.size()) return fail(c, GD_E_RANGE, "tid %d out of range", t);
    std::sort(s.begin(), s.end());
    s.erase(std::unique(s.begin(), s.end()), s.end());
    c->selected.swap(s);
    c->computed = false;
    return GD_OK;
}

// What the retired options (include/goleft_depth.h) were at in every library that shipped.
static int retired_option_default(int option)
{
    return option == GD_OPT_INGEST_PIECE_STREAMS ? 1 : option == GD_OPT_INGEST_BATCHES ? 8 : 0;
}

int gd_set_option(gd_ctx* c, int option, int64_t value)
{
    if (int r = in_flight(c)) return r;
    if (!c) return GD_E_INVALID;
    switch (option) {
    case GD_OPT_NT_STORES: c->tile_opt = value ? 1 : 0; break;
    case GD_OPT_FAST_KERNEL: c->fast_kernel = value != 0; break;
    case GD_OPT_COPY_THREADS:
        if (value < 1 || value > 16) return fail(c, GD_E_INVALID, "copy threads: 1..16");
        c->ing_copy_threads = (int)value;
        break;
    case GD_OPT_H2D_KERNEL:
        if (value < 0 || value > 4096) return fail(c, GD_E_INVALID, "h2d kernel: 0 (hipMemcpyAsync) or its grid, 1..4096 workgroups");
        c->h2d_kernel = value != 0;
        if (value > 1) c->h2d_grid = (unsigned)value;
        break;
    case GD_OPT_INGEST_CRC: c->ingest_crc = value != 0; break;
    case GD_OPT_INGEST_DMA:
        if (value != 0 && value != 1) return fail(c, GD_E_INVALID, "ingest DMA: 1 (a copy command) or 0 (a copy kernel on a high-priority stream)");
        c->ing_copy_engine = value == 1;
        break;
    case GD_OPT_BAM_REFS:
        if (value < 0 || value > 0x7fffffff) return fail(c, GD_E_INVALID, "BAM references: 0 (unknown) .. 2^31 - 1");
        c->bam_n_ref = (int32_t)value;
        break;
    case GD_OPT_PUSH_CHUNK:
        if (value < 4096 || value > (1 << 24)) return fail(c, GD_E_INVALID, "push chunk: 4096 .. 2^24 records");
        c->push_chunk = (size_t)value;
        break;
    case GD_OPT_PUSH_THREADS:
        if (value < 1 || value > 64) return fail(c, GD_E_INVALID, "push threads: 1..64");
        c->push_threads = (int)value;
        break;
    case GD_OPT_INGEST_INDEX: c->ingest_index = value != 0; break;
    case GD_OPT_INGEST_COPY_GRID:
        if (value < 1 || value > 4096) return fail(c, GD_E_INVALID, "ingest copy grid: 1 .. 4096 workgroups");
        c->ing_copy_grid = (unsigned)value;
        break;
    case GD_OPT_COMMIT_CHECK:
        if (value != 0 && value != 1) return fail(c, GD_E_INVALID, "commit check: 0 (host, in gd_commit) or 1 (device, deferred)");
        c->commit_check_device = value == 1;
        break;
    case GD_OPT_INGEST_CU_SPLIT:
        if (value < 0 || value > 64 || value == 1) return fail(c, GD_E_INVALID, "ingest CU split: 0 (off) or 2 .. 64");
        if (c->ing_stream[0] || c->ing_hp) return fail(c, GD_E_STATE, "the ingest streams exist already: set GD_OPT_INGEST_CU_SPLIT before the first gd_ingest_begin");
        c->ing_cu_split = (int)value;
        break;
    case GD_OPT_INGEST_RANGE_HINT:
        if (value < 0) return fail(c, GD_E_INVALID, "ingest range hint: bytes >= 0");
        c->ing_range_hint = (uint64_t)value;
        break;
    case GD_OPT_INFLATE_KERNEL:
        if (value < 0 || value > 1) return fail(c, GD_E_INVALID, "inflate kernel: 0 (a lane per member) or 1 (a workgroup per member)");
        c->inflate_kernel = (int)value;
        break;
    case GD_OPT_MOVDEBIAS_SEGMENT:
        if (value < 0 || value > (1 << 30)) return fail(c, GD_E_INVALID, "moving debias segment: 0 (the default for the window) or 1 .. 2^30 sorted rows");
        c->md_segment = value;
        break;
    case GD_OPT_INDEX_SLICE:
        if (value < 64 || value > (1 << 30)) return fail(c, GD_E_INVALID, "index slice: 64 .. 2^30 bytes");
        c->idx_slice = value;
        break;
    case GD_OPT_INDEX_GUESS_CHECKS:
        if (value < 0 || value > 64) return fail(c, GD_E_INVALID, "index guess checks: 0 .. 64 records");
        c->idx_checks = (int)value;
        break;
    case GD_OPT_INDEX_REPAIR_ROUNDS:
        if (value < 0 || value > (1 << 20)) return fail(c, GD_E_INVALID, "index repair rounds: 0 .. 2^20");
        c->idx_repair_rounds = (int)value;
        break;
    // retired (include/goleft_depth.h): the number is reserved and only the default is accepted
    case GD_OPT_INGEST_PIECE_STREAMS: case GD_OPT_INFLATE_LDS_PAD: case GD_OPT_INGEST_HYBRID: case GD_OPT_INGEST_BATCHES:
    case GD_OPT_INGEST_WALK_CUS:
        if (value != retired_option_default(option))
            return fail(c, GD_E_INVALID, "option %d is retired: only its default, %d, is accepted", option, retired_option_default(option));
        break;
    default: return fail(c, GD_E_INVALID, "unknown option %d", option);
    }
    c->computed = false;
    return GD_OK;
}

int gd_get_option(gd_ctx* c, int option, int64_t* value)
{
    if (!c || !value) return GD_E_INVALID;
    switch (option) {
    case GD_OPT_NT_STORES: *value = c->tile_opt & 1; break;
    case GD_OPT_FAST_KERNEL: *value = c->fast_kernel; break;
    case GD_OPT_COPY_THREADS: *value = c->ing_copy_threads; break;
    case GD_OPT_H2D_KERNEL: *value = c->h2d_kernel ? (int64_t)std::max(1u, c->h2d_grid) : 0; break;
    case GD_OPT_INGEST_CRC: *value = c->ingest_crc; break;
    case GD_OPT_INGEST_DMA: *value = c->ing_copy_engine; break;
    case GD_OPT_BAM_REFS: *value = c->bam_n_ref; break;
    case GD_OPT_PUSH_CHUNK: *value = (int64_t)c->push_chunk; break;
    case GD_OPT_PUSH_THREADS: *value = c->push_threads; break;
    case GD_OPT_INGEST_INDEX: *value = c->ingest_index; break;
    case GD_OPT_COMMIT_CHECK: *value = c->commit_check_device; break;
    case GD_OPT_INGEST_COPY_GRID: *value = c->ing_copy_grid; break;
    case GD_OPT_INGEST_CU_SPLIT: *value = c->ing_cu_split; break;
    case GD_OPT_INGEST_RANGE_HINT: *value = (int64_t)c->ing_range_hint; break;
    case GD_OPT_INFLATE_KERNEL: *value = c->inflate_kernel; break;
    case GD_OPT_MOVDEBIAS_SEGMENT: *value = c->md_segment; break;
    case GD_OPT_INDEX_SLICE: *value = c->idx_slice; break;
    case GD_OPT_INDEX_GUESS_CHECKS: *value = c->idx_checks; break;
    case GD_OPT_INDEX_REPAIR_ROUNDS: *value = c->idx_repair_rounds; break;
    case GD_OPT_INGEST_PIECE_STREAMS: case GD_OPT_INFLATE_LDS_PAD: case GD_OPT_INGEST_HYBRID: case GD_OPT_INGEST_BATCHES:
    case GD_OPT_INGEST_WALK_CUS: *value = retired_option_default(option); break;
    default: return fail(c, GD_E_INVALID, "unknown option %d", option);
    }
    return GD_OK;
}

int gd_get_stats(gd_ctx* c, gd_stats* out)
{
    if (!c || !out) return GD_E_INVALID;
    *out = c->stats;
    return GD_OK;
}

int gd_compute_timing(gd_ctx* c, double* seconds, int n)
{
    if (!c || !seconds || n < 0) return GD_E_INVALID;
    for (int i = 0; i < n; ++i) seconds[i] = i < 4 ? c->timing[i] : 0.0;
    return GD_OK;
}

int gd_set_profiling(gd_ctx* c, int on)
{
    if (!c) return GD_E_INVALID;
    c->profiling = on != 0;
    c->kernel_ms[GD_K_CKPT] = 0;                        // accumulates over the contigs checkpointed from now on
    return GD_OK;
}

int gd_kernel_ms(gd_ctx* c, int id, float* ms)
{
    if (!c || !ms || id < 0 || id >= GD_K_COUNT) return GD_E_INVALID;
    *ms = c->kernel_ms[id];
    return GD_OK;
}

#include "gd_api_records.inc"
#include "gd_api_compute.inc"
#include "gd_api_results.inc"
#include "gd_api_aux.inc"
#include "gd_api_ingest.inc"
#include "gd_api_covstats.inc"
#include "gd_api_index.inc"
#include "gd_api_indexcov.inc"
#include "gd_api_indexsplit.inc"
#include "gd_api_crai.inc"
#include "gd_api_devmat.inc"
#include "gd_api_emdepth.inc"
#include "gd_api_emcnv.inc"
#include "gd_api_colselect.inc"
#include "gd_api_chunkdebias.inc"
#include "gd_api_movdebias.inc"
#include "gd_api_svddebias.inc"
#include "gd_api_cnveval.inc"
#include "gd_api_perbase.inc"
#include "gd_api_dist.inc"
#include "gd_api_comm.inc"

void gd_destroy(gd_ctx* c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->copy_stream) (void)hipStreamSynchronize(c->copy_stream);
    (void)gd_ingest_abort(c);      // joins the reader thread; the pending IngestStates go before the IngestBufs they point into
    drop_state(c, c->cov);
    drop_state(c, c->idx);
    drop_state(c, c->ic);
    drop_state(c, c->isp);
    drop_state(c, c->ec);
    (void)gd_comm_destroy(c);
    drop_pool(c);
    delete c;
}

}  // extern "C"

gd_ctx::gd_ctx() = default;
gd_ctx::~gd_ctx() = default;
