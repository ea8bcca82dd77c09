/*
 * goleft_depth.h -- C ABI of the MI355X-native per-base depth engine.
 *
 * This is the drop-in boundary for ONE path of brentp/goleft: the `depth`
 * subcommand (reference paths below are relative to /root/reference).
 * The reference has no FFI for this path: its seam is a subprocess per
 * 10 Mb tile -- `samtools depth -Q q -d D -r chr:s-e bam` spawned through
 * gargs `process.Runner` (depth/depth.go:45, :392-394) whose text output is
 * re-parsed by the `callback` closure (depth/depth.go:238-364).  This library
 * replaces that subprocess, the text pipe and the per-line parse; the host
 * keeps flags, tiling and BED formatting (INTEGRATION.md shows the cgo stub).
 *
 * Conventions
 *   - plain C: opaque context, plain pointers and sizes, no C++/torch types;
 *   - every call returns 0 (GD_OK) or a negative gd_status; the library never
 *     exits or aborts (the Go host folds failures into its exit code the way
 *     depth/depth.go:395-399 does);
 *   - the library never retains caller host pointers after a call returns
 *     (cgo rule); staging memory handed out by gd_acquire is library-owned
 *     pinned memory; device pointers given to gd_adopt_device stay owned by
 *     the caller and must outlive the context or the next gd_reset;
 *   - all results are integers (int32 per base, int64 window sums, int32
 *     window minima, {start,end,class} runs); `%.4g` and BED text stay on the
 *     host so results are bit-exact by construction;
 *   - coordinates are 0-based half-open; CIGARs use the BAM encoding
 *     (len<<4 | op, op in MIDNSHP=X = 0..8), i.e. biogo `sam.CigarOp` memory.
 *   - calls on one context must be serialised by the caller; distinct
 *     contexts (one per device / per producer thread) are independent.
 */
#ifndef GOLEFT_DEPTH_H
#define GOLEFT_DEPTH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* GD_ABI_VERSION changes when an existing entry point or structure changes; GD_ABI_REVISION counts the releases that only
 * ADDED entry points since then (revision 1: gd_indexcov_*; 2: gd_indexsplit_*; 3: gd_crai_sizes).  A caller built against (15, r) runs on any (15, r' >= r).
 * gd_emdepth, gd_emdepth_cells and gd_emdepth_timing, and after them gd_emcnv_*, gd_sample_medians*, gd_chunk_debias*, gd_device_scale, the *_device entries, gd_moving_debias*, gd_svd_debias* and gd_svd_debias_scaled*, were added without a revision; look them up by symbol.  So were gd_cnveval and gd_cnveval_timing.  So were gd_perbase_runs and gd_perbase_runs_timing.  So were gd_depth_hist, gd_region_bins and gd_dist_timing.
 * Why indexcov did not become version 16: nothing that existed changed, so callers of ABI 15 need not be turned away, and
 * tests/test_host_cpu.py holds gd_abi_version() to 15 until something does change. */
#define GD_ABI_VERSION 15
#define GD_ABI_REVISION 3

typedef enum {
    GD_OK = 0,
    GD_E_INVALID = -1,   /* bad argument */
    GD_E_NOMEM = -2,     /* host or device allocation failed */
    GD_E_HIP = -3,       /* a HIP runtime call failed (see gd_last_error) */
    GD_E_STATE = -4,     /* call out of order (e.g. results before compute) */
    GD_E_RANGE = -5,     /* tid / coordinate out of range */
    GD_E_NODEVICE = -6,  /* no usable gfx950 device */
    GD_E_UNSORTED = -7,  /* records not coordinate sorted within a contig */
    GD_E_CAPACITY = -8   /* caller buffer too small (needed size reported) */
} gd_status;

/* Coverage classes, depth/depth.go:223-234 getCovClass. */
enum { GD_NO_COVERAGE = 0, GD_LOW_COVERAGE = 1, GD_CALLABLE = 2, GD_EXCESSIVE_COVERAGE = 3 };

/* samtools depth default read filter UNMAP|SECONDARY|QCFAIL|DUP. */
#define GD_DEFAULT_FLAG_MASK 0x704u

typedef struct gd_ctx gd_ctx;

/* Mirrors the `dargs` fields that reach the arithmetic (depth/depth.go:27-41;
 * defaults depth/depth.go:164-167). */
typedef struct {
    int32_t  window_size;     /* --windowsize, default 250 */
    int32_t  min_mapq;        /* -Q, default 1 (samtools depth -Q) */
    int32_t  min_cov;         /* --mincov, default 4 */
    int32_t  max_mean_depth;  /* --maxmeandepth, default 0 (EXCESSIVE class off) */
    uint32_t flag_mask;       /* reads with flag & mask are dropped; 0x704 */
    int32_t  max_span_hint;   /* expected max reference span of a read (0 = default 512);
                                 only a performance hint: the engine verifies it on device
                                 and transparently re-runs with the observed maximum */
    int64_t  step;            /* callable runs are split at multiples of this
                                 (depth/depth.go:48,:132; quirk Q1); 0 = derive
                                 max(1,10000000/W)*W */
} gd_params;

/* One block of decoded records, SoA.  For gd_acquire the pointers are pinned
 * host memory owned by the library; for gd_adopt_device they are device
 * pointers owned by the caller. */
typedef struct {
    int32_t*  pos;        /* [reads_cap]   0-based leftmost position */
    uint16_t* flag;       /* [reads_cap]   BAM FLAG */
    uint8_t*  mapq;       /* [reads_cap]   MAPQ */
    uint32_t* cigar_off;  /* [reads_cap+1] CSR offsets into cigar[], block relative */
    uint32_t* cigar;      /* [ops_cap]     BAM-encoded CIGAR ops */
    size_t    reads_cap;
    size_t    ops_cap;
    int32_t   slot;       /* ring slot (library use) */
} gd_batch;

typedef struct {
    int32_t start;        /* 0-based */
    int32_t end;          /* exclusive */
    int32_t cls;          /* GD_NO_COVERAGE .. GD_EXCESSIVE_COVERAGE */
} gd_run;

typedef struct {
    uint64_t n_reads;        /* records resident on the device */
    uint64_t n_ops;          /* CIGAR ops resident on the device */
    uint64_t n_ref_bases;    /* sum of contig lengths computed */
    uint64_t n_windows;
    uint64_t n_tiles;        /* LDS tiles (= workgroups of the tile kernel) */
    uint64_t n_runs;         /* callable runs found */
    int32_t  tile_positions; /* reference positions per LDS tile */
    int32_t  lookback;       /* look-back span in use */
    int32_t  max_span_seen;  /* largest reference span among kept reads */
    int32_t  reruns;         /* times the last gd_compute re-ran (span / run capacity) */
    int32_t  path;           /* GD_PATH_TILE / _SCATTER / _CHUNK: what the last gd_compute ran */
    int32_t  n_slow_tiles;   /* tile path with GD_OPT_FAST_KERNEL: tiles that took the generic kernel instead */
    uint64_t n_canonical_ops; /* (ABI 13: ops of canonical CIGARs; always 0 since ABI 14 -- every path reads the original ops) */
    int32_t  tile_kernel;    /* GD_TK_*: the kernel that did the per-base arithmetic of the last gd_compute */
    int32_t  reserved_;
    uint64_t n_deletions;    /* long-read path: entries of the deletion lists the tile kernel read (8 bytes each) */
} gd_stats;

/* gd_stats.tile_kernel */
enum { GD_TK_NONE = 0,
       GD_TK_GENERIC = 1,      /* gd_tile_kernel: any tile shape, CIGARs in any form */
       GD_TK_FAST = 2,         /* (ABI 13: the straight-line kernel on canonical records; not reported since ABI 14) */
       GD_TK_FAST_RAW = 3,     /* gd_tile_fast_kernel on the records as they arrived (+ the slow list) */
       GD_TK_LONG = 4,         /* gd_ltile2_kernel (long-read path) */
       GD_TK_SCATTER = 5,      /* gd_expand_scatter_kernel + gd_scan_kernel */
       GD_TK_SUMS_STREAM = 6,  /* (ABI 13: the streaming sums kernel over canonical records; not reported since ABI 14) */
       GD_TK_TILE_SUMS = 7,    /* gd_tile_sums_kernel (GD_OUT_SUMS_ONLY otherwise) */
       GD_TK_SUMS_STREAM_RAW = 8 };  /* gd_sums_stream_kernel over the records as they arrived */

/* Kernel ids for gd_kernel_ms.  Tile path: PREP, TILE, RUNS.  Long-read path: PREP, TILE (the long-read tile
 * kernel), RUNS; CKPT = its deletion lists + tile indexes, built when the records arrive (like NORM: summed over
 * the contigs since gd_set_profiling was last called, not cleared by gd_compute).
 * Scatter path: PREP (zero-fill + init), EXPAND (CIGAR expand + scatter), SCAN
 * (in-place scan + window / class reductions), RUNS. */
enum { GD_K_PREP = 0, GD_K_TILE = 1, GD_K_RUNS = 2, GD_K_EXPAND = 3, GD_K_SCAN = 4, GD_K_CKPT = 5,
       GD_K_SEQSTATS = 6,   /* the kernel of the last gd_seq_stats */
       GD_K_MDFLAGS = 7,    /* the kernel of the last gd_md_flags */
       GD_K_INFLATE = 8,    /* the kernel of the last gd_inflate_bgzf */
       GD_K_NORM = 9,       /* CIGAR normalisation (gd_adopt_device, gd_ingest_finish, or the first gd_compute
                               after gd_commit): summed over the contigs normalised since gd_set_profiling
                               was last called; not cleared by gd_compute */
       GD_K_COUNT = 10 };

/* Device algorithm of gd_compute.  All are bit exact; they differ in cost.
 *   TILE     one workgroup per 4096-position tile re-walks the CIGARs of the
 *            reads that start within one maximum read span before it (LDS
 *            difference array, fused scan): the short-read path, ~6.5 HBM bytes
 *            per base;
 *   CHUNK    the same tile shape for long reads (ONT/PacBio, spliced): one pass
 *            over the CIGARs leaves a reference-position checkpoint every 64 ops
 *            and every read's end; a tile then expands only the 64-op chunks that
 *            reach it (LDS marks, no global atomics, any read span);
 *   SCATTER  every CIGAR op is expanded once and scattered with global integer
 *            atomics, then one in-place scan pass: no look-back at all, kept for
 *            pathological span distributions and as a cross-check;
 *   AUTO     CHUNK when records average more than 6 CIGAR ops or a read spans
 *            more than 32768 reference bases, else TILE (default). */
enum { GD_PATH_AUTO = 0, GD_PATH_TILE = 1, GD_PATH_SCATTER = 2, GD_PATH_CHUNK = 3 };

const char* gd_strerror(int status);
int         gd_abi_version(void);
int         gd_abi_revision(void);
int         gd_device_count(int* n);

/* Create a context bound to one HIP device (hipSetDevice is re-issued inside
 * every entry point, so calls may come from any OS thread / goroutine). */
int  gd_create(int device_id, gd_ctx** out);
void gd_destroy(gd_ctx* ctx);
const char* gd_last_error(const gd_ctx* ctx);

/* Optional: run all work on a caller-provided hipStream_t (passed as void*). */
int gd_set_stream(gd_ctx* ctx, void* hip_stream);

int gd_set_params(gd_ctx* ctx, const gd_params* p);
int gd_default_params(gd_params* p);
/* Choose the device algorithm (GD_PATH_*); default GD_PATH_AUTO. */
int gd_set_path(gd_ctx* ctx, int path);

/* Switches (defaults are what the measurements in DESIGN.md chose; results are bit identical under every setting).  A C
 * library behind cgo takes no behaviour from the process environment: these are calls.
 * (Numbers 1, 2, 4, 11 belonged to tile shapes and to "canonical records", measured slower / without a caller: retired.) */
enum { GD_OPT_NT_STORES = 3,        /* 1 (default): non-temporal per-base stores; 0: plain */
       GD_OPT_FAST_KERNEL = 5,      /* 1 (default): ordinary tiles run the straight-line tile kernel, the rest the
                                       generic one; 0: the generic kernel for every tile */
       GD_OPT_COPY_THREADS = 6,     /* host threads filling the staging buffer of gd_ingest_feed: 1 (default) .. 16 */
       GD_OPT_PUSH_THREADS = 7,     /* host threads of gd_push copying into a pinned ring block: 16 (default), 1 .. 64
                                       (one core moves ~11 GB/s into pinned memory; the link takes five times that) */
       GD_OPT_H2D_KERNEL = 8,       /* how a committed staging block reaches HBM: 1 (default) one kernel whose workgroups
                                       read the page-locked block over the link (all five arrays in one launch; n > 1:
                                       with n workgroups), 0: five hipMemcpyAsync through a DMA engine */
       GD_OPT_PUSH_CHUNK = 9,       /* records per staging block of gd_push: 2^20 (default), 4096 .. 2^24 */
       GD_OPT_BAM_REFS = 10,        /* gd_ingest_*: number of references in the BAM header (0, the default: unknown).  The
                                       record walk takes the first record of ANOTHER reference as the end of a contig's
                                       records only when its refID is one a sorted BAM can hold there (greater than the
                                       contig's and below this number, or -1); anything else is a damaged record */
       GD_OPT_INGEST_CRC = 12,      /* 1 (default): gd_ingest_* checks the CRC32 of every BGZF member after inflating it, as htslib
                                       does; 0: the file is trusted (a second pass over the inflated bytes is saved) */
       GD_OPT_INGEST_DMA = 13,      /* gd_ingest_feed*: how a staged piece crosses the link: 1 (default) a copy command on one stream;
                                       0: a copy kernel on a high-priority stream (what the CLI uses, with GD_OPT_INGEST_CU_SPLIT).
                                       (2 .. 4 were slices of a piece on several streams, measured slower and retired: GD_E_INVALID) */
       GD_OPT_INGEST_INDEX = 14,    /* 1 (default): records are indexed as they arrive -- gd_adopt_device's check pass, a pass over
                                       every committed block once it has landed, the device BAM read's write pass: a position
                                       index (first read at or past every 64th position: the prep kernel looks its tiles' read
                                       ranges up instead of searching) and the largest reference span of any record (the first
                                       gd_compute starts with the right look-back instead of learning it; still verified).
                                       0: neither (the prep kernel searches, the look-back starts at max_span_hint or 512) */
       GD_OPT_INGEST_RANGE_HINT = 18, /* bytes of the LARGEST range gd_ingest_begin will be given (0, the default: unknown): the range
                                       buffers are allocated for it on first use instead of growing -- freeing and allocating --
                                       whenever a later range is larger than the ones before */
       GD_OPT_INGEST_CU_SPLIT = 19,   /* with GD_OPT_INGEST_DMA = 0: every n-th CU (2 .. 64; 0, the default: off) runs only the copy kernel that
                                       pulls staged pieces over the link, the other CUs only the inflate launches (CU-masked
                                       streams); set before the first gd_ingest_begin */
       GD_OPT_INFLATE_KERNEL = 20,    /* which kernel inflates BGZF members: 0 (default) a lane per member (gd_inflate.hpp); 1: a workgroup
                                       per member with the member's output in LDS (gd_inflate_wave.hpp, round 6; members it does not take
                                       go to the other kernel on the same stream).  Both produce zlib's bytes.  The second one moves a
                                       sixth of the bytes through memory and is the slower of the two on an MI355X (DESIGN.md 3.5 has the
                                       measurements and why); it is kept as a second implementation the tests compare the first with.
                                       (ABI 14 had a measurement switch with this number that produced wrong bytes: gone) */
       GD_OPT_INGEST_COPY_GRID = 25,  /* with GD_OPT_INGEST_DMA = 0: workgroups (of 256 threads) of the copy kernel that pulls a staged piece
                                       over the link: 16 (default), 1 .. 4096.  The link needs ~100 KB of reads in flight; a large grid
                                       keeps MEGABYTES of reads to host memory outstanding, and every other kernel on the device then
                                       runs 2.6 times slower (measured: inflate launches 62.7 ms with 512 workgroups, 24.1 ms behind a
                                       copy engine; the genome read 2.11 s with 512, 1.52 - 1.70 s with 8 .. 32, 1.76 s with 4 where
                                       the link starts to starve) */
       GD_OPT_COMMIT_CHECK = 23,      /* where the records of a gd_commit are checked (coordinate order, no negative position, CSR
                                       offsets non-decreasing): 0 (default) on the host, inside gd_commit -- a second pass by CPU
                                       threads over a block the producer has just written; 1: by the pass that indexes the block
                                       on the device once it has landed (it runs anyway), for blocks of 4096 records or more.
                                       gd_commit then returns before the verdict exists: it comes from gd_check_commits, or
                                       from the next gd_compute, which refuses to run on records that failed (the context
                                       needs a gd_reset then).  For producers that are short of CPU -- a decoder's threads --
                                       and do not need the verdict block by block; gdh_produce_in_place runs this way */
       GD_OPT_MOVDEBIAS_SEGMENT = 26, /* gd_moving_debias*: sorted rows a workgroup owns: 0 (default) 256 for a window up to 63, 1024
                                       above; 1 .. 2^30.  A test knob: the results do not depend on it */
       GD_OPT_INDEX_SLICE = 27,       /* gd_index_decode: bytes of the inflated stream per slice in which a record start is guessed:
                                       65536 (default), 64 .. 2^30.  A test knob: the results do not depend on it */
       GD_OPT_INDEX_GUESS_CHECKS = 28, /* ... and how many records the chain behind a candidate must stay a record: 3 (default),
                                       0 .. 64.  With 0 nearly every guess is wrong; the results do not depend on it */
       GD_OPT_INDEX_REPAIR_ROUNDS = 29, /* ... and after how many repair rounds whatever is still unconfirmed is walked as ONE segment behind
                                       the confirmed ones: 4 (default), 0 (at once) .. 2^20 (in effect never).  A test knob as well */

       /* ---- RETIRED ----
        * Switches of link and occupancy experiments that were measured neutral or worse on an MI355X; their code is gone
        * (HISTORY.md has what each one was, and the numbers).  The number stays reserved: gd_set_option accepts the default
        * given here and answers GD_E_INVALID to any other value, gd_get_option returns the default. */
       GD_OPT_INGEST_PIECE_STREAMS = 15, /* 1 */
       GD_OPT_INFLATE_LDS_PAD = 16,   /* 0 */
       GD_OPT_INGEST_HYBRID = 17,     /* 0 */
       GD_OPT_INGEST_BATCHES = 21,    /* 8 */
       GD_OPT_INGEST_WALK_CUS = 22 }; /* 0 */
int gd_set_option(gd_ctx* ctx, int option, int64_t value);
/* The value an option has now (a library that scopes a setting puts it back afterwards). */
int gd_get_option(gd_ctx* ctx, int option, int64_t* value);

/* What is built FROM the records: nothing on the short-read tile path and for the streaming sums (their kernels read the
 * records as they arrived); on the long-read path (GD_PATH_CHUNK, or GD_PATH_AUTO and more than 6 CIGAR ops per record)
 * deletion lists, read records and tile indexes -- by the first gd_compute that needs them, in one pass over the original
 * CIGARs, kept until the records change.  gd_drop_derived forgets them: the state right after the records arrived
 * (measurement: one gd_compute from there is what one `goleft depth` run pays).  gd_rebuild_derived builds the ones the
 * selected contigs currently hold again, into the device block they already occupy -- the work a fresh input costs,
 * without the allocator's.  (ABI 13 also had gd_normalize / gd_canonical_cigars: canonical records, removed.) */
int gd_drop_derived(gd_ctx* ctx);
int gd_rebuild_derived(gd_ctx* ctx);

/* Which results gd_compute materialises in HBM.  GD_OUT_PERBASE (default): the
 * int32 per-base vector (12.4 GB for a human genome), needed by gd_perbase,
 * gd_device_perbase and the --bed region reductions.  Without it only window
 * sums/minima and class runs are produced -- all `goleft depth` prints for a whole
 * genome, and what a cohort (depthwed) needs; tile and chunk paths only. */
enum { GD_OUT_PERBASE = 1,
       /* Window sums ONLY (no per-base vector, no minima, no class runs): all that depth.bed's mean
        * column and the depthwed matrix need.  The short-read path then makes ONE streaming pass over the
        * records as they arrived, every read adding its overlap with the one or two windows it touches -- no tiles,
        * no per-base scan at all (window_size >= 32; smaller windows and the long-read path silently run the
        * regular windows-only kernels).  gd_callable and minima report GD_E_STATE.  Excludes
        * GD_OUT_PERBASE. */
       GD_OUT_SUMS_ONLY = 2 };
int gd_set_outputs(gd_ctx* ctx, unsigned flags);

/* Reference sequence table (@SQ LN of the BAM header / .fai lengths,
 * depth/depth.go:134-149).  Drops all records and results.  Lengths are 0 .. GD_MAX_CONTIG_LENGTH (BAM itself
 * stops at 2^31 - 1; the last 64 Ki positions are given up so that tile arithmetic stays in 32 bits), else
 * GD_E_RANGE. */
#define GD_MAX_CONTIG_LENGTH 0x7fff0000LL
int gd_set_contigs(gd_ctx* ctx, int n_contigs, const int64_t* lengths);

/* Restrict computation to a subset of contigs (--chrom, depth/depth.go:145).
 * n == 0 selects all. */
int gd_select_contigs(gd_ctx* ctx, int n, const int32_t* tids);

/* ---- record ingest: pinned ring buffers -> HBM (replaces the BGZF/BAM read
 * that each `samtools depth` child performs) --------------------------------*/

/* Borrow a pinned staging block with at least the given capacities.  Waits
 * for the block's previous copy if that is still in flight.  A producer may
 * hold up to three blocks at a time (its threads write block k+1 while
 * gd_commit validates and sends block k -- gdh_produce_in_place does); blocks
 * go back to the ring in the order they were handed out, and GD_E_STATE
 * answers a gd_acquire that comes round to a block still held.  gd_commit
 * with n_reads 0 gives a block back unused; gd_reset gives all of them back. */
int gd_acquire(gd_ctx* ctx, size_t reads_cap, size_t ops_cap, gd_batch* out);

/* Append n_reads records (n_ops ops) of contig tid from a block obtained from
 * gd_acquire; the H2D copy is asynchronous on the copy stream and the block
 * returns to the ring when it completes.  Records of one contig must be
 * committed in coordinate order (GD_E_UNSORTED); a negative position is
 * GD_E_RANGE (a placed BAM record has POS >= 0).  The order of the commits is
 * the order of the records; whether it succeeds or not, the block is no longer
 * the caller's afterwards (a second commit of it is GD_E_STATE). */
int gd_commit(gd_ctx* ctx, const gd_batch* b, int32_t tid, size_t n_reads, size_t n_ops);

/* With GD_OPT_COMMIT_CHECK = 1: waits for the committed blocks to land and returns what their checks found --
 * GD_OK, GD_E_UNSORTED, GD_E_RANGE (a negative position) or GD_E_INVALID (CSR offsets) -- for everything
 * committed since the last call (or the last gd_compute / gd_reset).  Nothing to report and nothing waited
 * for when no block has been checked on the device. */
int gd_check_commits(gd_ctx* ctx);

/* Optional: room for n_reads more records / n_ops more CIGAR ops of contig tid in one step.  A producer that knows
 * its totals (the .bai metadata pseudo-bin holds a reference's mapped-record count) spares the device arrays their
 * growth by doubling, each step of which waits for the copies in flight. */
int gd_reserve(gd_ctx* ctx, int32_t tid, size_t n_reads, size_t n_ops);

/* Convenience: copy records from ordinary host memory (copies before
 * returning; never keeps the pointers). */
int gd_push(gd_ctx* ctx, int32_t tid, const int32_t* pos, const uint16_t* flag,
            const uint8_t* mapq, const uint32_t* cigar_off, const uint32_t* cigar,
            size_t n_reads, size_t n_ops);

/* Use records already resident in HBM (zero copy).  Replaces any records of
 * that contig.  The call waits for the device (whatever stream produced the
 * arrays) and checks them the way gd_commit checks a host block -- positions in
 * coordinate order (GD_E_UNSORTED) and not negative (GD_E_RANGE), CSR offsets non-decreasing from 0 and ending
 * inside the op array (GD_E_INVALID); one pass over pos / cigar_off.  Arrays aligned to 16 (pos, cigar_off),
 * 8 (flag) and 4 (mapq) bytes -- anything hipMalloc or a tensor allocator returns -- get the straight-line
 * tile kernel; others the generic one. */
int gd_adopt_device(gd_ctx* ctx, int32_t tid, const gd_batch* dev, size_t n_reads, size_t n_ops);

/* Drop records and results, keep contigs/params/allocations. */
int gd_reset(gd_ctx* ctx);

/* ---- compute -------------------------------------------------------------*/

/* Per-base depth for every selected contig, fused with the per-window
 * sum/min reduction and the coverage-class run-length encoding (what
 * `samtools depth` + callback compute per tile).  Synchronous: returns when
 * results are ready. */
int gd_compute(gd_ctx* ctx);
/* The same in two halves: gd_compute_launch enqueues every kernel and the read-back copies on the context's
 * stream and returns without waiting; gd_compute_finish waits, verifies (re-running synchronously when the
 * look-back / capacity checks ask for it) and publishes the results.  Between the two the host is free -- e.g.
 * to issue the collective of the PREVIOUS step while this one's kernels run (bench.py --gpus N).  Exactly one
 * compute may be in flight per context; until gd_compute_finish, result calls and calls that change the job
 * (records, contigs, parameters, path, outputs, options, gd_ingest_*, gd_md_*) are refused with GD_E_STATE --
 * gd_compute_launch starts overwriting the result arrays.  gd_set_export may be called in between (it takes
 * effect with the next launch). */
int gd_compute_launch(gd_ctx* ctx);
int gd_compute_finish(gd_ctx* ctx);

/* ---- results -------------------------------------------------------------*/

/* depth[start..end) of contig tid into host memory. */
int gd_perbase(gd_ctx* ctx, int32_t tid, int64_t start, int64_t end, int32_t* out);

/* Window sums (and optionally minima; mins may be NULL) for W-anchored
 * windows of contig tid: window k covers [k*W, min((k+1)*W, len)).
 * *n receives the window count; GD_E_CAPACITY if cap is too small. */
int gd_windows(gd_ctx* ctx, int32_t tid, int64_t* sums, int32_t* mins, size_t cap, size_t* n);

/* Coverage-class runs of contig tid in coordinate order, split at multiples
 * of params.step (reference quirk Q1) and nowhere else. */
int gd_callable(gd_ctx* ctx, int32_t tid, gd_run* out, size_t cap, size_t* n);

/* --bed mode (depth/depth.go:103-120): reductions over an arbitrary region of
 * the already computed per-base vector.  Windows stay anchored at absolute
 * multiples of W and are clipped to [start,end) (depth/depth.go:297-298);
 * positions past the contig end have depth 0. */
int gd_region_windows(gd_ctx* ctx, int32_t tid, int64_t start, int64_t end,
                      int64_t* sums, int32_t* mins, size_t cap, size_t* n);
int gd_region_callable(gd_ctx* ctx, int32_t tid, int64_t start, int64_t end,
                       gd_run* out, size_t cap, size_t* n);
/* The same two reductions for MANY regions in one call (a --bed file: one launch per reduction for
 * the whole batch instead of several launches, allocations and synchronisations per row).  Region r
 * is [start[r], end[r]) on contig tid[r].  Its W-anchored windows are sums/mins[win_off[r] ..
 * win_off[r+1]) and its class runs runs[run_off[r] .. run_off[r+1]); win_off and run_off have
 * n_regions + 1 entries and are written by the call.  mins may be NULL.  GD_E_CAPACITY when
 * cap_windows or cap_runs is too small: win_off[n_regions] / run_off[n_regions] then hold what is
 * needed (a windows shortfall is reported first, with run_off zeroed). */
int gd_regions(gd_ctx* ctx, size_t n_regions, const int32_t* tid, const int64_t* start, const int64_t* end,
               int64_t* sums, int32_t* mins, size_t cap_windows, size_t* win_off,
               gd_run* runs, size_t cap_runs, size_t* run_off);

/* ---- depthwed on device (depthwed/depthwed.go; BASELINE.json config 4) -----
 * A cohort is loaded as n_samples x n_ctg contigs of ONE context (tids[s*n_ctg+j]
 * = engine contig holding sample s, reference contig j; the n_samples contigs of
 * one j must have equal length).  After gd_compute, builds the sites x samples
 * matrix `goleft depthwed -s size` would print from the samples' depth.bed files:
 * rows = groups of ceil(size/W) consecutive windows per contig (the last group of
 * a contig may be shorter), cell = sum over the group's windows of
 * int(0.5 + "%.4g"(window_sum/window_len)) -- the text round trip is reproduced
 * exactly in arithmetic, no text is formatted.  cells is row major
 * [n_rows][n_samples]; row_ctg/row_start/row_end (each may be NULL) describe the
 * rows.  *n_rows receives the row count; GD_E_CAPACITY if cap_rows is too small. */
int gd_depthwed(gd_ctx* ctx, int n_samples, int n_ctg, const int32_t* tids, int64_t size,
                int64_t* cells, int32_t* row_ctg, int64_t* row_start, int64_t* row_end,
                size_t cap_rows, size_t* n_rows);
/* Same matrix, left in HBM for the next consumer (the normalisation / CNV steps that read
 * depthwed output, e.g. dcnv/dcnv.go:153-186): *d_cells is a device pointer to
 * [n_rows][n_samples] int64, valid until the next gd_depthwed* / gd_destroy. */
int gd_depthwed_device(gd_ctx* ctx, int n_samples, int n_ctg, const int32_t* tids, int64_t size,
                       const int64_t** d_cells, size_t* n_rows);

/* ---- `--stats` columns on device (depth/depth.go:191-200, :244-252) ----------
 * The reference appends "%.3g" of GC, CpG and masked fraction of each window's
 * reference bases (faidx.Stats, an external module: PARITY UNPINNED, semantics
 * restated in oracle/pyoracle.py::seq_stats).  gd_seq_load copies ONE contig's
 * bases (FASTA line breaks removed) into HBM, replacing the previous one; the
 * pointer is not retained.  gd_seq_stats then returns, for each window
 * [start[k], end[k]) clipped to the contig: n_gc = bases in "GCgc", n_masked =
 * lower-case bases, n_cpg = C/c followed by G/g (the following base may lie past
 * the window, not past the contig).  Integer counts only: the divisions by
 * (end - start) and the "%.3g" stay on the host.  Does not need gd_compute. */
int gd_seq_load(gd_ctx* ctx, const uint8_t* seq, int64_t len);
int gd_seq_stats(gd_ctx* ctx, size_t n_windows, const int64_t* start, const int64_t* end,
                 uint32_t* n_gc, uint32_t* n_cpg, uint32_t* n_masked);
/* The same plus what the other plausible reading of faidx.Stats needs (goleft_depth_host.h GDH_STATS_*; the
 * caller picks the contract, the library only counts): n_acgt = bases in "ACGTacgt" (a denominator that
 * skips N and IUPAC codes), n_masked_acgt = bases in "acgt"; either may be NULL.  line_bases > 0 (bases per
 * FASTA line, the .fai LINEBASES column): a C that is the last base of a line -- or of the window -- does not
 * start a CpG: what a scan of the window's raw, line-broken bytes sees; 0: the sequence is one line and the
 * base after the window counts. */
int gd_seq_stats_ex(gd_ctx* ctx, size_t n_windows, const int64_t* start, const int64_t* end, int32_t line_bases,
                    uint32_t* n_gc, uint32_t* n_cpg, uint32_t* n_masked, uint32_t* n_acgt, uint32_t* n_masked_acgt);

/* ---- multidepth on device (multidepth/multidepth.go) ----------------------------
 * The S samples are S equally long contigs tids[0..S) of ONE context, computed by
 * gd_compute with -Q = multidepth's Q (per-base output kept).  gd_md_flags replaces
 * the multi-file `samtools depth` text stream and its parse (:203-207, :148-161)
 * plus sufficientDepth (:163-171) with two bitmaps over the contig (bit x of word
 * x/32, little endian): any = some sample has depth > 0 (the positions samtools
 * prints), suf = MORE THAN min_samples samples have depth >= min_cov.  The block
 * state machine (:217-258) then runs on the host over the bitmaps.  gd_md_sums
 * returns, for each block [start, end) and sample, the reference's running sum
 * `dps[i] += float64(d) / 1000.` over the block's suf sites in position order
 * (means, :270-277) as the exact IEEE double; sums is row major [n_blocks][S] and
 * uses the samples and bitmaps of the last gd_md_flags.  GD_E_CAPACITY if n_words
 * < ceil(len/32). */
int gd_md_flags(gd_ctx* ctx, int n_samples, const int32_t* tids, int32_t min_cov, int32_t min_samples,
                uint32_t* any_bits, uint32_t* suf_bits, size_t n_words);
int gd_md_sums(gd_ctx* ctx, size_t n_blocks, const int64_t* start, const int64_t* end, double* sums);
/* The same bitmaps with the samples brought in GROUPS, so that only one group's per-base vectors have to be
 * resident (gd_select_contigs + gd_compute per group; the reference bounds memory with 5 Mb position chunks,
 * :114,126): gd_md_begin(len) zeroes the per-position accumulators, gd_md_accumulate adds a group (the tids of
 * the last gd_compute), gd_md_finish turns them into `any` / `suf` (copied out when the pointers are non-NULL)
 * and makes them the bitmaps gd_md_blocks and gd_md_sums_group use.  At most 65535 samples. */
int gd_md_begin(gd_ctx* ctx, int64_t len);
int gd_md_accumulate(gd_ctx* ctx, int n_samples, const int32_t* tids, int32_t min_cov);
int gd_md_finish(gd_ctx* ctx, int32_t min_samples, uint32_t* any_bits, uint32_t* suf_bits, size_t n_words);
/* Bitmaps made elsewhere become the current ones (tests; a host with its own depth source).  Precondition: suf is a
 * subset of any -- the reference only ever sees printed sites, so what gd_md_blocks answers for a sufficient but
 * unprinted site is not defined by it (gd_md_flags and gd_md_finish may produce such sites, with min_cov <= 0 or
 * min_samples < 0; the blocks over them are the device's own). */
int gd_md_load_flags(gd_ctx* ctx, const uint32_t* any_bits, const uint32_t* suf_bits, int64_t len);
/* The block state machine on the device (aggregate + splitBlocks, multidepth.go:188-268, for every chunk of
 * `chunk` positions, in chunk order -- what `multidepth -p 1` prints): blocks [start, end) over the current
 * bitmaps.  *n_blocks receives their number; GD_E_CAPACITY (with *n_blocks set) when cap is too small.  The
 * quirks of the reference are kept: nothing is reported before a chunk's first insufficient site, the last
 * cache of a chunk skips the min_size test, neighbouring chunks may report overlapping blocks. */
int gd_md_blocks(gd_ctx* ctx, int64_t chunk, int32_t max_skip, int32_t min_size, int32_t window,
                 int64_t* starts, int64_t* ends, size_t cap, size_t* n_blocks);
/* gd_md_sums for the samples tids[0..n_samples) of the last gd_compute (one group): sums is [n_blocks][n_samples]. */
int gd_md_sums_group(gd_ctx* ctx, int n_samples, const int32_t* tids, size_t n_blocks, const int64_t* start,
                     const int64_t* end, double* sums);

/* ---- BGZF inflate on device (the first stage of the BAM read of depth/depth.go:45) ----
 * A BGZF file is a sequence of independent <= 64 KiB DEFLATE streams ("members").  The
 * caller lists them (payload offset/length inside data, ISIZE, and where each member's
 * bytes go in out); one GPU lane inflates one member and checks it against crc[m], the
 * CRC32 of the gzip trailer (crc may be NULL: not checked).  status[m] is 0 or a decoder
 * error code (corrupt stream, ISIZE mismatch, 18 = CRC32 mismatch).  data, out and status
 * are host buffers. */
int gd_inflate_bgzf(gd_ctx* ctx, const uint8_t* data, size_t n_bytes, size_t n_members,
                    const uint64_t* in_off, const uint32_t* in_len, const uint64_t* out_off,
                    const uint32_t* out_len, const uint32_t* crc, uint8_t* out, size_t out_bytes,
                    uint32_t* status);

/* ---- the whole BAM read of one contig on the device -------------------------------------
 * data: a byte range of the BAM file that begins at a BGZF member boundary (its file offset
 * is base_coffset) and holds every record of the BAM reference ref_id, which become the records
 * of engine contig tid (the same number for `goleft depth`; multidepth maps one reference of S
 * files onto S contigs).  anchors: virtual file offsets
 * (coffset << 16 | uoffset, as stored in the .bai) of record starts inside the range,
 * strictly ascending, anchors[0] = the contig's first record -- the .bai linear index
 * provides one per 16 kb of reference (SAMv1 5.2).  The device inflates the members (one
 * lane each), one wave per anchor walks the records up to the next anchor (a record of
 * another reference ends the walk; it counts them and notes where each starts), a thread
 * per record then extracts, and {pos, flag, mapq, CIGAR (CG:B,I resolved)} become
 * the contig's record arrays in HBM, replacing what it held -- the state gd_push / gd_commit
 * would have left, without any decode on the host.  Every member's CRC32 is verified.
 * Errors: GD_E_INVALID (corrupt member or record, CRC mismatch, anchor that is not a record
 * start), GD_E_UNSORTED. */
int gd_ingest_bgzf(gd_ctx* ctx, int32_t tid, int32_t ref_id, const uint8_t* data, size_t n_bytes,
                   uint64_t base_coffset, const uint64_t* anchors, size_t n_anchors, uint64_t* n_records);
/* The same read as a stream, so that file I/O overlaps the device work: list the range's
 * members first (gd_bgzf_members, headers and trailers only), announce them
 * (gd_ingest_begin: allocations), then feed the range's bytes in order in pieces of any
 * size -- each piece is copied into page-locked staging (the pointer is not retained),
 * uploaded asynchronously, and every member that is complete on the device is inflated
 * behind the copy while the caller reads the next piece -- and finish with the anchors.
 * gd_ingest_bgzf is begin + one feed + finish.  gd_ingest_abort drops an unfinished read.
 * A fed range may hold several references (a BAM with thousands of small contigs: one inflate
 * pass has a latency floor of ~0.04 s whatever its size): gd_ingest_decode is gd_ingest_finish
 * without the release, so call it once per reference of the range (each with that reference's
 * anchors and its own contig), then gd_ingest_release -- or gd_ingest_finish for the last one.
 * Three ranges may be pending at a time: once a range is completely fed, gd_ingest_begin / _feed of
 * the NEXT range may run before the first is decoded, so that the last inflate launches of one
 * range (latency bound) overlap the upload of the next -- and with a third, the decode of the oldest
 * never holds the upload up; gd_ingest_decode, _finish and _release
 * always act on the oldest pending range, gd_ingest_feed on the newest.  A fourth gd_ingest_begin is
 * refused (GD_E_STATE, nothing changes); gd_ingest_begin while the newest range is only partly fed
 * abandons what is pending, like gd_ingest_abort (which drops everything).  An error while feeding or
 * decoding drops everything pending. */
int gd_bgzf_members(const uint8_t* data, size_t n_bytes, size_t cap, uint64_t* member_off, uint32_t* member_size,
                    uint16_t* header_size, uint32_t* isize, uint32_t* crc, size_t* n_members);
int gd_ingest_begin(gd_ctx* ctx, uint64_t n_bytes, uint64_t base_coffset, size_t n_members,
                    const uint64_t* member_off, const uint32_t* member_size, const uint16_t* header_size,
                    const uint32_t* isize, const uint32_t* crc);
int gd_ingest_feed(gd_ctx* ctx, const uint8_t* bytes, size_t n);
/* gd_ingest_feed with the bytes taken from an open file: n bytes from `offset` of `fd` are read (pread on the
 * context's worker threads, GD_OPT_PUSH_THREADS of them) straight into the page-locked staging buffers -- none
 * of the page faults of a mapping, no second copy.  The read runs on a thread of the context and the call returns
 * at once (fd must stay open): gd_ingest_decode / _release of the OLDEST pending range and gd_ingest_begin of
 * the next one proceed meanwhile; every other gd_ingest_* call waits for the read first and reports its error
 * (GD_E_INVALID: the file ended early or could not be read). */
int gd_ingest_feed_fd(gd_ctx* ctx, int fd, uint64_t offset, size_t n);
int gd_ingest_finish(gd_ctx* ctx, int32_t tid, int32_t ref_id, const uint64_t* anchors, size_t n_anchors,
                     uint64_t* n_records);
int gd_ingest_decode(gd_ctx* ctx, int32_t tid, int32_t ref_id, const uint64_t* anchors, size_t n_anchors,
                     uint64_t* n_records);
int gd_ingest_release(gd_ctx* ctx);
/* A reference read in SEVERAL ranges (passes cut inside a chromosome at .bai anchors: buffers of one pass instead of
 * one chromosome, and only the last pass's inflate and record walks left without an upload to hide behind): the
 * oldest pending range holds the reference's records from anchors[0] up to `end_anchor` -- the virtual offset of the
 * first record that belongs to the NEXT part (a record start the index knows, inside a member of this range; 0: the
 * part runs to the range's end, as gd_ingest_decode).  flags: GD_PART_APPEND -- the records are appended to what the
 * contig holds (parts must arrive in file order; coordinate order is checked across parts, and a reference that ended
 * in an earlier part must not resume), else they replace it; GD_PART_RELEASE -- the range is released afterwards.
 * expect_scale (>= 1; 0: unknown): how many times this part's share the whole reference is expected to be (its byte
 * range over this part's), so that the FIRST part allocates the contig's arrays once for all parts (they grow
 * geometrically when the estimate was short). */
enum { GD_PART_APPEND = 1, GD_PART_RELEASE = 2 };
int gd_ingest_decode_part(gd_ctx* ctx, int32_t tid, int32_t ref_id, const uint64_t* anchors, size_t n_anchors,
                          uint64_t end_anchor, unsigned flags, double expect_scale, uint64_t* n_records);
/* Where the device BAM read of this context has spent its wall clock so far, in seconds (measurement only):
 * out[0] reading into the staging buffers, [1] waiting for a staging buffer to leave for the device, [2] gd_ingest_begin
 * (allocations, member table), [3] decode: waiting for the inflate launches, [4] decode: the counting walk, [5] decode:
 * allocating the contig's arrays, [6] decode: the extraction (a thread per record over the walk's table).  Fills min(n, 7) values. */
int gd_ingest_timing(gd_ctx* ctx, double* out, size_t n);
/* ---- `goleft covstats` (covstats/covstats.go:122-220) on the fed ranges of the device BAM read ----
 * gd_covstats_begin starts a sampling run: n inserts to sample, the first `skip` records of the stream
 * skipped.  Then, range after range (gd_ingest_begin + gd_ingest_feed*), gd_covstats_decode walks EVERY
 * record of the oldest pending range in file order from first_voffset (the first record of the run, or the
 * previous call's `resume`), across references and through the unplaced tail, and drops the range.
 * anchors: ascending virtual offsets of record starts (the .bai linear indexes of all references, merged);
 * those inside the range cut the walk into segments, the rest are ignored.  last_range: the range ends the
 * file (a record it holds only in part is an error); otherwise such a record is where the next range resumes.
 * *out: the counts so far; done != 0 once the sampling loop has stopped (no further range is needed). */
typedef struct gd_covstats_counts {
    int64_t records;          /* records walked since gd_covstats_begin */
    int64_t range_records;    /* ... in the last range */
    int64_t skip_left;        /* records still to be skipped */
    int64_t unmapped, counted, bad, dup, proper;   /* nU, k, nBad, nDup, nProper of the sampling loop */
    int64_t sizes, inserts;   /* query lengths and insert sizes sampled */
    uint64_t resume;          /* virtual offset of the first record the range did not hold completely.  A record that
                               * starts on a member boundary is spelled (the member that begins there -- of several,
                               * the last: the one with bytes --, uoffset 0), never (the member before, its ISIZE); when
                               * every record of the range is whole: (the member that follows the range, 0), which for
                               * the file's last range is the file's size.  gd_covstats_decode takes either spelling
                               * as first_voffset. */
    int32_t done;
    int32_t reserved;
} gd_covstats_counts;
int gd_covstats_begin(gd_ctx* ctx, int64_t n, int64_t skip);
int gd_covstats_decode(gd_ctx* ctx, uint64_t first_voffset, const uint64_t* anchors, size_t n_anchors, int last_range,
                       gd_covstats_counts* out);
/* The sampled values of one kind (which: 0 query lengths, 1 insert sizes, 2 template lengths): *n_bins counts
 * of the values lo .. lo + n_bins - 1 (bins: NULL or room for *n_bins), and the values outside that window,
 * unordered (overflow: NULL or room for cap; *n_overflow: how many there are). */
int gd_covstats_histogram(gd_ctx* ctx, int which, int64_t* lo, size_t* n_bins, uint64_t* bins, int64_t* overflow,
                          size_t cap, size_t* n_overflow);
/* ---- a BAM's .bai (SAMv1 5.2) from the fed ranges of the device BAM read: no index needed, one is made ----
 * gd_index_begin starts a run over ONE file: its references (n_ref lengths from the header), the virtual offset of its
 * first record and its size.  Then, range after range in file order (gd_ingest_begin + gd_ingest_feed*; a range begins
 * with the member that holds the previous call's `resume`), gd_index_decode walks every record of the oldest pending
 * range and drops the range.  Record starts are GUESSED per slice of the inflated bytes (GD_OPT_INDEX_SLICE,
 * GD_OPT_INDEX_GUESS_CHECKS) and CONFIRMED by the walk: a wrong guess costs a repair round, never the answer (`rounds`).
 * last_range: the range ends the file (a record it holds only in part is an error); otherwise that record is where
 * the next range resumes.  gd_index_result gives what a .bai is assembled from (gdh_bai_assemble of the host library):
 * the runs -- maximal stretches of consecutive records of one (reference, bin), begin and end as virtual offsets, in file
 * order, as if the file had been one range --, the linear index before its backward fill (entry lin_off[r] + w of
 * reference r's 16 kb window w; all ones: no record touches the window; gd_index_windows gives lin_off[0 .. n_ref]: a
 * reference has its length in windows and a few more, and the array grows when a read hangs further over the end than
 * that, so ask after the last decode) and per reference the pseudo-bin's four words.  Every output may be NULL; a
 * capacity below what is there is GD_E_CAPACITY with the counts set.
 * Errors (gd_last_error names the record): GD_E_UNSORTED -- positions go backwards inside a reference, a reference
 * resumes after another began, a placed record follows an unplaced one; GD_E_INVALID -- a damaged member or record, a
 * placed record with a negative position or an end beyond 2^29.  gd_index_result before the file's last range has been
 * decoded is GD_E_STATE. */
typedef struct gd_index_counts {
    int64_t records;          /* records walked since gd_index_begin */
    int64_t range_records;    /* ... in the last range */
    int64_t runs;             /* runs so far (the last one may still grow) */
    int64_t n_no_coor;        /* records with refID < 0 so far */
    uint64_t resume;          /* as gd_covstats_counts.resume */
    int32_t slices;           /* of the last range: slices, */
    int32_t guesses;          /* ... those with a guess, */
    int32_t rounds;           /* ... and repair rounds: walks after the first (0: every guess was a record start) */
    int32_t reserved;
} gd_index_counts;
typedef struct gd_index_run { int32_t ref; uint32_t bin; uint64_t beg, end; } gd_index_run;
typedef struct gd_index_ref { uint64_t first_beg, last_end, n_mapped, n_unmapped; } gd_index_ref;   /* no records: all 0 */
int gd_index_begin(gd_ctx* ctx, int32_t n_ref, const int64_t* ref_len, uint64_t first_voffset, uint64_t file_size);
/* The same run for a .csi (CSI version 1): bins whose smallest span 2^min_shift positions (8 to
 * 24), `depth` levels below bin 0 (0 to 8), so positions up to min(2^(min_shift + 3 depth), 2^31 - 1); the linear array has
 * a window per 2^min_shift positions (gdh_csi_assemble takes the bins' loffset from it: a .csi stores no linear index).
 * gd_index_begin is this with 14 and 5 -- a .bai's scheme -- and a .bai's wording when a record lies beyond 2^29.
 * gd_index_decode, _result and _windows serve both.  GD_E_INVALID: min_shift or depth outside those ranges. */
int gd_index_begin_csi(gd_ctx* ctx, int32_t n_ref, const int64_t* ref_len, uint64_t first_voffset, uint64_t file_size,
                       int32_t min_shift, int32_t depth);
int gd_index_decode(gd_ctx* ctx, int last_range, gd_index_counts* out);
int gd_index_windows(gd_ctx* ctx, uint64_t* lin_off, size_t cap);   /* cap >= n_ref + 1 */
int gd_index_result(gd_ctx* ctx, gd_index_run* runs, size_t cap_runs, size_t* n_runs, uint64_t* linear, size_t cap_linear,
                    size_t* n_linear, gd_index_ref* refs, uint64_t* n_no_coor);
/* Seconds since gd_index_begin (measurement only): out[0] waiting for the inflate launches, [1] guessing, [2] the walks,
 * all rounds, [3] compaction, runs and linear kernels, [4] read-back.  Fills min(n, 5) values. */
int gd_index_timing(gd_ctx* ctx, double* out, size_t n);
/* ---- `goleft indexcov` (indexcov/indexcov.go, types.go) on the tile sizes of a cohort of .bai linear indexes ----
 * gd_indexcov_upload takes, for n_samples samples, EVERY tile size of every reference of each index (sizes, the
 * samples one after the other: sample s owns [sample_off[s], sample_off[s + 1]), never empty, never negative) --
 * the median is taken over all of them -- and, for the n_refs references that are reported, where the tiles of
 * (sample s, reference r) lie: tile_off[s * n_refs + r] (into sizes) and tile_cnt[...]; is_sex[r] marks the sex
 * references.  It computes the medians (Index.init) and the float32 depths (NormalizedDepth) at once; a sample
 * whose median is 0 has no tiles on any reference from then on.  gd_indexcov_set_depths replaces the depths (the
 * reference's -n pass runs on the host, in its order).  gd_indexcov_compute makes, per reference r with
 * longest[r] = the most tiles any sample has: the %.3g cells (cell_off[r] + tile * n_samples + sample; a packed
 * cell is digits | (exponent + 128) << 16, see gd_round3g.hpp), the 70 CountsAtDepth slots
 * ([r][sample][70]), per sample the counters {out, low, hi, in} over the non-sex references, GetCN of every sex
 * reference ([r][sample]; 0 elsewhere), the pca8 bytes ([sample][m], column col_off[r] + tile) and, with_gram != 0,
 * the exact Gram matrix G = pca8 * pca8^T ([sample][sample], int64). */
typedef struct gd_indexcov_dims {
    int64_t n_tiles, n_cells, m, m_pad;
    int32_t n_samples, n_refs;
} gd_indexcov_dims;
int gd_indexcov_upload(gd_ctx* ctx, int32_t n_samples, int32_t n_refs, const int64_t* sample_off, const int64_t* sizes,
                       const int64_t* tile_off, const int32_t* tile_cnt, const uint8_t* is_sex);
int gd_indexcov_get_dims(gd_ctx* ctx, gd_indexcov_dims* out, int32_t* longest, int64_t* cell_off, int64_t* col_off);
int gd_indexcov_medians(gd_ctx* ctx, int64_t* out);
int gd_indexcov_depths(gd_ctx* ctx, float* out, size_t cap);
int gd_indexcov_set_depths(gd_ctx* ctx, const float* in, size_t n);
int gd_indexcov_compute(gd_ctx* ctx, int with_gram);
int gd_indexcov_cells(gd_ctx* ctx, int64_t first, int64_t n, uint32_t* out);
int gd_indexcov_slots(gd_ctx* ctx, int32_t* out);
int gd_indexcov_counters(gd_ctx* ctx, int64_t* out);
int gd_indexcov_cn(gd_ctx* ctx, double* out);
int gd_indexcov_pca8(gd_ctx* ctx, uint8_t* out);
int gd_indexcov_gram(gd_ctx* ctx, int64_t* out);
/* Seconds of the last upload / compute (measurement only): upload, medians + depths, cells / slots / counters / pca8,
 * CN, Gram matrix.  Fills min(n, 5) values. */
int gd_indexcov_timing(gd_ctx* ctx, double* out, size_t n);
/* ---- `goleft indexsplit` (indexsplit/indexsplit.go:89-114): the sum of a cohort's tile sizes, cell by cell ----
 * gd_indexsplit_begin allocates one float64 per cell -- longest[r] cells for each of the n_refs references, one
 * reference after the other -- and zeroes them; a state of an earlier begin is dropped first.  gd_indexsplit_add
 * takes a batch of samples in the layout of gd_indexcov_upload (sample_off, sizes, tile_off, tile_cnt; n_refs is
 * begin's) and adds float64(size) / 1e9 of every tile to its cell, the samples in the order of the calls and then of
 * the batch: every cell sees the additions the reference makes, in its order, so the sums do not depend on how the
 * cohort was cut into batches.  A sample may be empty.  A batch is checked before any of it is added: offsets outside
 * the sample or tile_cnt above longest[r] are GD_E_RANGE, a negative size or a bad sample_off GD_E_INVALID, and the
 * sums stay as they were.  gd_indexsplit_sums copies the cells out (GD_E_CAPACITY when cap is below their number).
 * The state goes with the context or with the next gd_indexsplit_begin. */
int gd_indexsplit_begin(gd_ctx* ctx, int32_t n_refs, const int32_t* longest);
int gd_indexsplit_add(gd_ctx* ctx, int32_t n_samples, const int64_t* sample_off, const int64_t* sizes,
                      const int64_t* tile_off, const int32_t* tile_cnt);
int gd_indexsplit_sums(gd_ctx* ctx, double* out, size_t cap);
/* Seconds since gd_indexsplit_begin (measurement only): upload, kernel, read-back.  Fills min(n, 3) values. */
int gd_indexsplit_timing(gd_ctx* ctx, double* out, size_t n);
/* ---- the tile sizes of .crai slices (indexcov/crai/crai.go:56-127 makeSizes): what a .crai gives `indexcov` and
 * `indexsplit` in place of a .bai's linear index ----
 * A sequence is one reference of one index: the slices [seq_off[s], seq_off[s + 1]) of the three arrays, in file order
 * (alnStart, alnSpan and sliceLen of the index's lines).  One wavefront walks a sequence; the call takes as many
 * sequences as the caller has -- a whole cohort -- and the result of a sequence does not depend on what else is in the
 * call.  tile_off[s + 1] - tile_off[s] is the number of 16 384-base tiles of sequence s (tile_off[0] = 0) and status[s]
 * is 0, or 1 / 2 where the reference panics ("tilewidth logic error" / "logic error"; no input is known to get there;
 * the tiles of such a sequence are the ones emitted up to that point).  Both are always filled.  sizes == NULL: that
 * is all (count only).  Otherwise the tiles of sequence s are written to sizes[tile_off[s] .. tile_off[s + 1]), or,
 * when cap < tile_off[n_seq], nothing is and the call returns GD_E_CAPACITY with tile_off in place.  GD_E_INVALID: a
 * seq_off that does not start at 0 or decreases; GD_E_RANGE: an alnStart outside +-(2^31 - 1) or an alnSpan outside
 * 0 .. 2^31 - 1 -- both found before anything is launched.  n_seq == 0 is GD_OK.  Nothing is kept between calls. */
int gd_crai_sizes(gd_ctx* ctx, int32_t n_seq, const int64_t* seq_off,    /* [n_seq + 1] into the three arrays */
                  const int64_t* aln_start, const int64_t* aln_span, const int32_t* slice_len,
                  int64_t* tile_off,                                      /* out [n_seq + 1] */
                  int32_t* status,                                        /* out [n_seq]: 0, or which panic */
                  int64_t* sizes, size_t cap);                            /* NULL: count only */
/* ---- emdepth.EMDepth (emdepth/emdepth.go:117-206, :250-304) per row of a sites x samples depth matrix ----
 * For every row: the copy-number centres lambda[0..8] fitted by the reference's EM (median start, at most ten
 * classify-and-average passes), the number of passes run (1 .. 10), every cell's copy number (Type with adjustCN:
 * 0 .. 8, and 9 for a depth above lambda[8], as the reference's code -- not its unit test -- has it) and every cell's
 * log2(depth / lambda[2]) as float32 (-inf for a depth of 0).  Quirk for quirk: the median of an even row is
 * (b[N/2] + b[N/2 + 1]) / 2, and the centres are searched with the reference's binary search although they are not always
 * ascending.  n_samples is 1 or 3 .. 4096 (the reference panics on 0 and 2), GD_E_RANGE otherwise.  Any output may be
 * NULL.  n_rows == 0 is GD_OK.  Nothing is kept between calls; everything is checked before anything runs.
 *   gd_emdepth        depths: host float32 [n_rows][n_samples], each finite and >= 0 (GD_E_INVALID otherwise)
 *   gd_emdepth_cells  d_cells: DEVICE int64 [n_rows][n_samples] as gd_depthwed_device leaves them (non-negative); the
 *                     depth of a cell is (float)cell, and with scale (host [n_samples], finite and >= 0, or NULL)
 *                     (float)cell * scale[s] in float32: one rounding each.  The matrix does not leave HBM.
 * Rows whose depths are integers (times one power of two) give lambda bit for bit as the reference's float64 loop does;
 * otherwise the bin sums are taken in another order and lambda agrees to about n_samples * 2^-53 relative.
 * gd_emdepth_timing: seconds of the last call (measurement only): upload, kernel, read-back.  Fills min(n, 3) values. */
int gd_emdepth(gd_ctx* ctx, const float* depths, size_t n_rows, int n_samples,
               double* lambda /* [n_rows][9] */, uint8_t* iters /* [n_rows] */, uint8_t* cn /* [n_rows][n_samples] */,
               float* log2fc /* [n_rows][n_samples] */);
int gd_emdepth_cells(gd_ctx* ctx, const int64_t* d_cells, size_t n_rows, int n_samples, const float* scale,
                     double* lambda, uint8_t* iters, uint8_t* cn, float* log2fc);
int gd_emdepth_timing(gd_ctx* ctx, double* out, size_t n);
/* ---- emdepth.Cache (emdepth/emdepth.go:216-398): a sample's aberrant sites joined into CNV calls, on the device ----
 * The rows go in in input order, in blocks of any size (the result does not depend on the cut); every block runs the
 * emdepth kernel and keeps its outputs in HBM.  A cell is U when log2(depth / lambda[2]) (float64) >= 0.40, D when it is
 * <= -0.80; a cell is a member when it is U or D and the same sample's cell one row up has the same state (row 0 is
 * compared with itself).  A row r is a gap for a member of row a when (start[r] - end[a]) mod 2^32 >= 30000 -- a start
 * below that end wraps and counts.  A sample's consecutive members form one CNV until a gap row comes before the next
 * member; the CNV is emitted at the first gap row after its last member, or by gd_emcnv_finish (emit row = the row
 * count) when (start[last row] + 100000 - end[a]) mod 2^32 >= 30000, and never otherwise.  As in the reference, sample 0
 * loses its list in every Clear that finds any list: it yields single-site CNVs only, when the next row is a gap.
 * PSize is the number of samples holding a list when the CNV is emitted.  CNVs are ordered by (emit row, sample) --
 * the reference's order within one Clear is Go's map order -- and a CNV's members by row.
 *   gd_emcnv_begin      n_samples as gd_emdepth; drops an earlier state (a refused call does not)
 *   gd_emcnv_add        depths: host float32 [n_rows][n_samples], finite and >= 0; starts, ends: host [n_rows];
 *                       cn_out: NULL or host [n_rows][n_samples], the copy numbers gd_emdepth gives
 *   gd_emcnv_add_cells  d_cells: DEVICE int64 [n_rows][n_samples], scale: host [n_samples] or NULL, as gd_emdepth_cells
 *   gd_emcnv_finish     Clear(nil); the counts.  No rows at all: 0 and 0.  gd_emcnv_add* is GD_E_STATE afterwards.
 *   gd_emcnv_read       after gd_emcnv_finish (GD_E_STATE before); any output may be NULL.  member_off[k] .. [k + 1] are
 *                       CNV k's members in member_row (input row), depth, cn and log2fc (float32 of the float64 value).
 *   gd_emcnv_end        frees the state (gd_destroy does too)
 *   gd_emcnv_timing     seconds since gd_emcnv_begin: upload, emdepth kernel, CNV kernels, read-back; min(n, 4) values
 * A refused call leaves the state as it was.  Apart from cn_out, what is copied back is O(CNVs + members). */
int gd_emcnv_begin(gd_ctx* ctx, int n_samples);
int gd_emcnv_add(gd_ctx* ctx, const float* depths, size_t n_rows, const uint32_t* starts, const uint32_t* ends, uint8_t* cn_out);
int gd_emcnv_add_cells(gd_ctx* ctx, const int64_t* d_cells, size_t n_rows, const float* scale, const uint32_t* starts,
                       const uint32_t* ends, uint8_t* cn_out);
int gd_emcnv_finish(gd_ctx* ctx, uint64_t* n_cnvs, uint64_t* n_members);
int gd_emcnv_read(gd_ctx* ctx, uint32_t* sample /* [n_cnvs] */, uint32_t* psize, uint32_t* emit_row,
                  uint64_t* member_off /* [n_cnvs + 1] */, uint32_t* member_row /* [n_members] */, float* depth, uint8_t* cn,
                  float* log2fc);
int gd_emcnv_end(gd_ctx* ctx);
int gd_emcnv_timing(gd_ctx* ctx, double* out, size_t n);
/* ---- dcnv's SampleMedians (dcnv/dcnv.go:108-125): one order statistic per sample of a sites x samples matrix ----
 * For sample s over all n_rows rows: with the column sorted ascending, k its leading zeros (-0.0 is a zero) and
 * n = n_rows - k, med[s] = sorted[k + (int)(0.65 * (double)n)] -- the 0.65 quantile of the non-zero depths, not the median,
 * the product taken in float64 and truncated -- and n_nonzero[s] = n.  An all-zero column (the reference panics) gives 0
 * and 0.  The selection is exact (a radix select over the bit patterns on the device): med[s] is a value of the column.
 * n_samples is 1 .. 4096 and n_rows 1 .. 2^31 - 1, GD_E_RANGE otherwise.  n_nonzero may be NULL.  Nothing is kept between
 * calls; the temporaries are freed on return; a refused call leaves the context usable.
 *   gd_sample_medians        depths: host float32 [n_rows][n_samples], each finite and >= 0 (GD_E_INVALID otherwise, found
 *                            before anything runs)
 *   gd_sample_medians_cells  d_cells: DEVICE int64 [n_rows][n_samples] as gd_depthwed_device leaves them; exact for every
 *                            non-negative int64 (nothing passes through a float).  A negative cell is found by the
 *                            first pass over the matrix: GD_E_INVALID, nothing written.  The matrix does not leave HBM.
 * gd_sample_medians_timing: seconds of the last call (measurement only): upload, kernels, read-back; a fourth value, when
 * asked for, is the number of passes over the matrix the call ran.  Fills min(n, 4) values. */
int gd_sample_medians(gd_ctx* ctx, const float* depths, size_t n_rows, int n_samples, float* med /* [n_samples] */,
                      uint64_t* n_nonzero /* [n_samples] or NULL */);
int gd_sample_medians_cells(gd_ctx* ctx, const int64_t* d_cells, size_t n_rows, int n_samples, int64_t* med,
                            uint64_t* n_nonzero);
int gd_sample_medians_timing(gd_ctx* ctx, double* out, size_t n);
/* ---- dcnv's ChunkDebiaser (dcnv/debiaser/debiaser.go:125-171): a depth matrix freed of a per-row covariate's bias ----
 * vals[r] is the covariate of row r (GC content, say).  The rows, taken in ascending vals order, are cut into chunks: the
 * first row opens one, and a row whose value exceeds the value that OPENED the current chunk by more than score_window (a
 * float64 subtraction, strictly greater) opens the next.  For every chunk and sample: with the n cells sorted ascending and
 * k the leading zeros (-0.0 is a zero), median = sorted[(n - k) / 2] -- the index counts from the start, so n < 3k gives 0;
 * when the median is > 0 every cell becomes (double)d / (double)median, otherwise the cells stay.  out gets the quotients
 * narrowed to float32 (an overflow is stored as the IEEE result, inf), out64 (or NULL) the float64 quotients themselves: for
 * a matrix whose cells are float32 values these are the reference's, bit for bit, whatever order its argsort gives tied
 * vals.  chunk_of_row (or NULL) gets every row's chunk, n_chunks (or NULL) their number C, med (or NULL) the C x n_samples
 * medians (values of the matrix, +0.0 for a zero); med_rows is med's capacity in rows: fewer than C is GD_E_CAPACITY (with
 * n_chunks set).  n_samples is 1 .. 4096 and n_rows 1 .. 2^31 - 1, GD_E_RANGE otherwise; a depth that is not finite and
 * >= 0, a val that is not finite, a score_window that is not finite and > 0 (the reference panics on 0): GD_E_INVALID.  All
 * refusals happen before anything runs and leave the context usable.  The argsort and the chunk walk are host work inside
 * the call; nothing is kept between calls; the temporaries are freed on return.
 * gd_chunk_debias_timing (measurement only), of the last call: seconds of host sort + chunking, upload, kernels, read-back;
 * then the chunk count and the rows of the largest chunk; a seventh value is the median kernel's seconds alone when the
 * environment has GOLEFT_CHUNKDEBIAS_SPLIT (the kernels are then synchronised apart).  Fills min(n, 7) values. */
int gd_chunk_debias(gd_ctx* ctx, const float* depths, size_t n_rows, int n_samples, const double* vals /* [n_rows] */,
                    double score_window, float* out /* [n_rows][n_samples] */, double* out64 /* same shape or NULL */,
                    uint32_t* chunk_of_row /* [n_rows] or NULL */, size_t* n_chunks /* or NULL */,
                    float* med /* [n_chunks][n_samples] or NULL; capacity med_rows */, size_t med_rows);
int gd_chunk_debias_timing(gd_ctx* ctx, double* out, size_t n);
/* ---- the matrix stays in HBM: debias, normalise and call CNVs on gd_depthwed_device's cells ----
 * Every d_* argument is a DEVICE pointer (gd_device_alloc, or any allocation of the context's device); everything else is
 * host memory.  Added without a revision; look them up by symbol.
 *   gd_chunk_debias_cells     gd_chunk_debias for d_cells, DEVICE int64 [n_rows][n_samples] as gd_depthwed_device leaves
 *                             them: d_out, a caller-owned DEVICE float32 matrix of the same shape, receives the quotients --
 *                             bit for bit what gd_chunk_debias gives for (float)cell, one rounding to nearest even.  vals,
 *                             the chunking, chunk_of_row, n_chunks, med, med_rows and every refusal are gd_chunk_debias's;
 *                             besides: d_out overlapping d_cells is GD_E_INVALID before anything runs, and a negative cell
 *                             (found by the pass that converts) is GD_E_INVALID with the host outputs untouched and d_out
 *                             unspecified.  gd_chunk_debias_timing reports this call too: its upload is the three tables of
 *                             the chunking, its kernels include the conversion, its read-back is med.
 *   gd_device_scale           d_depths[r][s] = d_depths[r][s] * scale[s] in float32, in place: what `emdepth --scales` does
 *                             to a cell.  scale: host [n_samples], each finite and >= 0 (GD_E_INVALID otherwise, nothing
 *                             touched); n_samples 1 .. 4096 (GD_E_RANGE); n_rows == 0 is GD_OK.  The cells are not checked.
 *   gd_sample_medians_device  gd_sample_medians,
 *   gd_emdepth_device         gd_emdepth and
 *   gd_emcnv_add_device       gd_emcnv_add for a DEVICE float32 matrix: no host validation, no upload.  A pass over the matrix
 *                             first finds a cell that is not finite and >= 0 (-0.0 and denormals pass, as on the host):
 *                             GD_E_INVALID, gd_last_error naming the row and sample of the first one, nothing written, the
 *                             context and any gd_emcnv state as they were.  Then the same kernels on the same bits: every
 *                             output is byte for byte the host twin's.  Ranges, n_rows == 0 and GD_E_STATE as for the twins.
 *                             The matrix is only read. */
int gd_chunk_debias_cells(gd_ctx* ctx, const int64_t* d_cells, size_t n_rows, int n_samples, const double* vals /* [n_rows] */,
                          double score_window, float* d_out /* DEVICE [n_rows][n_samples] */,
                          uint32_t* chunk_of_row /* [n_rows] or NULL */, size_t* n_chunks /* or NULL */,
                          float* med /* [n_chunks][n_samples] or NULL; capacity med_rows */, size_t med_rows);
int gd_device_scale(gd_ctx* ctx, float* d_depths, size_t n_rows, int n_samples, const float* scale /* [n_samples] */);
int gd_sample_medians_device(gd_ctx* ctx, const float* d_depths, size_t n_rows, int n_samples, float* med /* [n_samples] */,
                             uint64_t* n_nonzero /* [n_samples] or NULL */);
int gd_emdepth_device(gd_ctx* ctx, const float* d_depths, size_t n_rows, int n_samples, double* lambda, uint8_t* iters,
                      uint8_t* cn, float* log2fc);
int gd_emcnv_add_device(gd_ctx* ctx, const float* d_depths, size_t n_rows, const uint32_t* starts, const uint32_t* ends,
                        uint8_t* cn_out);
/* ---- moving-median debias: dcnv's GeneralDebiaser, the debiaser dcnv's main runs with Window = 9 ----
 * Added without a revision; look them up by symbol.  The rows are taken in ascending order of vals, tied vals by row index
 * (the reference's argsort is unstable there).  For every sample, with c[0 .. R) its column in that order, W = window (odd,
 * 1 .. 255) and mid = (W - 1) / 2 + 1, the reference pushes P[t] = c[t] (t < mid), c[t + mid] (t >= mid) -- rows
 * mid .. 2 mid - 1 never enter a window -- and divides row i by the median of P[lo .. hi): hi = mid for i < mid, else
 * min(i + 1, max(mid, R - mid)); lo = max(0, hi - W).  The median of a full window is its (W + 1) / 2-th smallest value; of
 * m < W values it is (sorted[(m - 1) / 2] + sorted[m / 2]) / 2 in float64 (this library's definition: the reference's
 * moving-median library is not part of it).  out[row][s] = (float)((double)c[i] / max(median, 1.0)), at the row's original
 * place; med (or NULL) gets the medians themselves, before the max (-0.0 counts as 0.0 there).  n_samples is 1 .. 4096;
 * window even or outside 1 .. 255, n_rows < mid (the reference indexes past the column) or > 2^31 - 1: GD_E_RANGE; a depth
 * that is not finite and >= 0, a val that is not finite: GD_E_INVALID.  All refusals happen before anything runs and leave
 * the context usable.  The argsort is host work inside the call; nothing is kept between calls.
 *   gd_moving_debias_cells    the same for d_cells, DEVICE int64 [n_rows][n_samples] as gd_depthwed_device leaves them:
 *                             d_out, a caller-owned DEVICE float32 matrix of the same shape, receives what gd_moving_debias
 *                             gives for (float)cell, bit for bit.  d_out overlapping d_cells is GD_E_INVALID before anything
 *                             runs; a negative cell (found by the pass that converts) is GD_E_INVALID with d_out untouched.
 *                             The call holds a float32 copy of the matrix of its own while it runs.
 *   gd_moving_debias_timing   (measurement only) of the last call: seconds of host sort, upload, kernels (the conversion
 *                             included), read-back.  Fills min(n, 4) values. */
int gd_moving_debias(gd_ctx* ctx, const float* depths, size_t n_rows, int n_samples, const double* vals /* [n_rows] */,
                     int window, float* out /* [n_rows][n_samples] */, double* med /* same shape or NULL */);
int gd_moving_debias_cells(gd_ctx* ctx, const int64_t* d_cells, size_t n_rows, int n_samples, const double* vals /* [n_rows] */,
                           int window, float* d_out /* DEVICE [n_rows][n_samples] */);
int gd_moving_debias_timing(gd_ctx* ctx, double* out, size_t n);
/* ---- SVD debias: dcnv's SVD debiaser flanked by its z-score scaler ----
 * Added without a revision; look them up by symbol.  depths is [n_rows][n_samples] float32, every cell finite and >= 0,
 * taken to float64.  With zscore every row i gets m_i = sum / N and sd_i, the sample standard deviation (N - 1, two-pass),
 * and z_ij = (a_ij - m_i) / sd_i -- 0 for the whole row when sd_i == 0 (this library's choice: the reference divides by 0
 * there and its factorisation panics); without, Z = A.  s is the singular values of Z, descending, min(n_rows, n_samples) of
 * them, from the eigenvalues of the float64 Gram matrix Z^T Z the device sums (s = sqrt(max(w, 0)): values below about
 * 1e-8 of s[0] are not resolved).  n counts the leading values with 100 s[n] / sum(s) > min_variance_pct, at most
 * min(15, n_rows, n_samples) (the reference stops at 15 and reads past the end of fewer; an all-zero Z gives n = 0).
 * Z' = Z - (Z V_n) V_n^T with V_n the first n right singular vectors -- the reference's U Sigma' V^T -- and
 * out = (float)z', or (float)max(0, z' sd_i + m_i) with zscore (ZScore.UnScale): one rounding to float32.  s (or NULL) gets
 * the spectrum, n_removed (or NULL) n.  Two calls on the same input give the same bytes, and the three forms give the same
 * bytes for the same float32 matrix.  2 <= n_samples <= 1024 (the eigenpairs are O(n_samples^3) host work inside the call:
 * about a second at 1024), 1 <= n_rows <= 2^31 - 1, min_variance_pct finite and >= 0: GD_E_RANGE otherwise; a cell that is
 * not finite and >= 0: GD_E_INVALID, gd_last_error naming its row and sample.  All refusals leave the context usable.
 * While it runs the call holds 32 KB per 1024 rows and pair of 64-sample tiles on the device.
 *   gd_svd_debias_cells    the same for d_cells, DEVICE int64 [n_rows][n_samples] as gd_depthwed_device leaves them: d_out,
 *                          a caller-owned DEVICE float32 matrix of the same shape, receives what gd_svd_debias gives for
 *                          (float)cell.  d_out overlapping d_cells is GD_E_INVALID before anything runs; a negative cell is
 *                          GD_E_INVALID with d_out unspecified.
 *   gd_svd_debias_device   the same for a DEVICE float32 matrix, checked on the device first; d_out may be d_depths itself
 *                          (every row is read before it is written), any other overlap is GD_E_INVALID.
 *   gd_svd_debias_timing   (measurement only) of the last call: seconds of upload (cells: conversion and check; device:
 *                          check), row statistics + Gram matrix and its read-back, eigenpairs on the host, projection,
 *                          read-back.  Fills min(n, 5) values. */
int gd_svd_debias(gd_ctx* ctx, const float* depths, size_t n_rows, int n_samples, double min_variance_pct, int zscore,
                  float* out /* [n_rows][n_samples] */, double* s /* [min(n_rows, n_samples)] or NULL */,
                  int* n_removed /* or NULL */);
int gd_svd_debias_cells(gd_ctx* ctx, const int64_t* d_cells, size_t n_rows, int n_samples, double min_variance_pct, int zscore,
                        float* d_out /* DEVICE [n_rows][n_samples] */, double* s, int* n_removed);
int gd_svd_debias_device(gd_ctx* ctx, const float* d_depths, size_t n_rows, int n_samples, double min_variance_pct, int zscore,
                         float* d_out /* DEVICE [n_rows][n_samples]; may equal d_depths */, double* s, int* n_removed);
int gd_svd_debias_timing(gd_ctx* ctx, double* out, size_t n);
/* The same three with the scaler named: GD_SVD_SCALER_NONE and GD_SVD_SCALER_ZSCORE run what zscore 0 and 1 run above, any
 * other value but the three is GD_E_RANGE (the zscore argument above takes every non-zero value as 1, hence the new entries).
 * GD_SVD_SCALER_LOG2 is dcnv's Log2 scaler (dcnv/scalers/scalers.go:134-164 of the reference):
 * l_ij = log2(1 + a_ij); every SAMPLE is centred on c_j = sorted(l_.j)[n_rows / 2], its upper median over all rows, zeros
 * included (= log2(1 + m_j), m_j the cell of that rank); the spectrum, the cut and the projection above on z = l - c;
 * out_ij = (float)max(0, 2^(z'_ij + c_j) - 1).  The "- 1" and the clamp are this project's: the reference's UnScale returns
 * 2^x, depth + 1 after a round trip, which its own TestLog2RoundTrip refuses; a zero cell may leave the projection below 0.
 * centre_cells (or NULL; host, [n_samples]) gets m_j, and is untouched unless the scaler is log2.  Sizes, refusals, the
 * equal bytes from call to call and from form to form, d_out == d_depths and the timing slots are as above; the selection of
 * the centres counts into the second slot of gd_svd_debias_timing.  A refused call leaves its outputs untouched. */
enum { GD_SVD_SCALER_NONE = 0, GD_SVD_SCALER_ZSCORE = 1, GD_SVD_SCALER_LOG2 = 2 };
int gd_svd_debias_scaled(gd_ctx* ctx, const float* depths, size_t n_rows, int n_samples, double min_variance_pct, int scaler,
                         float* out /* [n_rows][n_samples] */, double* s /* [min(n_rows, n_samples)] or NULL */,
                         int* n_removed /* or NULL */, float* centre_cells /* [n_samples] or NULL */);
int gd_svd_debias_scaled_cells(gd_ctx* ctx, const int64_t* d_cells, size_t n_rows, int n_samples, double min_variance_pct,
                               int scaler, float* d_out /* DEVICE [n_rows][n_samples] */, double* s, int* n_removed,
                               float* centre_cells);
int gd_svd_debias_scaled_device(gd_ctx* ctx, const float* d_depths, size_t n_rows, int n_samples, double min_variance_pct,
                                int scaler, float* d_out /* DEVICE [n_rows][n_samples]; may equal d_depths */, double* s,
                                int* n_removed, float* centre_cells);
/* ---- cnveval.Evaluate (cnveval/cnveval.go:163-341 of the reference): the calls of every sample
 * scored against a truth set, on the device.  One host form: the inputs are kilobytes to megabytes.
 *   samples     ids 0 .. n_samples - 1: the union of the samples of both sets.
 *   calls       grouped by sample: sample s owns [cnv_off[s], cnv_off[s + 1]) of the four int32 arrays (chromosome rank,
 *               start, end, copy number), in (chromosome rank, start) order within the sample -- where two calls of a
 *               sample tie, the order given is the order taken.  A rank is any integer >= 0 that orders the chromosomes
 *               as the caller wants them ordered (the reference: their names as byte strings), the same in both sets.
 *   truths      n_truths intervals (rank, start, end, copy number) in any order; truth t names the samples
 *               t_samples[t_off[t] .. t_off[t + 1]) -- a sample named twice counts twice, as in the reference.
 *   min_overlap above 0, at most 1.
 *   stats       host, [n_samples][3][4]: size class (length below 20000, below 100000, the rest) by FP, FN, TP, TN.  A
 *               sample without calls is not evaluated: its twelve counts are 0.
 * A call matches a truth on its chromosome when overlap / min(lengths) >= min_overlap (one float64 division; a zero
 * length matches nothing) and the copy numbers are equal after those above 2 become 3.  The counts are the reference's
 * to the last one, its quirks included, and two calls give the same bytes.
 * Everything is checked before anything runs, and a refused call leaves stats untouched: min_overlap, the limits below,
 * a negative start or rank, end < start or a sample id outside the samples GD_E_RANGE; offsets that do not start at 0 or
 * decrease GD_E_INVALID; calls of a sample out of order GD_E_UNSORTED -- each with the index in gd_last_error.  No calls
 * or no truths is valid.
 * gd_cnveval_timing: seconds of the last call (measurement only): preparation and upload, kernels, read-back, and as a
 * fourth value the part of the second that the first kernel (the truths that name a sample) took.  Fills min(n, 4) values. */
#define GD_CNVEVAL_MAX_SAMPLES (1 << 20)
#define GD_CNVEVAL_MAX_TRUTHS (1 << 24)
#define GD_CNVEVAL_MAX_CNVS (1 << 26)
#define GD_CNVEVAL_MAX_ENTRIES (1 << 28)        /* (truth, sample) namings */
#define GD_CNVEVAL_MAX_MEMBER_WORDS (1 << 28)   /* n_truths * ceil(n_samples / 32): 1 GiB of membership bits */
int gd_cnveval(gd_ctx* ctx, int32_t n_samples, const int64_t* cnv_off /* [n_samples + 1] */, const int32_t* cnv_chrom,
               const int32_t* cnv_start, const int32_t* cnv_end, const int32_t* cnv_cn, size_t n_truths,
               const int32_t* t_chrom, const int32_t* t_start, const int32_t* t_end, const int32_t* t_cn,
               const int64_t* t_off /* [n_truths + 1] */, const int32_t* t_samples, double min_overlap,
               int64_t* stats /* [n_samples][3][4] */);
int gd_cnveval_timing(gd_ctx* ctx, double* out, size_t n);
/* ---- the per-base vector of a region as runs of equal value: what bedGraph, mosdepth's
 * per-base.bed and `bedtools genomecov -bga` hold, run-length encoded on the device so that only the runs cross the link.
 * After a gd_compute with GD_OUT_PERBASE, for contig tid of length len, a region 0 <= start <= end <= len and the
 * computed per-base vector d:
 *   value     with n_cuts == 0, v(p) = d[p]; otherwise v(p) = the number of cuts <= d[p]: the index, 0 .. n_cuts, of the bin
 *             [0, cuts[0]), [cuts[0], cuts[1]), ... [cuts[n_cuts - 1], inf) that holds the depth.  Cuts are strictly
 *             increasing, each 1 .. 2^31 - 1, at most GD_PERBASE_MAX_CUTS of them.
 *   run start position p starts a run iff p == start or v(p) != v(p - 1): the region's first position always does, even when
 *             d[start] == d[start - 1]; a change of depth inside one bin starts none.
 *   runs      run k is (run_start[k], run_value[k]), in ascending position; it ends at run_start[k + 1], the last one at
 *             `end`.  Runs of depth 0 are runs like any other; a contig without records is one run of 0; start == end
 *             gives no runs and GD_OK.
 * The call pattern is gd_callable's: *n always receives the number of runs; GD_E_CAPACITY when cap is below it or an output
 * is NULL (NULL and 0 is how a caller asks for the count), and the outputs are then untouched.  GD_E_RANGE: a region outside
 * 0 <= start <= end <= len, a tid that is none or was not selected; GD_E_INVALID: cuts that do not increase, a cut below 1,
 * more than GD_PERBASE_MAX_CUTS; GD_E_STATE: before a compute, while one is in flight, or when the context was computed
 * without GD_OUT_PERBASE.  A refused call leaves the context as it was.  Two calls give the same bytes.
 * gd_perbase_runs_timing: seconds of the last call (measurement only): the count kernel, the scan with the read of the
 * count, the emit kernel, the read-back (the last two are 0 after a call that only counted).  Fills min(n, 4) values.
 * Added without a revision, as the entry points before them: look them up by symbol. */
#define GD_PERBASE_MAX_CUTS 32
int gd_perbase_runs(gd_ctx* ctx, int32_t tid, int64_t start, int64_t end, int n_cuts, const int32_t* cuts /* [n_cuts] or NULL */,
                    uint32_t* run_start, int32_t* run_value, size_t cap, size_t* n);
int gd_perbase_runs_timing(gd_ctx* ctx, double* out, size_t n);
/* ---- the per-base vector reduced along the depth axis: what mosdepth's *.dist.txt, *.summary.txt
 * and *.thresholds.bed are made of, counted on the device so that a few kilobytes cross the link.  After a gd_compute with
 * GD_OUT_PERBASE.  Region r is [start[r], end[r]) on contig tid[r], 0 <= start <= end <= that contig's length; regions may
 * overlap, repeat, be empty and come in any order, and n_regions == 0 is GD_OK.
 *   gd_depth_hist   one histogram over the multiset of all positions of all regions (a position that two regions hold counts
 *                   twice): bins[k] = the number of positions p with min(d[p], n_bins - 1) == k, 1 <= n_bins <=
 *                   GD_DEPTH_HIST_MAX_BINS; *sum = the sum of d[p], *min and *max over the same positions, not clamped.  Each
 *                   of sum, min, max may be NULL.  Without a position every bin, *sum, *min and *max are 0.
 *   gd_region_bins  for every region on its own: counts[r * (n_cuts + 1) + b] = the number of its positions whose number of
 *                   cuts <= d[p] is b (gd_perbase_runs' value with cuts, and its rules for them).  n_cuts == 0: one column,
 *                   the region's length.  The number of positions at or above cut k is the sum of columns k + 1 .. n_cuts.
 * Both are exact integer counts: two calls give the same numbers.  The checks and their order are gd_perbase_runs':
 * GD_E_RANGE: a region outside 0 <= start <= end <= len, a tid that is none or was not selected, more positions than one
 * call takes (2^31 - 16 chunks of 4096 on each region's 16-byte grid); GD_E_INVALID: n_bins out of range, bad cuts, a NULL
 * that is needed; GD_E_STATE: before a compute, while one is in flight, or computed without GD_OUT_PERBASE.  Everything is
 * checked before anything is allocated or launched, and a refused call leaves the context and the outputs as they were.
 * gd_dist_timing: seconds of the last call of either (measurement only): the tables' upload with the zeroing, the kernel,
 * the read-back.  Fills min(n, 3) values.  Added without a revision, as the entry points before them. */
#define GD_DEPTH_HIST_MAX_BINS 65536
int gd_depth_hist(gd_ctx* ctx, size_t n_regions, const int32_t* tid, const int64_t* start, const int64_t* end,
                  int32_t n_bins, uint64_t* bins /* [n_bins] */, int64_t* sum, int32_t* min, int32_t* max);
int gd_region_bins(gd_ctx* ctx, size_t n_regions, const int32_t* tid, const int64_t* start, const int64_t* end,
                   int n_cuts, const int32_t* cuts /* [n_cuts] or NULL */, uint64_t* counts /* [n_regions][n_cuts + 1] */);
int gd_dist_timing(gd_ctx* ctx, double* out, size_t n);
int gd_ingest_abort(gd_ctx* ctx);
/* Page-locked host memory for the byte range handed to gd_ingest_bgzf (read the file
 * straight into it: the H2D copy then runs at PCIe speed instead of through a bounce
 * buffer).  Plain pageable memory works too, only slower. */
int gd_host_alloc(gd_ctx* ctx, size_t bytes, void** out);
int gd_host_free(gd_ctx* ctx, void* p);

/* Device-side views of the results (for RCCL gathers and zero-copy
 * consumers).  Pointers stay valid until the next gd_compute/gd_reset. */
int gd_device_perbase(gd_ctx* ctx, int32_t tid, const int32_t** dptr, int64_t* len);
int gd_device_windows(gd_ctx* ctx, const int64_t** d_sums, const int32_t** d_mins,
                      size_t* n_total);
/* Window offset of contig tid inside the concatenated window arrays. */
int gd_window_offset(gd_ctx* ctx, int32_t tid, size_t* off, size_t* n);
/* Ordered run boundaries {pos, cls | tid<<2} of all contigs. */
int gd_device_runs(gd_ctx* ctx, const int32_t** d_bounds, size_t* n_bounds);

/* Packed export block for a merge step (the reference's merge loop, depth/depth.go:394-421, run by
 * one rank for N workers): when device_buf is not NULL, every gd_compute also writes -- before its
 * single synchronisation, no extra launch latency -- the int64 words
 *     [n_bounds][sums: max_windows][mins: ceil(max_windows / 2) words of int32 pairs][bounds: cap_bounds]
 * into that caller-owned device buffer (e.g. an RCCL send buffer), so the exchange is one collective
 * on one buffer with no host round trip for sizes.  n_bounds is the true boundary count (it may
 * exceed cap_bounds: the receiver must check); the window arrays hold the computed contigs in
 * ascending tid order; a boundary is {int32 pos, int32 cls | index_among_computed_contigs << 2}.
 * GD_E_CAPACITY from gd_compute if the job has more windows than max_windows.  NULL switches it off. */
int gd_set_export(gd_ctx* ctx, void* device_buf, int64_t max_windows, int64_t cap_bounds);
/* Everything this context enqueues from now on waits for `hip_event` (a hipEvent_t the caller recorded on a
 * stream of its own, passed as void*): how a caller that hands the export block to a collective tells the
 * engine "the collective that was still reading this buffer is over" without blocking the host
 * (hipStreamWaitEvent on the context's stream). */
int gd_wait_event(gd_ctx* ctx, void* hip_event);

/* ---- the exchange step: export blocks to one root over RCCL (xGMI between the GPUs of a node) ----------------
 * One context per GPU, one rank per context -- in one process (a worker thread per device, the counterpart of the
 * reference's `-p` pool, depth/depth.go:392-394) or one process per GPU.  The root owns the BED files like the
 * reference's merge loop (depth/depth.go:394-421) and receives every rank's export block (gd_set_export: window sums,
 * minima, ordered class-run boundaries; the boundary count travels in word 0) with ONE grouped send / receive.
 *   gd_comm_unique_id   on one rank; the 128 bytes reach the others by whatever means the host has (a Go channel,
 *                       a file, MPI, torch.distributed)
 *   gd_comm_init        collective over the `world` contexts; librccl is opened here, on first use (dlopen): a
 *                       single-GPU run never loads it.  GD_E_NODEVICE: no RCCL on this machine
 *   gd_gather_export    after a gd_compute: `words` int64 words -- send == NULL: the export block (words == 0: all
 *                       of it) -- to `root`, which receives rank r's at recv + r * words (every rank passes the same
 *                       `words`).  Asynchronous: issued on the context's copy stream behind the compute that filled
 *                       the block, so it runs under the kernels of the next gd_compute; with two export buffers
 *                       alternating (gd_set_export before each compute) nothing is written into a buffer a gather
 *                       may still read -- the compute stream waits for the gather before the last one
 *   gd_gather_wait      the host waits until every gather issued so far has landed */
#define GD_COMM_ID_BYTES 128
int gd_comm_unique_id(void* id, size_t bytes);
/* Which RCCL the calls above use: its path into `out` (NUL terminated, cut to `cap`); *shared = 1 when the process had one
 * mapped already -- a host that imported torch has torch's own copy, and that one is used: never two RCCLs in one process --
 * 0 when the library opened librccl.so.1 by name.  GD_E_NODEVICE: none on this machine.  Local and cheap: every rank can
 * ask BEFORE any rank enters the collective gd_comm_init (a rank that cannot open RCCL would leave the others waiting there). */
int gd_comm_library(char* out, size_t cap, int* shared);
int gd_comm_init(gd_ctx* ctx, int rank, int world, const void* id, size_t bytes);
int gd_comm_destroy(gd_ctx* ctx);
int gd_gather_export(gd_ctx* ctx, const int64_t* send, int64_t* recv, size_t words, int root);
int gd_gather_wait(gd_ctx* ctx);
/* Device memory for a host that has no HIP binding of its own (cgo): the send / receive buffers of gd_gather_export, and
 * a synchronous read of them (waits for the context's streams first). */
int gd_device_alloc(gd_ctx* ctx, size_t bytes, void** out);
int gd_device_free(gd_ctx* ctx, void* p);
int gd_device_read(gd_ctx* ctx, void* dst_host, const void* src_device, size_t bytes);

/* ---- measurement ---------------------------------------------------------*/
int gd_get_stats(gd_ctx* ctx, gd_stats* out);
/* HIP-event timing of the kernels of the last gd_compute, recorded on the
 * stream the kernels ran on.  Enable before gd_compute. */
int gd_set_profiling(gd_ctx* ctx, int on);
int gd_kernel_ms(gd_ctx* ctx, int kernel_id, float* ms);
/* Host wall clock of the last gd_compute (or launch + finish pair), seconds[0 .. n): [0] contig table + device
 * allocations (what only a context's FIRST compute of a job size pays), [1] enqueueing the launches, [2] the wait
 * for the device incl. verification, re-runs and publishing, [3] their total.  What the reference's counterpart
 * spends per tile on fork/exec and pipes (depth/depth.go:392-394) is here one number per genome. */
int gd_compute_timing(gd_ctx* ctx, double* seconds, int n);

#ifdef __cplusplus
}
#endif
#endif /* GOLEFT_DEPTH_H */
