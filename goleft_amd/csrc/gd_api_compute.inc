// gd_api_compute.inc -- gd_compute: contig table, allocations, the launch sequence of the three device
// algorithms and the verified look-back (part of gd_api.hip, inside extern "C").

// gd_compute is three steps over one ComputeState (gd_ctx::cs): PREPARE (contig table, allocations), then per
// attempt ENQUEUE (every launch of the chosen path + the read-back copies, no host synchronisation) and COMPLETE
// (the one synchronisation, the verified look-back / capacity checks: 1 = enqueue again), then PUBLISH.
// gd_compute_launch = prepare + enqueue, gd_compute_finish = complete (+ re-runs) + publish: a caller with other
// work for the host -- issuing the collective of the PREVIOUS step, say -- does it between the two.

// What the tile path may run on the job as it stands: the alignment the straight-line kernel's vector loads need.
static void compute_survey(gd_ctx* c, ComputeState& S)
{
    S.raw_aligned = true;
    for (int32_t tid : S.tids) {
        const ContigHost& h = c->contigs[tid];
        if (h.length <= 0) continue;
        if (h.n_reads)
            S.raw_aligned = S.raw_aligned && (reinterpret_cast<uintptr_t>(h.pos.get()) & 15u) == 0 &&
                            (reinterpret_cast<uintptr_t>(h.off.get()) & 15u) == 0 && (reinterpret_cast<uintptr_t>(h.flag.get()) & 7u) == 0 &&
                            (reinterpret_cast<uintptr_t>(h.mapq.get()) & 3u) == 0;
    }
}

// The contig table.
static void compute_build_table(gd_ctx* c, ComputeState& S)
{
    constexpr int T = kTileT;
    const gd_params& P = c->params;
    c->h_ctgs.clear();
    c->job_tids.clear();
    S.tile_beg = S.base_off = S.win_off = S.bases = 0;
    S.n_units = 0;
    S.n_groups = 0;
    for (int32_t tid : S.tids) {
        ContigHost& h = c->contigs[tid];
        if (h.length <= 0) continue;
        gd::ContigDev d{};
        d.pos = h.pos; d.flag = h.flag; d.mapq = h.mapq;
        d.off = h.off;
        d.cigar = h.cigar;
        d.pidx = h.ridx && h.n_reads && h.ridx_reads == h.n_reads ? h.ridx : nullptr;
        d.pidx_last = (uint32_t)std::min<int64_t>((int64_t)h.last_pos >> 6, (h.length >> 6) + 1);
        d.pad_ = 0;
        d.n_reads = (uint32_t)h.n_reads;
        d.n_ops = (uint32_t)h.n_ops;
        d.length = (int32_t)h.length;
        d.tile_beg = (int32_t)S.tile_beg;
        d.n_tiles = (int32_t)((h.length + T - 1) / T);
        d.base_off = S.base_off;
        d.win_off = S.win_off;
        d.tid = tid;
        d.unit_beg = (uint32_t)S.n_units;
        d.lrec = h.ck_ok ? h.lrec : nullptr;
        d.lfq = h.ck_ok ? h.lfq : nullptr;
        d.dl = h.ck_ok ? h.dl : nullptr;
        d.pck = h.ck_ok ? h.pck : nullptr;
        d.ndel = h.ck_ok ? h.ndel : nullptr;
        d.grp_beg = (uint32_t)S.n_groups;
        S.n_units += (h.n_reads + 63) / 64;
        S.n_groups += (h.n_reads + gd::sums::GROUP * gd::sums::GPW - 1) / (gd::sums::GROUP * gd::sums::GPW);   // reads per wave
        h.base_off = S.base_off;
        h.win_off = S.win_off;
        h.n_win = (h.length + P.window_size - 1) / P.window_size;
        S.tile_beg += d.n_tiles;
        S.base_off += (int64_t)d.n_tiles * T;
        S.win_off += h.n_win;
        S.bases += h.length;
        c->h_ctgs.push_back(d);
        c->job_tids.push_back(tid);
    }
}

// The contigs of a job: the selected ones, else all.
static std::vector<int32_t> selected_or_all(const gd_ctx* c)
{
    std::vector<int32_t> tids = c->selected;
    if (tids.empty()) { tids.resize(c->contigs.size()); for (size_t i = 0; i < tids.size(); ++i) tids[i] = (int32_t)i; }
    return tids;
}

// 0 = ready to enqueue, 1 = nothing to compute (no tiles), < 0 error
static int compute_prepare(gd_ctx* c, ComputeState& S)
{
    if (int r = set_device(c)) return r;
    if (c->contigs.empty()) return fail(c, GD_E_STATE, "gd_set_contigs has not been called");
    bool ing_holds = false;
    for (const auto& b : c->ing_bufs) ing_holds = ing_holds || b.in;
    if (c->ing_n == 0 && ing_holds) {
        // the BAM read is over: its buffers go back -- when the results need the room (giving 35 GB back takes a
        // second; a genome's records and results leave 200 GB of HBM unused)
        size_t fr = 0, tot = 0, need = 16ull << 30;
        for (const auto& h : c->contigs) need += (size_t)h.length * (c->keep_perbase ? 5 : 1);
        if (hipMemGetInfo(&fr, &tot) != hipSuccess || fr < need)
            for (auto& b : c->ing_bufs) b.drop();
    }
    c->computed = false;                                 // until compute_publish: the result arrays are about to be overwritten

    // ---- contig table ------------------------------------------------------
    S.tids = selected_or_all(c);
    for (auto& h : c->contigs) { h.base_off = h.win_off = -1; h.n_win = 0; h.run_beg = h.run_end = 0; }
    {
        const float ck_ms = c->kernel_ms[GD_K_CKPT];     // ingest-time work
        memset(c->kernel_ms, 0, sizeof c->kernel_ms);
        c->kernel_ms[GD_K_CKPT] = ck_ms;
    }
    S.n_reads = S.n_ops = 0;
    for (int32_t tid : S.tids)
        if (c->contigs[tid].length > 0) { S.n_reads += c->contigs[tid].n_reads; S.n_ops += c->contigs[tid].n_ops; }
    compute_survey(c, S);
    compute_build_table(c, S);                           // (for the layout totals; the enqueue builds the table it uploads)
    if (S.tile_beg > 0x7fffffffLL) return fail(c, GD_E_RANGE, "too many tiles");
    if (S.n_units > 0xfffffff0ull) return fail(c, GD_E_RANGE, "too many records");
    c->n_tiles = S.tile_beg;
    c->n_win_total = S.win_off;
    c->n_bases = S.bases;
    c->bounds.clear();
    S.route = GD_TK_NONE;                                // (until an enqueue decides it)
    if (c->n_tiles == 0) return 1;
    if (c->export_buf && c->n_win_total > c->export_max_w)
        return fail(c, GD_E_CAPACITY, "gd_set_export: %lld windows, the export block holds %lld",
                    (long long)c->n_win_total, (long long)c->export_max_w);

    // ---- allocations -------------------------------------------------------
    // (every array is asked on its own whether it has the room: arrays of one size grow in the same calls)
    if (int r = ensure_dev(c, c->d_ctgs, c->h_ctgs.size())) return r;
    if (int r = ensure_dev(c, c->d_tiles, (size_t)c->n_tiles)) return r;
    if (int r = ensure_dev(c, c->d_tile_cnt, (size_t)c->n_tiles)) return r;
    if (int r = ensure_dev(c, c->d_tile_off, (size_t)c->n_tiles)) return r;
    if (int r = ensure_dev(c, c->d_super_cnt, (size_t)c->n_tiles / gd::SUPER + 1)) return r;
    if (straight_line_allowed(c))                        // (allocations belong here, not in the enqueue)
        if (int r = ensure_dev(c, c->d_ftiles, (size_t)c->n_tiles)) return r;
    if (c->keep_perbase) {
        if (int r = ensure_dev(c, c->d_perbase, (size_t)S.base_off)) return r;
    } else if (c->d_perbase) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, c->d_perbase.reset_checked());     // windows-only: give the HBM back
    }
    if (int r = ensure_dev(c, c->d_wsum, (size_t)std::max<int64_t>(S.win_off, 1))) return r;
    if (int r = ensure_dev(c, c->d_wmin, (size_t)std::max<int64_t>(S.win_off, 1))) return r;
    if (!c->d_ordered) {                                 // (the second of the two: with it the pair is whole)
        const size_t want = std::max<size_t>(1u << 16, (size_t)c->n_tiles * 2);
        if (int r = ensure_dev(c, c->d_chunks, want)) return r;
        if (int r = ensure_dev(c, c->d_ordered, want)) return r;
    }
    // records staged on the copy stream must have landed
    HIPCHK(c, hipEventRecord(c->copy_done, c->copy_stream));
    HIPCHK(c, hipStreamWaitEvent(c->stream, c->copy_done, 0));
    if (c->ingest_span_dirty || c->commit_checks_pending) {
        // blocks have been committed since the host last looked: the largest span the index kernel has seen becomes
        // this compute's look-back (one 16-byte read per batch of commits, not per compute), and with GD_OPT_COMMIT_CHECK = 1
        // this is where records that failed their checks stop
        uint32_t w[3] = {0, 0, 0};
        if (int r = read_ingest_words(c, c->stream, w)) return r;
        if (c->commit_checks_pending)
            if (int r = commit_verdict(c)) return r;
        const int32_t span = (int32_t)w[1];
        if (c->ingest_span_dirty) take_ingest_span(c, span);
    }

    S.reruns = 0;
    S.used_lookback = c->lookback;
    return GD_OK;
}

// Profiling: the record that opens the stage `id` (a GD_K_* interval of gd_kernel_ms) and closes the one before it.
static constexpr int kStagesEnd = -1;                    // the record behind the last launch opens nothing
static int compute_stage(gd_ctx* c, ComputeState& S, int id)
{
    if (!c->profiling) return GD_OK;
    HIPCHK(c, hipEventRecord(c->ev[S.n_stages], c->stream));
    S.stage_id[S.n_stages++] = (int8_t)id;
    return GD_OK;
}

static int compute_enqueue(gd_ctx* c, ComputeState& S)
{
    const gd_params& P = c->params;
    // which device algorithm and kernel (include/goleft_depth.h GD_PATH_*, GD_TK_*)
    const int route = compute_route(c, S);
    if (route < 0)
        return fail(c, route, "windows-only output (gd_set_outputs without GD_OUT_PERBASE) is not "
                              "available on the scatter path");
    S.route = route;
    S.n_stages = 0;
    gd::Job job{};
    job.ctgs = c->d_ctgs;
    job.n_ctgs = (int32_t)c->h_ctgs.size();
    job.n_tiles = (int32_t)c->n_tiles;
    job.tiles = c->d_tiles;
    if (route == GD_TK_FAST_RAW) { job.fast = 1; job.ftiles = c->d_ftiles; }   // (the sums-only tile kernel reads the generic tile table)
    job.perbase = c->d_perbase;
    job.win_sum = c->d_wsum;
    job.win_min = c->d_wmin;
    job.n_win_total = c->n_win_total;
    job.run_chunks = c->d_chunks;
    job.run_cap = (uint32_t)std::min<size_t>(c->d_ordered.cap(), 0xffffffffu);
    job.tile_cnt = c->d_tile_cnt;
    job.tile_off = c->d_tile_off;
    job.super_cnt = c->d_super_cnt;
    job.counters = c->d_counters;
    job.W = P.window_size;
    job.Q = P.min_mapq;
    job.mincov = P.min_cov;
    job.maxmean = P.max_mean_depth;
    job.flag_mask = P.flag_mask;
    job.lookback = c->lookback;
    job.step = derive_step(P);
    magic_u31((uint32_t)job.W, &job.w_magic, &job.w_shift);
    magic_u31(job.step > 0x7fffffffLL ? 0x7fffffffu : (uint32_t)job.step, &job.s_magic, &job.s_shift);

    job.tile_status = c->d_status;
    job.parity = (c->parity ^= 1u);
    // gd_prep_kernel counts slow tiles in n_slow[parity] and zeroes the OTHER counter for the next compute; a
    // compute that ran without it (scatter path, streaming sums, an enqueue that failed) leaves this one stale
    if (!c->slow_counter_clean)
        HIPCHK(c, hipMemsetAsync(c->d_counters.as<char>() + offsetof(gd::Counters, n_slow) + job.parity * sizeof(uint32_t),
                                 0, sizeof(uint32_t), c->stream));
    c->slow_counter_clean = false;

    if (route == GD_TK_LONG) {
        // deletion lists, read records and tile indexes of every contig that lacks them, as ONE batch, straight from the
        // records as they arrived -- also for short-read data forced onto this path, or after a span made AUTO leave
        // the tile path.
        if (int r = ck_tids(c, S.tids)) return r;
        S.chunk_span = 0;
        for (int32_t tid : S.tids) {
            const ContigHost& h = c->contigs[tid];
            if (h.length > 0) S.chunk_span = std::max(S.chunk_span, h.max_span);
        }
        // the look-back IS the largest span (exact, known since the records arrived)
        job.lookback = std::max(64, (int32_t)((S.chunk_span + 63) & ~63));
        S.used_lookback = job.lookback;                  // (gd_stats.lookback: what the tile table was built with)
    }
    // compute_prepare built the table for its totals; this is the one that is uploaded: the long-read pointers in it
    // only exist after ck_tids, and under GD_PATH_AUTO a later attempt may be the first to need them
    compute_build_table(c, S);
    // the table only changes when records, contigs or the path change: an identical one is not uploaded again
    // (a pageable-memory upload is a blocking staging copy, ~10 us of every step)
    if (c->d_ctgs != c->up_ctgs_dev || c->up_ctgs.size() != c->h_ctgs.size() ||
        memcmp(c->up_ctgs.data(), c->h_ctgs.data(), c->h_ctgs.size() * sizeof(gd::ContigDev)) != 0) {
        HIPCHK(c, hipMemcpyAsync(c->d_ctgs, c->h_ctgs.data(), c->h_ctgs.size() * sizeof(gd::ContigDev),
                                 hipMemcpyHostToDevice, c->stream));
        c->up_ctgs = c->h_ctgs;
        c->up_ctgs_dev = c->d_ctgs;
    }
    job.n_units = (uint32_t)S.n_units;
    if (route == GD_TK_SCATTER) {
        if (int r = ensure_dev(c, c->d_status, (size_t)c->n_tiles)) return r;
        job.tile_status = c->d_status;
        if (int r = compute_stage(c, S, GD_K_PREP)) return r;
        // the per-base array doubles as the difference array: zero it, padding included
        HIPCHK(c, hipMemsetAsync(c->d_perbase, 0, (size_t)S.base_off * sizeof(int32_t), c->stream));
        {
            int64_t work = std::max<int64_t>(job.n_tiles, std::min<int64_t>(job.n_win_total, 1 << 22));
            hipLaunchKernelGGL(gd::gd_linit_kernel, dim3((unsigned)((work + 255) / 256)), dim3(256), 0,
                               c->stream, job);
        }
        if (int r = compute_stage(c, S, GD_K_EXPAND)) return r;
        if (S.n_units > (1ull << 26) - 64)               // one wave per 64-read unit; a launch holds fewer than 2^32 work-items
            return fail(c, GD_E_RANGE, "the scatter path takes at most 2^32 records per compute");
        if (S.n_units) {
            const uint64_t groups = (S.n_units + 3) / 4;
            const unsigned grid = (unsigned)(((groups + 7) / 8) * 8);
            hipLaunchKernelGGL(gd::gd_expand_scatter_kernel, dim3(grid), dim3(256), 0, c->stream, job);
        }
        if (int r = compute_stage(c, S, GD_K_SCAN)) return r;
        hipLaunchKernelGGL(gd::gd_scan_kernel, dim3((unsigned)c->n_tiles), dim3(gd::shape::NT), 0, c->stream, job);
    } else if (route == GD_TK_SUMS_STREAM_RAW) {
        job.n_groups = (uint32_t)S.n_groups;
        if (int r = compute_stage(c, S, GD_K_PREP)) return r;
        HIPCHK(c, hipMemsetAsync(c->d_wsum, 0, (size_t)c->n_win_total * sizeof(int64_t), c->stream));
        HIPCHK(c, hipMemsetAsync(c->d_counters, 0, sizeof(gd::Counters), c->stream));
        if (int r = compute_stage(c, S, GD_K_TILE)) return r;
        if (S.n_groups)
            hipLaunchKernelGGL(gd::sums::gd_sums_stream_kernel, dim3((unsigned)((S.n_groups + 3) / 4)), dim3(256), 0,
                               c->stream, job);
    } else {
        if (int r = compute_stage(c, S, GD_K_PREP)) return r;
        launch_prep(c, job);
        c->slow_counter_clean = true;
        if (int r = compute_stage(c, S, GD_K_TILE)) return r;
        if (route == GD_TK_LONG) launch_ltile(c, job);
        else launch_tile(c, job, route);
    }
    if (int r = compute_stage(c, S, GD_K_RUNS)) return r;
    if (!route_sums_only(route)) launch_runs_order(c, job);   // (no class runs in sums-only mode: an empty stage)
    if (int r = compute_stage(c, S, kStagesEnd)) return r;
    if (c->export_buf) {                                     // (its window capacity was checked before anything was launched)
        // the last gather may still be reading this very block (a host that does not alternate two export buffers):
        // the export waits for it -- with two buffers the pointers differ and nothing waits (ADVICE round 4)
        if (c->comm && c->comm_seq > 0 && c->comm_last_send == c->export_buf)
            HIPCHK(c, hipStreamWaitEvent(c->stream, c->comm_ev[c->comm_last_ev], 0));
        const int64_t work = std::max<int64_t>(c->n_win_total, 1024);
        const unsigned grid = (unsigned)std::min<int64_t>((work + 255) / 256, 2048);
        hipLaunchKernelGGL(gd::gd_export_kernel, dim3(grid), dim3(256), 0, c->stream, c->d_wsum, c->d_wmin,
                           c->n_win_total, c->d_ordered, c->d_counters, c->export_buf,
                           c->export_max_w, c->export_cap_b, job.run_cap);
    }
    HIPCHK(c, hipGetLastError());
    // The counters and the first boundaries (a whole-genome run has a few hundred of them; more than kSpecBounds: a
    // second, exact copy below) go back to page-locked host memory through ONE small kernel that stores them over the
    // link, so that one synchronisation serves both.  Two hipMemcpyAsync did the same through the runtime's copy path,
    // whose first use behind running kernels cost the first gd_compute of a process 1.3 - 13 ms inside the enqueue
    // (measured box to box), and every later one two copy commands.
    S.spec = std::min(kSpecBounds, c->d_ordered.cap());
    hipLaunchKernelGGL(gd::gd_readback_kernel, dim3(1), dim3(256), 0, c->stream, c->d_counters, c->d_ordered, (uint32_t)S.spec,
                       c->h_counters, c->h_bounds);
    HIPCHK(c, hipGetLastError());
    return GD_OK;
}

// 0 = done, 1 = enqueue again (look-back / path / capacity), < 0 error
static int compute_complete(gd_ctx* c, ComputeState& S)
{
    const bool scatter = S.route == GD_TK_SCATTER, chunk = S.route == GD_TK_LONG;
    HIPCHK(c, hipStreamSynchronize(c->stream));

    const gd::Counters k = *c->h_counters;
    if (chunk) {
        c->stats.max_span_seen = S.chunk_span;           // over all records with ops (the filter is applied per tile)
    } else if (scatter) {
        if (k.pad1 != 0) return fail(c, GD_E_HIP, "scan look-back timed out (internal error)");
    } else {
        c->stats.max_span_seen = k.max_span > 0 ? k.max_span : 0;
        if (c->path == GD_PATH_AUTO && k.max_span > kAutoLongSpan) {
            // reads this long make the tile path re-examine too much: switch paths
            c->span_forces_long = true;
            ++S.reruns;
            return 1;
        }
        if (k.max_span >= kMaxSpan)
            return fail(c, GD_E_RANGE, "a read spans %d reference bases (tile path limit %d; use GD_PATH_CHUNK)",
                        k.max_span, kMaxSpan - 1);
        if (k.max_span > c->lookback) {
            // a kept read spans more reference than the look-back: redo with the observed maximum
            c->lookback = (k.max_span + 63) & ~63;
            ++S.reruns;
            return 1;
        }
        S.used_lookback = c->lookback;
        if (!c->lookback_pinned && k.max_span > 0) {
            // the tile kernel reports the true maximum: a look-back far above it only
            // costs re-examined reads, so the next compute uses a tighter (still verified) one
            // (max_span == 0: nothing was measured -- the streaming sums kernel has no look-back and reports none;
            // shrinking on its account cost the next tile compute a re-run)
            const int want = std::max(64, (k.max_span + 63) & ~63);
            if (want * 2 <= c->lookback) c->lookback = want;
        }
    }
    if ((size_t)k.run_cursor > c->d_ordered.cap()) {
        const size_t want = (size_t)k.run_cursor + (size_t)k.run_cursor / 8 + 1024;
        if (int r = ensure_dev(c, c->d_chunks, want)) return r;
        if (int r = ensure_dev(c, c->d_ordered, want)) return r;
        ++S.reruns;
        return 1;
    }
    // ---- ordered boundaries to the host (small) -------------------------
    c->bounds.resize(k.run_cursor);
    if (k.run_cursor && (size_t)k.run_cursor <= S.spec)
        memcpy(c->bounds.data(), c->h_bounds, (size_t)k.run_cursor * sizeof(int2));
    else if (k.run_cursor)
        HIPCHK(c, hipMemcpy(c->bounds.data(), c->d_ordered, (size_t)k.run_cursor * sizeof(int2), hipMemcpyDeviceToHost));
    return 0;
}

static int compute_publish(gd_ctx* c, ComputeState& S)
{
    for (int k = 0; k + 1 < S.n_stages; ++k)                // (the stages the enqueue opened; none without profiling)
        HIPCHK(c, hipEventElapsedTime(&c->kernel_ms[S.stage_id[k]], c->ev[k], c->ev[k + 1]));
    // slice the boundary list per contig
    {
        size_t i = 0;
        const size_t n = c->bounds.size();
        for (size_t j = 0; j < c->job_tids.size(); ++j) {
            ContigHost& h = c->contigs[c->job_tids[j]];
            h.run_beg = i;
            while (i < n && (size_t)(c->bounds[i].y >> 2) == j) ++i;
            h.run_end = i;
        }
        if (i != n) return fail(c, GD_E_HIP, "run boundaries out of order (internal error)");
    }
    c->stats.n_reads = S.n_reads;
    c->stats.n_ops = S.n_ops;
    c->stats.n_ref_bases = (uint64_t)S.bases;
    c->stats.n_windows = (uint64_t)c->n_win_total;
    c->stats.n_tiles = (uint64_t)c->n_tiles;
    c->stats.n_runs = c->bounds.size();
    c->stats.tile_positions = kTileT;
    c->stats.lookback = S.used_lookback;
    c->stats.reruns = S.reruns;
    c->stats.path = route_path(S.route);
    c->stats.n_slow_tiles = (int32_t)c->h_counters->n_slow[c->parity];
    c->stats.tile_kernel = S.route;
    // the slow list is normally one tile per contig: a small grid strides over it; data with many slow tiles
    // (deep pile-ups) gets a wider one from the next compute on
    if ((uint32_t)c->stats.n_slow_tiles > c->slow_grid * 4u) c->slow_grid = std::min<uint32_t>(2048u, (uint32_t)c->stats.n_slow_tiles);
    c->stats.n_canonical_ops = 0;
    c->stats.n_deletions = 0;
    if (S.route == GD_TK_LONG)
        for (int32_t tid : c->job_tids) c->stats.n_deletions += c->contigs[tid].n_dels;
    if (S.route == GD_TK_SCATTER) c->stats.max_span_seen = 0;   // not measured on this path
    c->computed = true;
    return GD_OK;
}

static double compute_now()
{
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

int gd_compute_launch(gd_ctx* c)
{
    if (!c) return GD_E_INVALID;
    if (c->cs.pending) return fail(c, GD_E_STATE, "a compute is already in flight: gd_compute_finish first");
    const double t0 = compute_now();
    const int r = compute_prepare(c, c->cs);
    const double t1 = compute_now();
    c->timing[0] = t1 - t0; c->timing[1] = c->timing[2] = 0; c->timing[3] = t1 - t0;
    if (r < 0) return r;
    c->cs.nothing = r == 1;
    c->alloc_in_enqueue = 0;
    if (!c->cs.nothing)
        if (int e = compute_enqueue(c, c->cs)) return e;
    c->timing[1] = compute_now() - t1 - c->alloc_in_enqueue;
    c->timing[0] += c->alloc_in_enqueue;                 // device allocations are `prepare`, wherever they happen
    c->timing[3] = c->timing[0] + c->timing[1];
    c->cs.pending = true;
    return GD_OK;
}

int gd_compute_finish(gd_ctx* c)
{
    if (!c) return GD_E_INVALID;
    if (!c->cs.pending) return fail(c, GD_E_STATE, "gd_compute_launch has not been called");
    c->cs.pending = false;
    double t0 = 0;
    if (!c->cs.nothing) {
        if (int r = set_device(c)) return r;
        t0 = compute_now();
        for (;;) {
            const int r = compute_complete(c, c->cs);
            if (r < 0) return r;
            if (r == 0) break;
            if (int e = compute_enqueue(c, c->cs)) return e;
        }
    }
    // what the results hold: the route of the LAST attempt (under GD_PATH_AUTO a re-run may have left a sums-only
    // route for the long-read one); GD_TK_NONE for a job without tiles
    c->ran_sums_only = route_sums_only(c->cs.route);
    if (c->cs.nothing) { c->computed = true; return GD_OK; }
    const int rp = compute_publish(c, c->cs);
    c->timing[2] = compute_now() - t0;
    c->timing[3] += c->timing[2];
    return rp;
}

int gd_compute(gd_ctx* c)
{
    if (int r = gd_compute_launch(c)) return r;
    return gd_compute_finish(c);
}

// Rebuilds, from the records, the long-read structures the selected contigs hold, into the device block they already
// occupy.
int gd_rebuild_derived(gd_ctx* c)
{
    if (!c) return GD_E_INVALID;
    if (int r = in_flight(c)) return r;
    if (int r = set_device(c)) return r;
    if (c->contigs.empty()) return fail(c, GD_E_STATE, "gd_set_contigs has not been called");
    const std::vector<int32_t> tids = selected_or_all(c);
    c->computed = false;
    std::vector<int32_t> raw;
    for (int32_t tid : tids) {
        ContigHost& h = c->contigs[tid];
        if (h.length <= 0) continue;
        if (h.ck_ok) { h.ck_ok = false; raw.push_back(tid); }
    }
    return ck_tids(c, raw);
}

// Drops everything derived from the records (long-read structures): the state
// right after the records arrived.
int gd_drop_derived(gd_ctx* c)
{
    if (!c) return GD_E_INVALID;
    if (int r = in_flight(c)) return r;
    if (int r = set_device(c)) return r;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (auto& h : c->contigs) drop_ck(h);
    c->computed = false;
    return GD_OK;
}
