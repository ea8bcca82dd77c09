// gd_api_results.inc -- results of the last gd_compute to the host: per-base, windows, coverage-class
// runs, and the --bed mode region reductions (part of gd_api.hip, inside extern "C").

static int check_result_tid(gd_ctx* c, int32_t tid)
{
    if (!c->computed) return fail(c, GD_E_STATE, "no results: call gd_compute first");
    if (tid < 0 || (size_t)tid >= c->contigs.size()) return fail(c, GD_E_RANGE, "tid %d out of range", tid);
    if (c->contigs[tid].length > 0 && c->contigs[tid].base_off < 0)
        return fail(c, GD_E_RANGE, "contig %d was not selected in the last gd_compute", tid);
    return GD_OK;
}

int gd_perbase(gd_ctx* c, int32_t tid, int64_t start, int64_t end, int32_t* out)
{
    if (!c || !out) return GD_E_INVALID;
    if (int r = set_device(c)) return r;
    if (int r = check_result_tid(c, tid)) return r;
    const ContigHost& h = c->contigs[tid];
    if (start < 0 || end < start || end > h.length) return fail(c, GD_E_RANGE, "region [%lld,%lld) outside contig of length %lld", (long long)start, (long long)end, (long long)h.length);
    if (end == start) return GD_OK;
    if (!c->d_perbase) return fail(c, GD_E_STATE, "the per-base vector was not kept (gd_set_outputs)");
    HIPCHK(c, hipMemcpy(out, c->d_perbase + h.base_off + start, (size_t)(end - start) * sizeof(int32_t), hipMemcpyDeviceToHost));
    return GD_OK;
}

int gd_windows(gd_ctx* c, int32_t tid, int64_t* sums, int32_t* mins, size_t cap, size_t* n)
{
    if (!c || !n) return GD_E_INVALID;
    if (int r = set_device(c)) return r;
    if (int r = check_result_tid(c, tid)) return r;
    const ContigHost& h = c->contigs[tid];
    *n = (size_t)h.n_win;
    if (h.n_win == 0) return GD_OK;
    if (cap < (size_t)h.n_win || !sums) return fail(c, GD_E_CAPACITY, "need room for %lld windows", (long long)h.n_win);
    if (mins && c->ran_sums_only) return fail(c, GD_E_STATE, "window minima were not produced (GD_OUT_SUMS_ONLY)");
    HIPCHK(c, hipMemcpy(sums, c->d_wsum + h.win_off, (size_t)h.n_win * sizeof(int64_t), hipMemcpyDeviceToHost));
    if (mins)
        HIPCHK(c, hipMemcpy(mins, c->d_wmin + h.win_off, (size_t)h.n_win * sizeof(int32_t), hipMemcpyDeviceToHost));
    return GD_OK;
}

int gd_callable(gd_ctx* c, int32_t tid, gd_run* out, size_t cap, size_t* n)
{
    if (!c || !n) return GD_E_INVALID;
    if (int r = check_result_tid(c, tid)) return r;
    if (c->ran_sums_only) return fail(c, GD_E_STATE, "coverage-class runs were not produced (GD_OUT_SUMS_ONLY)");
    const ContigHost& h = c->contigs[tid];
    const size_t k = h.run_end - h.run_beg;
    *n = k;
    if (k == 0) return GD_OK;
    if (cap < k || !out) return fail(c, GD_E_CAPACITY, "need room for %zu runs", k);
    for (size_t i = 0; i < k; ++i) {
        const int2 b = c->bounds[h.run_beg + i];
        out[i].start = b.x;
        out[i].cls = b.y & 3;
        out[i].end = (i + 1 < k) ? c->bounds[h.run_beg + i + 1].x : (int32_t)h.length;
    }
    return GD_OK;
}

int gd_region_windows(gd_ctx* c, int32_t tid, int64_t start, int64_t end, int64_t* sums,
                      int32_t* mins, size_t cap, size_t* n)
{
    if (!c || !n) return GD_E_INVALID;
    if (int r = set_device(c)) return r;
    if (int r = check_result_tid(c, tid)) return r;
    if (start < 0 || end < start) return fail(c, GD_E_RANGE, "bad region");
    const ContigHost& h = c->contigs[tid];
    const int64_t W = c->params.window_size;
    if (end == start) { *n = 0; return GD_OK; }
    const int64_t first = start / W, last = (end - 1) / W;
    const size_t k = (size_t)(last - first + 1);
    *n = k;
    if (cap < k || !sums) return fail(c, GD_E_CAPACITY, "need room for %zu windows", k);
    if (h.length <= 0) { for (size_t i = 0; i < k; ++i) { sums[i] = 0; if (mins) mins[i] = 0; } return GD_OK; }
    if (!c->d_perbase) return fail(c, GD_E_STATE, "the per-base vector was not kept (gd_set_outputs)");
    DevBuf d_s, d_m;
    if (int r = d_s.alloc(c, k * sizeof(int64_t))) return r;
    if (int r = d_m.alloc(c, k * sizeof(int32_t))) return r;
    hipLaunchKernelGGL(gd::gd_region_windows_kernel, dim3((unsigned)k), dim3(256), 0, c->stream,
                       c->d_perbase + h.base_off, h.length, start, end, (int32_t)W, first, d_s.as<int64_t>(), d_m.as<int32_t>());
    HIPCHK(c, hipMemcpyAsync(sums, d_s.get(), k * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    if (mins) HIPCHK(c, hipMemcpyAsync(mins, d_m.get(), k * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return GD_OK;
}

int gd_region_callable(gd_ctx* c, int32_t tid, int64_t start, int64_t end, gd_run* out, size_t cap, size_t* n)
{
    if (!c || !n) return GD_E_INVALID;
    if (int r = set_device(c)) return r;
    if (int r = check_result_tid(c, tid)) return r;
    if (start < 0 || end < start || end > 0x7fffffffLL) return fail(c, GD_E_RANGE, "bad region");
    const ContigHost& h = c->contigs[tid];
    if (end == start) { *n = 0; return GD_OK; }
    if (h.length <= 0) {
        *n = 1;
        if (cap < 1 || !out) return fail(c, GD_E_CAPACITY, "need room for 1 run");
        out[0].start = (int32_t)start; out[0].end = (int32_t)end; out[0].cls = GD_NO_COVERAGE;
        return GD_OK;
    }
    if (!c->d_perbase) return fail(c, GD_E_STATE, "the per-base vector was not kept (gd_set_outputs)");
    size_t bcap = std::max<size_t>(cap, 1024);
    for (;;) {
        DevBuf d_b;                              // (a round that found too little room gives its buffer back before the next)
        if (int r = d_b.alloc(c, bcap * sizeof(int2))) return r;
        (void)hipMemsetAsync(c->d_region_cursor, 0, sizeof(uint32_t), c->stream);
        int64_t len = end - start;
        unsigned blocks = (unsigned)std::min<int64_t>((len + 255) / 256, 4096);
        hipLaunchKernelGGL(gd::gd_region_bounds_kernel, dim3(blocks), dim3(256), 0, c->stream,
                           c->d_perbase + h.base_off, h.length, start, end, c->params.min_cov,
                           c->params.max_mean_depth, d_b.as<int2>(), (uint32_t)std::min<size_t>(bcap, 0xffffffffu),
                           c->d_region_cursor);
        uint32_t cnt = 0;
        HIPCHK(c, hipMemcpyAsync(&cnt, c->d_region_cursor, sizeof cnt, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (cnt > bcap) { bcap = cnt; continue; }
        std::vector<int2> b(cnt);
        if (cnt) HIPCHK(c, hipMemcpy(b.data(), d_b.get(), cnt * sizeof(int2), hipMemcpyDeviceToHost));
        std::sort(b.begin(), b.end(), [](const int2& a, const int2& z) { return a.x < z.x; });
        *n = cnt;
        if (cap < cnt || !out) return fail(c, GD_E_CAPACITY, "need room for %u runs", cnt);
        for (uint32_t i = 0; i < cnt; ++i) {
            out[i].start = b[i].x;
            out[i].cls = b[i].y & 3;
            out[i].end = (i + 1 < cnt) ? b[i + 1].x : (int32_t)end;
        }
        return GD_OK;
    }
}

// Many regions at once: what a --bed file with 10^5 rows needs (one launch per reduction instead of
// three launches, six allocations and three synchronisations per row).
int gd_regions(gd_ctx* c, size_t n_regions, const int32_t* tid, const int64_t* start, const int64_t* end,
               int64_t* sums, int32_t* mins, size_t cap_windows, size_t* win_off,
               gd_run* runs, size_t cap_runs, size_t* run_off)
{
    if (!c || !win_off || !run_off || (n_regions && (!tid || !start || !end))) return GD_E_INVALID;
    if (int r = set_device(c)) return r;
    const int64_t W = c->params.window_size;
    // ---- layout: windows of every region, regions that need the device ----------------------
    std::vector<gd::RegionTab> tab;
    std::vector<uint32_t> dev_region;                     // batch index of every device region
    std::vector<uint32_t> win_region, chunk_region;
    size_t nw = 0;
    for (size_t r = 0; r < n_regions; ++r) {
        if (int rc = check_result_tid(c, tid[r])) return rc;
        if (start[r] < 0 || end[r] < start[r] || end[r] > 0x7fffffffLL)
            return fail(c, GD_E_RANGE, "region %zu: bad coordinates", r);
        win_off[r] = nw;
        if (end[r] == start[r]) continue;
        const size_t k = (size_t)((end[r] - 1) / W - start[r] / W + 1);
        const ContigHost& h = c->contigs[tid[r]];
        if (h.length > 0) {
            if (!c->d_perbase) return fail(c, GD_E_STATE, "the per-base vector was not kept (gd_set_outputs)");
            if (nw + k > 0xfffffff0ull) return fail(c, GD_E_RANGE, "too many windows in one batch");
            gd::RegionTab t{};
            t.depth = c->d_perbase + h.base_off;
            t.clen = h.length; t.start = start[r]; t.end = end[r]; t.first_win = start[r] / W;
            t.win_off = (uint32_t)win_region.size();
            t.chunk_off = (uint32_t)chunk_region.size();
            const uint32_t ti = (uint32_t)tab.size();
            win_region.insert(win_region.end(), k, ti);
            const size_t nch = (size_t)((end[r] - start[r] + gd::REGION_CHUNK - 1) / gd::REGION_CHUNK);
            if (chunk_region.size() + nch > 0x7ffffff0ull) return fail(c, GD_E_RANGE, "too many positions in one batch");
            chunk_region.insert(chunk_region.end(), nch, ti);
            tab.push_back(t);
            dev_region.push_back((uint32_t)r);
        }
        nw += k;
    }
    win_off[n_regions] = nw;
    if (nw > cap_windows || (nw && !sums)) {
        for (size_t r = 0; r <= n_regions; ++r) run_off[r] = 0;
        return fail(c, GD_E_CAPACITY, "need room for %zu windows", nw);
    }
    for (size_t i = 0; i < nw; ++i) { sums[i] = 0; if (mins) mins[i] = 0; }      // zero-length contigs stay 0

    // ---- device part -------------------------------------------------------------------------
    std::vector<int4> b;
    if (!tab.empty()) {
        const size_t n_dw = win_region.size(), n_ch = chunk_region.size();
        size_t bcap = std::max<size_t>(tab.size() * 4 + 1024, 1u << 16);
        for (;;) {
            const size_t o_tab = 0, o_wr = o_tab + tab.size() * sizeof(gd::RegionTab);
            const size_t o_cr = o_wr + ((n_dw * 4 + 15) & ~(size_t)15), o_s = o_cr + ((n_ch * 4 + 15) & ~(size_t)15);
            const size_t o_m = o_s + n_dw * 8, o_b = (o_m + n_dw * 4 + 15) & ~(size_t)15, o_c = o_b + bcap * sizeof(int4);
            DevBuf d;
            if (int r = d.alloc(c, o_c + 16)) return r;
            uint8_t* base = d.as<uint8_t>();
            gd::RegionTab* d_tab = reinterpret_cast<gd::RegionTab*>(base + o_tab);
            uint32_t* d_wr = reinterpret_cast<uint32_t*>(base + o_wr);
            uint32_t* d_cr = reinterpret_cast<uint32_t*>(base + o_cr);
            int64_t* d_s = reinterpret_cast<int64_t*>(base + o_s);
            int32_t* d_m = reinterpret_cast<int32_t*>(base + o_m);
            int4* d_b = reinterpret_cast<int4*>(base + o_b);
            uint32_t* d_cur = reinterpret_cast<uint32_t*>(base + o_c);
            HIPCHK(c, hipMemcpyAsync(d_tab, tab.data(), tab.size() * sizeof(gd::RegionTab), hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipMemcpyAsync(d_wr, win_region.data(), n_dw * 4, hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipMemcpyAsync(d_cr, chunk_region.data(), n_ch * 4, hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipMemsetAsync(d_cur, 0, sizeof(uint32_t), c->stream));
            hipLaunchKernelGGL(gd::gd_regions_windows_kernel, dim3((unsigned)n_dw), dim3(256), 0, c->stream,
                               d_tab, d_wr, (int32_t)W, d_s, d_m);
            hipLaunchKernelGGL(gd::gd_regions_bounds_kernel, dim3((unsigned)n_ch), dim3(256), 0, c->stream,
                               d_tab, d_cr, c->params.min_cov, c->params.max_mean_depth, d_b,
                               (uint32_t)std::min<size_t>(bcap, 0xffffffffu), d_cur);
            uint32_t cnt = 0;
            std::vector<int64_t> hs(n_dw);
            std::vector<int32_t> hm(n_dw);
            HIPCHK(c, hipMemcpyAsync(&cnt, d_cur, sizeof cnt, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipMemcpyAsync(hs.data(), d_s, n_dw * 8, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipMemcpyAsync(hm.data(), d_m, n_dw * 4, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            HIPCHK(c, hipGetLastError());
            if (cnt > bcap) { bcap = (size_t)cnt + 1024; continue; }      // more boundaries than guessed: once more
            b.resize(cnt);
            if (cnt) HIPCHK(c, hipMemcpy(b.data(), d_b, (size_t)cnt * sizeof(int4), hipMemcpyDeviceToHost));
            for (size_t i = 0; i < tab.size(); ++i) {                     // device windows to their batch slots
                const size_t r = dev_region[i], k = win_off[r + 1] - win_off[r];
                for (size_t j = 0; j < k; ++j) {
                    sums[win_off[r] + j] = hs[tab[i].win_off + j];
                    if (mins) mins[win_off[r] + j] = hm[tab[i].win_off + j];
                }
            }
            break;
        }
        std::sort(b.begin(), b.end(), [](const int4& a, const int4& z) { return a.z != z.z ? a.z < z.z : a.x < z.x; });
    }
    // ---- runs per region -----------------------------------------------------------------------
    size_t nr = 0, bi = 0, di = 0;
    for (size_t r = 0; r < n_regions; ++r) {
        run_off[r] = nr;
        if (end[r] == start[r]) continue;
        if (di < dev_region.size() && dev_region[di] == r) {
            const size_t b0 = bi;
            while (bi < b.size() && (size_t)b[bi].z == di) ++bi;
            for (size_t i = b0; i < bi; ++i, ++nr)
                if (nr < cap_runs && runs) {
                    runs[nr].start = b[i].x;
                    runs[nr].cls = b[i].y & 3;
                    runs[nr].end = i + 1 < bi ? b[i + 1].x : (int32_t)end[r];
                }
            ++di;
        } else {                                                          // a contig of length 0
            if (nr < cap_runs && runs) { runs[nr].start = (int32_t)start[r]; runs[nr].end = (int32_t)end[r]; runs[nr].cls = GD_NO_COVERAGE; }
            ++nr;
        }
    }
    run_off[n_regions] = nr;
    if (nr > cap_runs || (nr && !runs)) return fail(c, GD_E_CAPACITY, "need room for %zu runs", nr);
    return GD_OK;
}

int gd_device_perbase(gd_ctx* c, int32_t tid, const int32_t** dptr, int64_t* len)
{
    if (!c || !dptr) return GD_E_INVALID;
    if (int r = check_result_tid(c, tid)) return r;
    const ContigHost& h = c->contigs[tid];
    if (!c->d_perbase) return fail(c, GD_E_STATE, "the per-base vector was not kept (gd_set_outputs)");
    *dptr = h.length > 0 ? c->d_perbase + h.base_off : nullptr;
    if (len) *len = h.length;
    return GD_OK;
}

int gd_device_windows(gd_ctx* c, const int64_t** d_sums, const int32_t** d_mins, size_t* n_total)
{
    if (!c) return GD_E_INVALID;
    if (!c->computed) return fail(c, GD_E_STATE, "no results: call gd_compute first");
    if (d_sums) *d_sums = c->d_wsum;
    if (d_mins) *d_mins = c->d_wmin;
    if (n_total) *n_total = (size_t)c->n_win_total;
    return GD_OK;
}

int gd_window_offset(gd_ctx* c, int32_t tid, size_t* off, size_t* n)
{
    if (!c) return GD_E_INVALID;
    if (int r = check_result_tid(c, tid)) return r;
    const ContigHost& h = c->contigs[tid];
    if (off) *off = h.win_off < 0 ? 0 : (size_t)h.win_off;
    if (n) *n = (size_t)h.n_win;
    return GD_OK;
}

int gd_device_runs(gd_ctx* c, const int32_t** d_bounds, size_t* n_bounds)
{
    if (!c) return GD_E_INVALID;
    if (!c->computed) return fail(c, GD_E_STATE, "no results: call gd_compute first");
    if (d_bounds) *d_bounds = c->d_ordered.as<const int32_t>();
    if (n_bounds) *n_bounds = c->bounds.size();
    return GD_OK;
}

int gd_set_export(gd_ctx* c, void* device_buf, int64_t max_windows, int64_t cap_bounds)
{
    if (!c || max_windows < 0 || cap_bounds < 0) return GD_E_INVALID;
    c->export_buf = static_cast<int64_t*>(device_buf);
    c->export_max_w = max_windows;
    c->export_cap_b = cap_bounds;
    return GD_OK;
}

int gd_wait_event(gd_ctx* c, void* ev)
{
    if (!c || !ev) return GD_E_INVALID;
    if (int r = set_device(c)) return r;
    HIPCHK(c, hipStreamWaitEvent(c->stream, static_cast<hipEvent_t>(ev), 0));
    return GD_OK;
}
