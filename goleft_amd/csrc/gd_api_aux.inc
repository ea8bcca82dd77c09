// gd_api_aux.inc -- the callers next to the path: depthwed matrix, --stats sequence counts, multidepth
// flags and block sums (part of gd_api.hip, inside extern "C").

// Builds the matrix in the context's scratch buffer; *d_cells points at [rows][n_samples].
static int depthwed_on_device(gd_ctx* c, int n_samples, int n_ctg, const int32_t* tids, int64_t size,
                              int32_t* row_ctg, int64_t* row_start, int64_t* row_end, size_t cap_rows,
                              bool need_cap, size_t* n_rows, int64_t** d_cells)
{
    if (!c || !n_rows || n_samples < 1 || n_ctg < 1 || !tids || size < 1) return GD_E_INVALID;
    if (int r = set_device(c)) return r;
    if (!c->computed) return fail(c, GD_E_STATE, "no results: call gd_compute first");
    const int64_t W = c->params.window_size;
    const int64_t group = (size + W - 1) / W;      // depthwed.go:126: rows until span >= size
    std::vector<int64_t> off((size_t)n_samples * n_ctg), nwin(n_ctg), clen(n_ctg), row_beg(n_ctg + 1);
    int64_t rows = 0;
    for (int j = 0; j < n_ctg; ++j) {
        for (int s = 0; s < n_samples; ++s) {
            const int32_t tid = tids[(size_t)s * n_ctg + j];
            if (int r = check_result_tid(c, tid)) return r;
            const ContigHost& h = c->contigs[tid];
            if (s == 0) { clen[j] = h.length; nwin[j] = h.n_win; }
            else if (h.length != clen[j])
                return fail(c, GD_E_INVALID, "sample %d contig %d: length %lld differs from sample 0 (%lld)",
                            s, j, (long long)h.length, (long long)clen[j]);
            off[(size_t)s * n_ctg + j] = h.win_off < 0 ? 0 : h.win_off;
        }
        row_beg[j] = rows;
        rows += (nwin[j] + group - 1) / group;
    }
    row_beg[n_ctg] = rows;
    *n_rows = (size_t)rows;
    *d_cells = nullptr;
    if (rows == 0) return GD_OK;
    if (need_cap && cap_rows < (size_t)rows) return fail(c, GD_E_CAPACITY, "need room for %lld rows", (long long)rows);
    for (int j = 0; j < n_ctg; ++j)
        for (int64_t r = 0; r < row_beg[j + 1] - row_beg[j]; ++r) {
            const int64_t k = row_beg[j] + r;
            if ((size_t)k >= cap_rows) break;
            if (row_ctg) row_ctg[k] = j;
            if (row_start) row_start[k] = r * group * W;
            if (row_end) row_end[k] = std::min<int64_t>((r + 1) * group * W, clen[j]);
        }
    // small tables + the matrix live in one context-owned allocation
    const size_t n_tab = off.size() + nwin.size() + clen.size() + row_beg.size();
    const size_t n_cells = (size_t)rows * (size_t)n_samples;
    if (int r = ensure_dev(c, c->d_wed, n_tab + n_cells)) return r;
    int64_t* d = c->d_wed;
    std::vector<int64_t> tab;
    tab.reserve(n_tab);
    tab.insert(tab.end(), off.begin(), off.end());
    tab.insert(tab.end(), nwin.begin(), nwin.end());
    tab.insert(tab.end(), clen.begin(), clen.end());
    tab.insert(tab.end(), row_beg.begin(), row_beg.end());
    gd::WedJob j{};
    j.win_sum = c->d_wsum;
    j.off = d; j.nwin = d + off.size(); j.clen = j.nwin + nwin.size(); j.row_beg = j.clen + clen.size();
    j.cells = d + n_tab;
    j.n_samples = n_samples; j.n_ctg = n_ctg; j.n_rows = rows; j.W = W; j.group = group;
    HIPCHK(c, hipMemcpyAsync(d, tab.data(), n_tab * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    if ((rows + gd::WED_TILE - 1) / gd::WED_TILE > 0x7fffffffLL) return fail(c, GD_E_RANGE, "too many matrix rows");
    hipLaunchKernelGGL(gd::gd_depthwed_kernel,
                       dim3((unsigned)((rows + gd::WED_TILE - 1) / gd::WED_TILE), (unsigned)((n_samples + gd::WED_TILE - 1) / gd::WED_TILE)),
                       dim3(256), 0, c->stream, j);
    HIPCHK(c, hipStreamSynchronize(c->stream));       // `tab` must outlive the copy
    *d_cells = j.cells;
    return GD_OK;
}

int gd_depthwed(gd_ctx* c, int n_samples, int n_ctg, const int32_t* tids, int64_t size,
                int64_t* cells, int32_t* row_ctg, int64_t* row_start, int64_t* row_end,
                size_t cap_rows, size_t* n_rows)
{
    int64_t* d_cells = nullptr;
    if (n_rows && cap_rows && !cells) return GD_E_INVALID;
    if (int r = depthwed_on_device(c, n_samples, n_ctg, tids, size, row_ctg, row_start, row_end, cap_rows, true,
                                   n_rows, &d_cells))
        return r;
    if (!d_cells) return GD_OK;
    HIPCHK(c, hipMemcpy(cells, d_cells, *n_rows * (size_t)n_samples * sizeof(int64_t), hipMemcpyDeviceToHost));
    return GD_OK;
}

int gd_depthwed_device(gd_ctx* c, int n_samples, int n_ctg, const int32_t* tids, int64_t size,
                       const int64_t** d_cells, size_t* n_rows)
{
    if (int r = in_flight(c)) return r;
    if (!d_cells) return GD_E_INVALID;
    int64_t* p = nullptr;
    const int r = depthwed_on_device(c, n_samples, n_ctg, tids, size, nullptr, nullptr, nullptr, 0, false, n_rows, &p);
    *d_cells = p;
    return r;
}

int gd_seq_load(gd_ctx* c, const uint8_t* seq, int64_t len)
{
    if (!c || len < 0 || (len > 0 && !seq)) return GD_E_INVALID;
    if (len >= 0x7fffffffLL - 16) return fail(c, GD_E_RANGE, "sequence of %lld bases (contigs are < 2^31)", (long long)len);
    if (int r = set_device(c)) return r;
    const size_t padded = (((size_t)len + 3) & ~(size_t)3) + 8;
    if (int r = ensure_dev(c, c->d_seq, padded)) return r;
    if (len) HIPCHK(c, hipMemcpyAsync(c->d_seq, seq, (size_t)len, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(c->d_seq + len, 0, padded - (size_t)len, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));          // the caller's buffer is not retained
    c->seq_len = len;
    c->seq_padded = (uint32_t)padded;
    return GD_OK;
}

int gd_seq_stats_ex(gd_ctx* c, size_t n_windows, const int64_t* start, const int64_t* end, int32_t line_bases,
                    uint32_t* n_gc, uint32_t* n_cpg, uint32_t* n_masked, uint32_t* n_acgt, uint32_t* n_masked_acgt)
{
    if (!c || (n_windows && (!start || !end || !n_gc || !n_cpg || !n_masked)) || line_bases < 0) return GD_E_INVALID;
    if (int r = set_device(c)) return r;
    if (c->seq_len < 0) return fail(c, GD_E_STATE, "gd_seq_load has not been called");
    if (n_windows == 0) return GD_OK;
    if (n_windows > 0x7fffffffull * 4) return fail(c, GD_E_RANGE, "too many windows");
    // one scratch allocation: starts, ends (int64), then the five count arrays (uint32)
    const size_t bytes = n_windows * (2 * sizeof(int64_t) + 5 * sizeof(uint32_t));
    DevBuf d;
    if (int r = d.alloc(c, bytes)) return r;
    int64_t* d_s = d.as<int64_t>();
    int64_t* d_e = d_s + n_windows;
    uint32_t* d_c = reinterpret_cast<uint32_t*>(d_e + n_windows);
    gd::SeqStatsJob j{};
    j.seq = c->d_seq; j.len = c->seq_len; j.padded = c->seq_padded;
    j.win_start = d_s; j.win_end = d_e;
    j.gc = d_c; j.cpg = d_c + n_windows; j.masked = d_c + 2 * n_windows;
    j.acgt = n_acgt ? d_c + 3 * n_windows : nullptr;
    j.masked_acgt = n_masked_acgt ? d_c + 4 * n_windows : nullptr;
    j.n_win = (int64_t)n_windows;
    j.line_bases = (uint32_t)line_bases;
    HIPCHK(c, hipMemcpyAsync(d_s, start, n_windows * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_e, end, n_windows * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    if (c->profiling) (void)hipEventRecord(c->ev[0], c->stream);
    hipLaunchKernelGGL(gd::gd_seq_stats_kernel, dim3((unsigned)((n_windows + 3) / 4)), dim3(256), 0, c->stream, j);
    if (c->profiling) (void)hipEventRecord(c->ev[1], c->stream);
    HIPCHK(c, hipMemcpyAsync(n_gc, j.gc, n_windows * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(n_cpg, j.cpg, n_windows * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(n_masked, j.masked, n_windows * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    if (n_acgt) HIPCHK(c, hipMemcpyAsync(n_acgt, j.acgt, n_windows * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    if (n_masked_acgt) HIPCHK(c, hipMemcpyAsync(n_masked_acgt, j.masked_acgt, n_windows * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->profiling) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, c->ev[0], c->ev[1]) == hipSuccess) c->kernel_ms[GD_K_SEQSTATS] = ms;
    }
    return GD_OK;
}

int gd_seq_stats(gd_ctx* c, size_t n_windows, const int64_t* start, const int64_t* end,
                 uint32_t* n_gc, uint32_t* n_cpg, uint32_t* n_masked)
{
    return gd_seq_stats_ex(c, n_windows, start, end, 0, n_gc, n_cpg, n_masked, nullptr, nullptr);
}

// the per-base vectors of n_samples equally long contigs of the last gd_compute
static int md_sample_ptrs(gd_ctx* c, int n_samples, const int32_t* tids, std::vector<const int32_t*>* ptrs,
                          int64_t* len)
{
    if (!c->computed) return fail(c, GD_E_STATE, "no results: call gd_compute first");
    if (!c->d_perbase) return fail(c, GD_E_STATE, "the per-base vector was not kept (gd_set_outputs)");
    ptrs->resize((size_t)n_samples);
    for (int s = 0; s < n_samples; ++s) {
        if (int r = check_result_tid(c, tids[s])) return r;
        const ContigHost& h = c->contigs[tids[s]];
        if (s == 0) *len = h.length;
        else if (h.length != *len)
            return fail(c, GD_E_INVALID, "sample %d: contig length %lld differs from sample 0 (%lld)", s,
                        (long long)h.length, (long long)*len);
        (*ptrs)[(size_t)s] = c->d_perbase + h.base_off;
    }
    return GD_OK;
}

int gd_md_flags(gd_ctx* c, int n_samples, const int32_t* tids, int32_t min_cov, int32_t min_samples,
                uint32_t* any_bits, uint32_t* suf_bits, size_t n_words)
{
    if (int r = in_flight(c)) return r;
    if (!c || n_samples < 1 || !tids) return GD_E_INVALID;
    if (int r = set_device(c)) return r;
    std::vector<const int32_t*> ptrs;
    int64_t len = 0;
    if (int r = md_sample_ptrs(c, n_samples, tids, &ptrs, &len)) return r;
    const size_t need = (size_t)((len + 31) / 32);
    if (n_words < need || ((!any_bits || !suf_bits) && need))
        return fail(c, GD_E_CAPACITY, "need room for %zu bitmap words", need);
    c->md_len = -1;
    if (need == 0) { c->md_len = 0; c->md_tids.assign(tids, tids + n_samples); return GD_OK; }
    if (int r = ensure_dev(c, c->d_md_bits, 2 * need)) return r;
    DevBuf d_ptrs;
    if (int r = d_ptrs.alloc(c, ptrs.size() * sizeof(ptrs[0]))) return r;
    gd::MdFlagsJob j{};
    j.depth = d_ptrs.as<const int32_t*>(); j.n_samples = n_samples; j.len = len; j.min_cov = min_cov; j.min_samples = min_samples;
    j.any_bits = c->d_md_bits; j.suf_bits = c->d_md_bits + need;
    HIPCHK(c, hipMemcpyAsync(d_ptrs.get(), ptrs.data(), ptrs.size() * sizeof(ptrs[0]), hipMemcpyHostToDevice, c->stream));
    if (c->profiling) (void)hipEventRecord(c->ev[0], c->stream);
    hipLaunchKernelGGL(gd::gd_md_flags_kernel, dim3((unsigned)((len + 255) / 256)), dim3(256), 0, c->stream, j);
    if (c->profiling) (void)hipEventRecord(c->ev[1], c->stream);
    HIPCHK(c, hipMemcpyAsync(any_bits, j.any_bits, need * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(suf_bits, j.suf_bits, need * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->profiling) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, c->ev[0], c->ev[1]) == hipSuccess) c->kernel_ms[GD_K_MDFLAGS] = ms;
    }
    c->md_len = len;
    c->md_tids.assign(tids, tids + n_samples);
    return GD_OK;
}

// ---- samples in groups: gd_md_begin, gd_md_accumulate per group, gd_md_finish ------------------
int gd_md_begin(gd_ctx* c, int64_t len)
{
    if (!c || len < 0 || len >= 0x7fffffffLL) return GD_E_INVALID;
    if (int r = set_device(c)) return r;
    const size_t need = (size_t)((len + 31) / 32);
    c->md_len = -1;
    c->md_tids.clear();
    c->md_acc_len = -1;
    if (int r = ensure_dev(c, c->d_md_bits, 2 * std::max<size_t>(need, 1))) return r;
    if (int r = ensure_dev(c, c->d_md_cnt, (size_t)std::max<int64_t>(len, 1))) return r;
    HIPCHK(c, hipMemsetAsync(c->d_md_bits, 0, 2 * std::max<size_t>(need, 1) * sizeof(uint32_t), c->stream));
    HIPCHK(c, hipMemsetAsync(c->d_md_cnt, 0, (size_t)std::max<int64_t>(len, 1) * sizeof(uint16_t), c->stream));
    c->md_acc_len = len;
    c->md_acc_samples = 0;
    return GD_OK;
}

int gd_md_accumulate(gd_ctx* c, int n_samples, const int32_t* tids, int32_t min_cov)
{
    if (int r = in_flight(c)) return r;
    if (!c || n_samples < 1 || !tids) return GD_E_INVALID;
    if (int r = set_device(c)) return r;
    if (c->md_acc_len < 0) return fail(c, GD_E_STATE, "gd_md_begin has not been called");
    std::vector<const int32_t*> ptrs;
    int64_t len = 0;
    if (int r = md_sample_ptrs(c, n_samples, tids, &ptrs, &len)) return r;
    if (len != c->md_acc_len) return fail(c, GD_E_INVALID, "contig length %lld differs from gd_md_begin's %lld", (long long)len, (long long)c->md_acc_len);
    if (c->md_acc_samples + (int64_t)n_samples > 65535) return fail(c, GD_E_RANGE, "more than 65535 samples");
    c->md_acc_samples += n_samples;
    if (len == 0) return GD_OK;
    DevBuf d_ptrs;
    if (int r = d_ptrs.alloc(c, ptrs.size() * sizeof(ptrs[0]))) return r;
    gd::MdAccJob j{};
    j.depth = d_ptrs.as<const int32_t*>(); j.n_samples = n_samples; j.len = len; j.min_cov = min_cov;
    j.cnt = c->d_md_cnt; j.any_bits = c->d_md_bits;
    HIPCHK(c, hipMemcpyAsync(d_ptrs.get(), ptrs.data(), ptrs.size() * sizeof(ptrs[0]), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(gd::gd_md_acc_kernel, dim3((unsigned)((len + 255) / 256)), dim3(256), 0, c->stream, j);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return GD_OK;
}

int gd_md_finish(gd_ctx* c, int32_t min_samples, uint32_t* any_bits, uint32_t* suf_bits, size_t n_words)
{
    if (!c) return GD_E_INVALID;
    if (int r = set_device(c)) return r;
    if (c->md_acc_len < 0) return fail(c, GD_E_STATE, "gd_md_begin has not been called");
    const int64_t len = c->md_acc_len;
    const size_t need = (size_t)((len + 31) / 32);
    if ((any_bits || suf_bits) && n_words < need) return fail(c, GD_E_CAPACITY, "need room for %zu bitmap words", need);
    if (len) {
        hipLaunchKernelGGL(gd::gd_md_finish_kernel, dim3((unsigned)((len + 255) / 256)), dim3(256), 0, c->stream,
                           c->d_md_cnt, len, min_samples, c->d_md_bits + need);
        if (any_bits) HIPCHK(c, hipMemcpyAsync(any_bits, c->d_md_bits, need * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        if (suf_bits) HIPCHK(c, hipMemcpyAsync(suf_bits, c->d_md_bits + need, need * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    c->md_len = len;
    c->md_tids.clear();                                   // the samples are not resident as a set: gd_md_sums_group
    return GD_OK;
}

int gd_md_load_flags(gd_ctx* c, const uint32_t* any_bits, const uint32_t* suf_bits, int64_t len)
{
    if (!c || len < 0 || len >= 0x7fffffffLL || (len && (!any_bits || !suf_bits))) return GD_E_INVALID;
    if (int r = set_device(c)) return r;
    const size_t need = (size_t)((len + 31) / 32);
    c->md_len = -1;
    c->md_tids.clear();
    if (int r = ensure_dev(c, c->d_md_bits, 2 * std::max<size_t>(need, 1))) return r;
    if (need) {
        HIPCHK(c, hipMemcpyAsync(c->d_md_bits, any_bits, need * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->d_md_bits + need, suf_bits, need * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    c->md_len = len;
    return GD_OK;
}

// ---- the block finder (gd_multidepth.hpp B1..B5) -------------------------------------------------
int gd_md_blocks(gd_ctx* c, int64_t chunk, int32_t max_skip, int32_t min_size, int32_t window,
                 int64_t* starts, int64_t* ends, size_t cap, size_t* n_blocks)
{
    if (!c || !n_blocks || chunk < 1 || max_skip < 0) return GD_E_INVALID;
    *n_blocks = 0;
    if (int r = set_device(c)) return r;
    if (c->md_len < 0) return fail(c, GD_E_STATE, "no bitmaps: call gd_md_flags, gd_md_finish or gd_md_load_flags first");
    const int64_t len = c->md_len;
    if (len == 0) return GD_OK;
    const int64_t nw = (len + 31) / 32, n_chunks = (len + chunk - 1) / chunk;
    // every chunk's stream is walked by one thread (the reference uses 5 Mb / 1 Mb chunks: at most ~2 000 per contig)
    if (n_chunks > (1 << 20)) return fail(c, GD_E_RANGE, "%lld chunks of %lld positions (at most 2^20)", (long long)n_chunks, (long long)chunk);
    // scratch: everything but the run / pair / block arrays, whose sizes are only known after the scans
    DevList sc;
    gd::MdBlkJob j{};
    j.any_bits = c->d_md_bits; j.suf_bits = c->d_md_bits + nw;
    j.len = len; j.nw = nw; j.chunk = chunk; j.max_skip = max_skip; j.min_size = min_size; j.window = window;
    j.n_chunks = n_chunks;
    if (int r = sc.alloc(c, &j.rs, (size_t)nw)) return r;
    if (int r = sc.alloc(c, &j.re, (size_t)nw)) return r;
    if (int r = sc.alloc(c, &j.ps, (size_t)nw + 1)) return r;
    if (int r = sc.alloc(c, &j.prs, (size_t)nw + 1)) return r;
    if (int r = sc.alloc(c, &j.pre, (size_t)nw + 1)) return r;
    if (int r = sc.alloc(c, &j.z0, (size_t)n_chunks)) return r;
    if (int r = sc.alloc(c, &j.E, (size_t)n_chunks)) return r;
    if (int r = sc.alloc(c, &j.pa, (size_t)n_chunks)) return r;
    if (int r = sc.alloc(c, &j.k_lo, (size_t)n_chunks)) return r;
    if (int r = sc.alloc(c, &j.pair_off, (size_t)n_chunks + 1)) return r;
    const unsigned wgrid = (unsigned)((nw + 255) / 256);
    hipLaunchKernelGGL(gd::gd_md_runs_kernel, dim3(wgrid), dim3(256), 0, c->stream, j);
    if (int r = launch_scan(c, j.ps, (uint32_t)nw)) return r;
    if (int r = launch_scan(c, j.prs, (uint32_t)nw)) return r;
    if (int r = launch_scan(c, j.pre, (uint32_t)nw)) return r;
    uint32_t n_runs = 0;
    HIPCHK(c, hipMemcpyAsync(&n_runs, j.prs + nw, sizeof n_runs, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (n_runs == 0) return GD_OK;
    if (int r = sc.alloc(c, &j.starts, (size_t)n_runs)) return r;
    if (int r = sc.alloc(c, &j.ends, (size_t)n_runs)) return r;
    hipLaunchKernelGGL(gd::gd_md_compact_kernel, dim3(wgrid), dim3(256), 0, c->stream, j);
    hipLaunchKernelGGL(gd::gd_md_chunks_kernel, dim3(1), dim3(256), 0, c->stream, j);
    uint32_t n_pairs = 0;
    HIPCHK(c, hipMemcpyAsync(&n_pairs, j.pair_off + n_chunks, sizeof n_pairs, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (n_pairs == 0) return GD_OK;
    if (int r = sc.alloc(c, &j.nblk, (size_t)n_pairs + 1)) return r;
    HIPCHK(c, hipMemsetAsync(j.nblk + n_pairs, 0, 4, c->stream));
    const unsigned pgrid = (unsigned)((n_pairs + 255u) / 256u);
    hipLaunchKernelGGL(gd::gd_md_count_kernel, dim3(pgrid), dim3(256), 0, c->stream, j, n_pairs);
    if (int r = launch_scan(c, j.nblk, n_pairs)) return r;
    uint32_t nb = 0;
    HIPCHK(c, hipMemcpyAsync(&nb, j.nblk + n_pairs, sizeof nb, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *n_blocks = nb;
    if (nb == 0) return GD_OK;
    if ((size_t)nb > cap || !starts || !ends) return fail(c, GD_E_CAPACITY, "%u blocks, room for %zu", nb, cap);
    if (int r = sc.alloc(c, &j.bstart, (size_t)nb)) return r;
    if (int r = sc.alloc(c, &j.bend, (size_t)nb)) return r;
    hipLaunchKernelGGL(gd::gd_md_blocks_kernel, dim3(pgrid), dim3(256), 0, c->stream, j, n_pairs);
    HIPCHK(c, hipMemcpyAsync(starts, j.bstart, (size_t)nb * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(ends, j.bend, (size_t)nb * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return GD_OK;
}

static int md_sums_impl(gd_ctx* c, int n_samples, const int32_t* tids, size_t n_blocks, const int64_t* start,
                        const int64_t* end, double* sums);

int gd_md_sums(gd_ctx* c, size_t n_blocks, const int64_t* start, const int64_t* end, double* sums)
{
    if (!c || (n_blocks && (!start || !end || !sums))) return GD_E_INVALID;
    if (int r = set_device(c)) return r;
    if (c->md_len < 0 || c->md_tids.empty()) return fail(c, GD_E_STATE, "gd_md_flags has not been called");
    return md_sums_impl(c, (int)c->md_tids.size(), c->md_tids.data(), n_blocks, start, end, sums);
}

int gd_md_sums_group(gd_ctx* c, int n_samples, const int32_t* tids, size_t n_blocks, const int64_t* start,
                     const int64_t* end, double* sums)
{
    if (!c || n_samples < 1 || !tids || (n_blocks && (!start || !end || !sums))) return GD_E_INVALID;
    if (int r = set_device(c)) return r;
    if (c->md_len < 0) return fail(c, GD_E_STATE, "no bitmaps: call gd_md_flags or gd_md_finish first");
    return md_sums_impl(c, n_samples, tids, n_blocks, start, end, sums);
}

static int md_sums_impl(gd_ctx* c, int n_samples, const int32_t* tids, size_t n_blocks, const int64_t* start,
                        const int64_t* end, double* sums)
{
    if (n_blocks == 0) return GD_OK;
    std::vector<const int32_t*> ptrs;
    int64_t len = 0;
    if (int r = md_sample_ptrs(c, n_samples, tids, &ptrs, &len)) return r;
    if (len != c->md_len) return fail(c, GD_E_STATE, "results changed since the bitmaps were made");
    for (size_t b = 0; b < n_blocks; ++b)
        if (start[b] < 0 || end[b] < start[b] || end[b] > len)
            return fail(c, GD_E_RANGE, "block %zu [%lld, %lld) outside the contig", b, (long long)start[b], (long long)end[b]);
    const size_t n_cells = n_blocks * (size_t)n_samples;
    const size_t bytes = ptrs.size() * sizeof(ptrs[0]) + 2 * n_blocks * sizeof(int64_t) + n_cells * sizeof(double);
    DevBuf d;
    if (int r = d.alloc(c, bytes)) return r;
    const int32_t** d_ptrs = d.as<const int32_t*>();
    int64_t* d_s = reinterpret_cast<int64_t*>(d.as<uint8_t>() + ptrs.size() * sizeof(ptrs[0]));
    int64_t* d_e = d_s + n_blocks;
    double* d_sums = reinterpret_cast<double*>(d_e + n_blocks);
    gd::MdSumsJob j{};
    j.depth = d_ptrs; j.suf_bits = c->d_md_bits + (size_t)((len + 31) / 32);
    j.start = d_s; j.end = d_e; j.sums = d_sums; j.n_blocks = (int64_t)n_blocks; j.n_samples = n_samples;
    HIPCHK(c, hipMemcpyAsync(d_ptrs, ptrs.data(), ptrs.size() * sizeof(ptrs[0]), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_s, start, n_blocks * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_e, end, n_blocks * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(gd::gd_md_sums_kernel, dim3((unsigned)((n_cells + 63) / 64)), dim3(64), 0, c->stream, j);
    HIPCHK(c, hipMemcpyAsync(sums, d_sums, n_cells * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return GD_OK;
}
