// gd_api_dist.inc -- the kept per-base vector reduced along the depth axis: gd_depth_hist (a histogram with sum, minimum and
// maximum over a region list) and gd_region_bins (per region, its positions in each depth bin) (part of gd_api.hip, inside
// extern "C"; DESIGN.md section 3.22).  The kernels are gd_depth_hist.hpp's, on the context's stream.  Everything is checked
// before anything is allocated or launched; what is kept between calls is one device block (the region table, the chunk
// table and the counts: grow-only, freed with the context) and the timings.

// The checks both entries share and make first, in gd_perbase_runs' order: a compute, every tid, every region's coordinates.
static int dist_check(gd_ctx* c, size_t n_regions, const int32_t* tid, const int64_t* start, const int64_t* end)
{
    if (!c->computed) return fail(c, GD_E_STATE, "no results: call gd_compute first");
    for (size_t r = 0; r < n_regions; ++r) {
        if (int rc = check_result_tid(c, tid[r])) return rc;
        const ContigHost& h = c->contigs[tid[r]];
        if (start[r] < 0 || end[r] < start[r] || end[r] > h.length)
            return fail(c, GD_E_RANGE, "region %zu [%lld,%lld) outside contig of length %lld", r, (long long)start[r], (long long)end[r], (long long)h.length);
    }
    return GD_OK;
}

// Their last check, and the tables: an entry per region that holds a position and per chunk of it.
static int dist_tables(gd_ctx* c, const char* what, size_t n_regions, const int32_t* tid, const int64_t* start, const int64_t* end,
                       std::vector<gd::DhRegion>* tab, std::vector<uint32_t>* chunk_region)
{
    if (!c->d_perbase) return fail(c, GD_E_STATE, "the per-base vector was not kept (gd_set_outputs)");
    for (size_t r = 0; r < n_regions; ++r) {
        if (end[r] == start[r]) continue;
        const ContigHost& h = c->contigs[tid[r]];
        gd::DhRegion t{};
        t.base_off = h.base_off;
        t.start = start[r]; t.end = end[r];
        t.g0 = start[r] - (int64_t)((reinterpret_cast<uintptr_t>(c->d_perbase + h.base_off + start[r]) >> 2) & 3u);
        t.chunk_off = (uint32_t)chunk_region->size();
        t.row = (uint32_t)r;
        const size_t nch = (size_t)((end[r] - t.g0 + gd::DH_CHUNK - 1) / gd::DH_CHUNK);
        if (r > 0xfffffff0ull || chunk_region->size() + nch > 0x7ffffff0ull) return fail(c, GD_E_RANGE, "%s: too many positions in one batch", what);
        chunk_region->insert(chunk_region->end(), nch, (uint32_t)tab->size());
        tab->push_back(t);
    }
    return GD_OK;
}

// The call's device block: the region table, the chunk table, `n_out` counters (zeroed) and, with `stats`, the scalars.
static int dist_upload(gd_ctx* c, const std::vector<gd::DhRegion>& tab, const std::vector<uint32_t>& chunk_region, size_t n_out, bool stats, gd::DhJob* j)
{
    const size_t o_cr = tab.size() * sizeof(gd::DhRegion), o_out = (o_cr + chunk_region.size() * 4 + 15) & ~(size_t)15;
    const size_t o_st = o_out + n_out * 8;
    if (int r = ensure_dev(c, c->d_dist, o_st + sizeof(gd::DhStats))) return r;
    uint8_t* base = c->d_dist.get();
    j->perbase = c->d_perbase;
    j->tab = reinterpret_cast<const gd::DhRegion*>(base);
    j->chunk_region = reinterpret_cast<const uint32_t*>(base + o_cr);
    j->n_chunks = (uint32_t)chunk_region.size();
    j->out = reinterpret_cast<unsigned long long*>(base + o_out);
    j->stats = reinterpret_cast<gd::DhStats*>(base + o_st);
    HIPCHK(c, hipMemcpyAsync(base, tab.data(), o_cr, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(base + o_cr, chunk_region.data(), chunk_region.size() * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(j->out, 0, n_out * 8, c->stream));
    if (stats) {
        const gd::DhStats s0{0ull, INT32_MAX, INT32_MIN};
        HIPCHK(c, hipMemcpyAsync(j->stats, &s0, sizeof s0, hipMemcpyHostToDevice, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));                // (the tables are the caller's stack; and the parts are timed apart)
    return GD_OK;
}

int gd_depth_hist(gd_ctx* c, size_t n_regions, const int32_t* tid, const int64_t* start, const int64_t* end, int32_t n_bins,
                  uint64_t* bins, int64_t* sum, int32_t* min, int32_t* max)
{
    if (!c || !bins || (n_regions && (!tid || !start || !end))) return GD_E_INVALID;
    if (int r = in_flight(c)) return r;
    std::vector<gd::DhRegion> tab;
    std::vector<uint32_t> chunk_region;
    if (int r = dist_check(c, n_regions, tid, start, end)) return r;
    if (n_bins < 1 || n_bins > GD_DEPTH_HIST_MAX_BINS) return fail(c, GD_E_INVALID, "depth hist: 1 .. %d bins, not %d", GD_DEPTH_HIST_MAX_BINS, n_bins);
    if (int r = dist_tables(c, "depth hist", n_regions, tid, start, end, &tab, &chunk_region)) return r;
    c->dist_secs[0] = c->dist_secs[1] = c->dist_secs[2] = 0;
    for (int32_t k = 0; k < n_bins; ++k) bins[k] = 0;
    if (sum) *sum = 0;
    if (min) *min = 0;
    if (max) *max = 0;
    if (tab.empty()) return GD_OK;
    if (int r = set_device(c)) return r;

    gd::DhJob j{};
    j.top = (uint32_t)(n_bins - 1);
    const double t0 = ing_now();
    if (int r = dist_upload(c, tab, chunk_region, (size_t)n_bins, true, &j)) return r;
    c->dist_secs[0] = ing_now() - t0;
    // a few workgroups a CU, each striding over the chunk table; more of them where one would see 2^30 positions
    int cus = 0;
    HIPCHK(c, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device));
    const uint32_t persistent = (uint32_t)std::max(cus, 1) * gd::DH_WG_PER_CU;
    const uint32_t grid = std::max(std::min(j.n_chunks, persistent), (j.n_chunks + gd::DH_MAX_CHUNKS_PER_WG - 1) / gd::DH_MAX_CHUNKS_PER_WG);
    const double t1 = ing_now();
    hipLaunchKernelGGL(gd::gd_dh_hist_kernel, dim3(grid), dim3(gd::DH_WG), 0, c->stream, j);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->dist_secs[1] = ing_now() - t1;
    const double t2 = ing_now();
    gd::DhStats s{};
    HIPCHK(c, hipMemcpyAsync(bins, j.out, (size_t)n_bins * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&s, j.stats, sizeof s, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->dist_secs[2] = ing_now() - t2;
    if (sum) *sum = (int64_t)s.sum;
    if (min) *min = s.min;
    if (max) *max = s.max;
    return GD_OK;
}

int gd_region_bins(gd_ctx* c, size_t n_regions, const int32_t* tid, const int64_t* start, const int64_t* end, int n_cuts,
                   const int32_t* cuts, uint64_t* counts)
{
    if (!c || (n_regions && (!tid || !start || !end || !counts))) return GD_E_INVALID;
    if (int r = in_flight(c)) return r;
    std::vector<gd::DhRegion> tab;
    std::vector<uint32_t> chunk_region;
    if (int r = dist_check(c, n_regions, tid, start, end)) return r;
    if (n_cuts < 0 || n_cuts > GD_PERBASE_MAX_CUTS) return fail(c, GD_E_INVALID, "region bins: 0 .. %d cuts, not %d", GD_PERBASE_MAX_CUTS, n_cuts);
    if (n_cuts > 0 && !cuts) return GD_E_INVALID;
    for (int k = 0; k < n_cuts; ++k) {
        if (cuts[k] < 1) return fail(c, GD_E_INVALID, "region bins: cut %d is %d: a cut is at least 1", k, cuts[k]);
        if (k && cuts[k] <= cuts[k - 1]) return fail(c, GD_E_INVALID, "region bins: cut %d (%d) is not above cut %d (%d)", k, cuts[k], k - 1, cuts[k - 1]);
    }
    if (int r = dist_tables(c, "region bins", n_regions, tid, start, end, &tab, &chunk_region)) return r;
    c->dist_secs[0] = c->dist_secs[1] = c->dist_secs[2] = 0;
    const size_t n_out = n_regions * (size_t)(n_cuts + 1);
    if (tab.empty()) {
        for (size_t i = 0; i < n_out; ++i) counts[i] = 0;
        return GD_OK;
    }
    if (int r = set_device(c)) return r;

    gd::DhJob j{};
    j.n_cuts = n_cuts;
    for (int k = 0; k < n_cuts; ++k) j.cuts[k] = cuts[k];
    const double t0 = ing_now();
    if (int r = dist_upload(c, tab, chunk_region, n_out, false, &j)) return r;
    c->dist_secs[0] = ing_now() - t0;
    const double t1 = ing_now();
    hipLaunchKernelGGL(gd::gd_dh_region_bins_kernel, dim3(j.n_chunks), dim3(gd::DH_WG), 0, c->stream, j);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->dist_secs[1] = ing_now() - t1;
    const double t2 = ing_now();
    HIPCHK(c, hipMemcpyAsync(counts, j.out, n_out * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->dist_secs[2] = ing_now() - t2;
    return GD_OK;
}

int gd_dist_timing(gd_ctx* c, double* out, size_t n)
{
    if (!c || !out) return GD_E_INVALID;
    for (size_t i = 0; i < n && i < 3; ++i) out[i] = c->dist_secs[i];
    return GD_OK;
}
