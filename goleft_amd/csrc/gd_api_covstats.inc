// gd_api_covstats.inc -- `goleft covstats` on the fed ranges of the device BAM read: begin (n, skip) / decode (walk,
// scan, histograms of the oldest pending range) / histogram (part of gd_api.hip, inside extern "C").  The walk is
// gd_bamdecode.hpp's, the other kernels gd_covstats.hpp's; what a decode begins with (the oldest range, its inflate, virtual
// offsets, the walk's page-locked tables) is gd_api_ingest.inc's, shared with the depth read.

namespace {

struct CovState {
    int64_t target = 0, skip_left = 0;
    gd_covstats_counts tot{};                  // over every range decoded since gd_covstats_begin
    std::vector<int64_t> ovf[3];               // overflow values read back after every range
    DevArr<uint8_t> d_slots, d_recs, d_role, d_tile, d_ovf;   // in bytes (IngestBufs::fit)
    DevArr<unsigned long long> d_acc;          // [CS_ACC_WORDS]
    DevArr<unsigned long long> d_hist;         // [3 * CS_HBINS]
};

// The virtual offset of byte b of the inflated range (b == total: where the member after the range begins).
static uint64_t cov_at(const IngestState* g, uint64_t b)
{
    if (b >= g->total) return (g->base + g->m_end[g->nm - 1]) << 16;
    const size_t k = (size_t)(std::upper_bound(g->out_off.begin(), g->out_off.end(), b) - g->out_off.begin()) - 1;
    return (g->m_coff[k] << 16) | (b - g->out_off[k]);
}

}  // namespace

int gd_covstats_begin(gd_ctx* c, int64_t n, int64_t skip)
{
    if (!c || skip < 0) return GD_E_INVALID;
    if (int r = set_device(c)) return r;
    if (!c->cov) {
        c->cov.reset(new (std::nothrow) CovState());
        if (!c->cov) return GD_E_NOMEM;
    }
    CovState& s = *c->cov;
    if (!s.d_acc) HIPCHK(c, s.d_acc.alloc(gd::CS_ACC_WORDS));
    if (!s.d_hist) HIPCHK(c, s.d_hist.alloc(3ull * gd::CS_HBINS));
    HIPCHK(c, hipMemsetAsync(s.d_acc, 0, gd::CS_ACC_WORDS * sizeof(unsigned long long), c->stream));
    HIPCHK(c, hipMemsetAsync(s.d_hist, 0, 3ull * gd::CS_HBINS * sizeof(unsigned long long), c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    s.target = n;
    s.skip_left = skip;
    s.tot = gd_covstats_counts{};
    s.tot.skip_left = skip;
    for (auto& v : s.ovf) v.clear();
    return GD_OK;
}

int gd_covstats_decode(gd_ctx* c, uint64_t first_voffset, const uint64_t* anchors, size_t n_anchors, int last_range,
                       gd_covstats_counts* out)
{
    if (!c || !out || (n_anchors && !anchors)) return GD_E_INVALID;
    if (!c->cov) return fail(c, GD_E_STATE, "gd_covstats_begin has not been called");
    IngestGuard guard{c, false};
    IngestState* g = nullptr;
    if (int r = ingest_oldest(c, &guard, &g)) return r;
    CovState& s = *c->cov;
    const uint64_t total = g->total;
    // ---- segments: the first record, then every anchor of the range behind it -------------------------------
    uint64_t b0 = 0;
    if (!ingest_voff(g, first_voffset, &b0))
        return fail(c, GD_E_INVALID, "the first record (virtual offset %llu) is not inside a member of the range",
                    (unsigned long long)first_voffset);
    std::vector<uint64_t> beg{b0};
    const uint64_t* a = std::upper_bound(anchors, anchors + n_anchors, first_voffset);
    for (; a != anchors + n_anchors; ++a) {
        uint64_t b = 0;
        if ((*a >> 16) > g->m_coff[g->nm - 1]) break;       // (behind the range)
        if (!ingest_voff(g, *a, &b) || b >= total) continue;   // (an anchor in a record the range holds only in part)
        if (b > beg.back()) beg.push_back(b);
    }
    const size_t n_seg = beg.size();
    if (n_seg > 0xfffffff0ull) return fail(c, GD_E_RANGE, "too many anchors");
    if (int r = ingest_wait_inflated(c, g)) return r;
    const double td1 = ing_now();
    // the walk's per-segment tables (page-locked: the kernels read and write them over the link)
    if (int r = ingest_walk_table(c, n_seg * (5 * sizeof(uint64_t) + 2 * sizeof(uint32_t)), "covstats")) return r;
    uint64_t* t_beg = c->h_walk.as<uint64_t>();
    uint64_t* t_end = t_beg + n_seg;
    uint64_t* t_slot = t_end + n_seg;
    uint64_t* t_rbase = t_slot + n_seg;
    uint64_t* t_endoff = t_rbase + n_seg;
    uint32_t* t_nrec = reinterpret_cast<uint32_t*>(t_endoff + n_seg);
    uint32_t* t_flags = t_nrec + n_seg;
    uint64_t n_slots = 0;
    for (size_t i = 0; i < n_seg; ++i) {
        t_beg[i] = beg[i];
        t_end[i] = i + 1 < n_seg ? beg[i + 1] : total;
        t_slot[i] = n_slots;
        n_slots += (t_end[i] - t_beg[i]) / 36 + 1;
    }
    if (!IngestBufs::fit(s.d_slots, (size_t)n_slots * sizeof(gd::CsRec)))
        return fail(c, GD_E_NOMEM, "device allocation for the covstats walk failed");
    gd::CsWalkJob wj{};
    wj.data = g->d_out; wj.n_bytes = total; wj.seg_beg = t_beg; wj.seg_end = t_end; wj.slot_base = t_slot;
    wj.n_seg = (uint32_t)n_seg; wj.open_end = last_range ? 0u : 1u; wj.slots = s.d_slots.as<gd::CsRec>();
    wj.n_rec = t_nrec; wj.end_off = t_endoff; wj.flags = t_flags;
    hipLaunchKernelGGL(gd::gd_cs_walk_kernel, dim3((unsigned)n_seg), dim3(64), 0, c->stream, wj);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    uint64_t N = 0;
    for (size_t i = 0; i < n_seg; ++i) {
        if (t_flags[i] & gd::BW_CORRUPT) return fail(c, GD_E_INVALID, "corrupt BAM record in covstats segment %zu", i);
        if (t_flags[i] & gd::BW_OVERRAN) return fail(c, GD_E_INVALID, "anchor %zu is not a record start (stale or foreign index?)", i);
        if (i + 1 < n_seg && t_endoff[i] != t_end[i])
            return fail(c, GD_E_INVALID, "covstats segment %zu ends inside a record", i);
        t_rbase[i] = N;
        N += t_nrec[i];
    }
    const uint64_t stopped = t_endoff[n_seg - 1];           // the first record the range does not hold completely
    // ---- the dense array, the scan, the histograms -----------------------------------------------------------
    const uint64_t first = (uint64_t)std::min<int64_t>(s.skip_left, (int64_t)N);
    s.skip_left -= (int64_t)first;
    bool done = false;
    unsigned long long acc[gd::CS_ACC_WORDS] = {};
    if (s.target <= 0) {
        done = s.skip_left == 0;                             // the sampling loop does not run at all
    } else if (N > first) {
        if (!IngestBufs::fit(s.d_recs, (size_t)N * sizeof(gd::CsRec)) ||
            !IngestBufs::fit(s.d_role, (size_t)N) ||
            !IngestBufs::fit(s.d_ovf, 3 * (size_t)N * sizeof(int64_t)))
            return fail(c, GD_E_NOMEM, "device allocation for the covstats scan failed");
        const uint64_t n_tiles = (N + gd::CS_TILE - 1) / gd::CS_TILE;
        if (n_tiles > 0x7fffffffull) return fail(c, GD_E_RANGE, "too many records in one range");
        if (!IngestBufs::fit(s.d_tile, (size_t)n_tiles * 24))
            return fail(c, GD_E_NOMEM, "device allocation for the covstats scan failed");
        hipLaunchKernelGGL(gd::gd_cs_compact_kernel, dim3((unsigned)n_seg), dim3(256), 0, c->stream,
                           s.d_slots.as<const gd::CsRec>(), (const uint64_t*)t_slot, (const uint64_t*)t_rbase,
                           (const uint32_t*)t_nrec, (uint32_t)n_seg, s.d_recs.as<gd::CsRec>());
        HIPCHK(c, hipGetLastError());
        // the stop word and the overflow counters start over in every range (the counts go on)
        const unsigned long long reset[gd::CS_ACC_WORDS - gd::CS_ACC_STOP] = {~0ull, 0, 0, 0, 0};
        HIPCHK(c, hipMemcpyAsync(s.d_acc + gd::CS_ACC_STOP, reset, sizeof reset, hipMemcpyHostToDevice, c->stream));
        gd::CsScanJob sj{};
        sj.rec = s.d_recs.as<const gd::CsRec>(); sj.n = N; sj.first = first; sj.target = s.target;
        sj.sizes0 = s.tot.sizes; sj.ins0 = s.tot.inserts;
        uint64_t* tw = s.d_tile.as<uint64_t>();
        sj.pre_g = tw; sj.pre_e = tw + n_tiles;
        sj.tile_g = reinterpret_cast<uint32_t*>(tw + 2 * n_tiles); sj.tile_e = sj.tile_g + n_tiles;
        sj.n_tiles = (uint32_t)n_tiles;
        sj.role = s.d_role.as<uint8_t>(); sj.acc = s.d_acc; sj.hist = s.d_hist;
        sj.ovf = s.d_ovf.as<int64_t>(); sj.ovf_cap = N;
        hipLaunchKernelGGL(gd::gd_cs_tile_kernel, dim3((unsigned)n_tiles), dim3(256), 0, c->stream, sj);
        hipLaunchKernelGGL(gd::gd_cs_tscan_kernel, dim3(1), dim3(256), 0, c->stream, sj);
        hipLaunchKernelGGL(gd::gd_cs_select_kernel, dim3((unsigned)n_tiles), dim3(256), 0, c->stream, sj);
        hipLaunchKernelGGL(gd::gd_cs_hist_kernel, dim3((unsigned)n_tiles), dim3(256), 0, c->stream, sj);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(acc, s.d_acc, sizeof acc, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        done = acc[gd::CS_ACC_STOP] != ~0ull;
        for (int k = 0; k < 3; ++k) {
            const uint64_t m = acc[gd::CS_ACC_OVF + k];
            if (m > N) return fail(c, GD_E_INVALID, "covstats overflow list out of room (internal error)");
            if (!m) continue;
            std::vector<int64_t>& v = s.ovf[k];
            const size_t at = v.size();
            v.resize(at + (size_t)m);
            HIPCHK(c, hipMemcpy(v.data() + at, s.d_ovf.as<int64_t>() + (size_t)k * N, (size_t)m * sizeof(int64_t),
                                hipMemcpyDeviceToHost));
        }
        s.tot.unmapped = (int64_t)acc[0]; s.tot.counted = (int64_t)acc[1]; s.tot.bad = (int64_t)acc[2];
        s.tot.dup = (int64_t)acc[3]; s.tot.proper = (int64_t)acc[4]; s.tot.sizes = (int64_t)acc[5];
        s.tot.inserts = (int64_t)acc[6];
    }
    c->ing_secs[4] += ing_now() - td1;
    s.tot.records += (int64_t)N;
    s.tot.skip_left = s.skip_left;
    s.tot.done = done ? 1 : 0;
    s.tot.range_records = (int64_t)N;
    s.tot.resume = cov_at(g, stopped);
    *out = s.tot;
    guard.on = false;
    ingest_pop(c);
    return GD_OK;
}

int gd_covstats_histogram(gd_ctx* c, int which, int64_t* lo, size_t* n_bins, uint64_t* bins, int64_t* overflow, size_t cap,
                          size_t* n_overflow)
{
    if (!c || which < 0 || which > 2) return GD_E_INVALID;
    if (!c->cov || !c->cov->d_hist) return fail(c, GD_E_STATE, "gd_covstats_begin has not been called");
    if (int r = set_device(c)) return r;
    const CovState& s = *c->cov;
    if (lo) *lo = which == 0 ? gd::CS_LO_SIZE : which == 1 ? gd::CS_LO_INS : gd::CS_LO_TL;
    if (n_bins) *n_bins = gd::CS_HBINS;
    if (n_overflow) *n_overflow = s.ovf[which].size();
    if (bins) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, hipMemcpy(bins, s.d_hist + (size_t)which * gd::CS_HBINS, gd::CS_HBINS * sizeof(uint64_t), hipMemcpyDeviceToHost));
    }
    if (overflow) {
        if (cap < s.ovf[which].size()) return fail(c, GD_E_CAPACITY, "%zu overflow values, room for %zu", s.ovf[which].size(), cap);
        if (!s.ovf[which].empty()) memcpy(overflow, s.ovf[which].data(), s.ovf[which].size() * sizeof(int64_t));
    }
    return GD_OK;
}
