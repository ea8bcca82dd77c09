// gd_api_index.inc -- a BAM's .bai or .csi from the fed ranges of the device BAM read: begin (references, first record, file
// size; gd_index_begin_csi: and the binning scheme)
// / decode (guess, walk and confirm, runs, linear index of the oldest pending range) / result (part of gd_api.hip, inside
// extern "C").  The guesses are gd_bamguess.hpp's, the walk gd_bamdecode.hpp's (IndexWalk), the other kernels
// gd_baiindex.hpp's; what a decode begins with is gd_api_ingest.inc's, shared with the depth read and covstats.  The
// .bai's bytes are assembled on the host (gdh_bai_assemble, host/index_host.cpp).

namespace {

struct IdxState {
    int32_t n_ref = 0;
    std::vector<uint64_t> lin_off;             // [n_ref + 1]
    uint64_t next_voff = 0, file_size = 0;     // where the next range's first record begins; where the file's last record must end
    bool has_prev = false, finished = false;
    std::vector<int64_t> ref_len;              // as given
    uint64_t slack = 4;                        // windows every reference has beyond its length (grows when a read hangs further over)
    uint32_t min_shift = 14, depth = 5;        // the binning scheme: a .bai's unless gd_index_begin_csi gave another
    int64_t max_end = 1ll << 29;               // where a placed record may end at most
    bool csi = false;
    gd::IdxRec prev{};                         // the last record of the range before
    std::vector<gd_index_run> runs;            // in file order, unplaced ones (ref -1) included: they end the run in front
    gd_index_counts tot{};
    DevArr<int32_t> d_ref_len;
    DevArr<uint64_t> d_lin_off;
    DevArr<unsigned long long> d_lin, d_ref_cnt, d_acc;
    DevArr<uint8_t> d_slots, d_recs, d_runs, d_tile, d_mtab;   // in bytes (IngestBufs::fit)
};

// One segment of the guess-and-confirm loop.  `end` (the guess behind it) never moves; `beg` moves forward to where the
// segment in front stopped.
struct IdxSeg {
    uint64_t beg, end, slot, endoff = 0;
    uint32_t nrec = 0, flags = 0;
    bool ok = false, dirty = true;
};

// The most windows a reference can have: what the geometry can address (32768 in a .bai).
static uint64_t idx_max_windows(const IdxState& s) { return ((uint64_t)s.max_end + (1ull << s.min_shift) - 1) >> s.min_shift; }

// A reference's share of the linear array: its length in windows of 2^min_shift positions (16 kb in a .bai) and `slack`
// more (a read may hang over the end), at most what the geometry can address.
static void idx_layout(IdxState& s)
{
    s.lin_off.assign((size_t)s.n_ref + 1, 0);
    const uint64_t win = 1ull << s.min_shift;
    for (int32_t r = 0; r < s.n_ref; ++r) {
        const uint64_t len = (uint64_t)std::max<int64_t>(0, std::min<int64_t>(s.ref_len[(size_t)r], s.max_end));
        s.lin_off[(size_t)r + 1] = s.lin_off[(size_t)r] + std::min<uint64_t>((len + win - 1) / win + s.slack, idx_max_windows(s));
    }
}

}  // namespace

// gd_index_begin and gd_index_begin_csi: the state, the window array, the counters
static int idx_begin(gd_ctx* c, int32_t n_ref, const int64_t* ref_len, uint64_t first_voffset, uint64_t file_size, bool csi,
                     int32_t min_shift, int32_t depth)
{
    if (!c || n_ref < 0 || (n_ref && !ref_len)) return GD_E_INVALID;
    if (int r = set_device(c)) return r;
    drop_state(c, c->idx);
    c->idx.reset(new (std::nothrow) IdxState());
    if (!c->idx) return GD_E_NOMEM;
    IdxState& s = *c->idx;
    s.n_ref = n_ref;
    s.next_voff = first_voffset;
    s.file_size = file_size;
    s.ref_len.assign(ref_len, ref_len + n_ref);
    s.csi = csi;
    s.min_shift = (uint32_t)min_shift;
    s.depth = (uint32_t)depth;
    s.max_end = std::min<int64_t>(1ll << (min_shift + 3 * depth), 0x7fffffffll);
    std::vector<int32_t> len32((size_t)n_ref);
    for (int32_t r = 0; r < n_ref; ++r) len32[(size_t)r] = (int32_t)std::min<int64_t>(ref_len[r] < 0 ? 0 : ref_len[r], 0x7fffffff);
    idx_layout(s);
    const size_t n_lin = (size_t)s.lin_off[(size_t)n_ref];
    HIPCHK(c, s.d_ref_len.alloc((size_t)n_ref));
    HIPCHK(c, s.d_lin_off.alloc((size_t)n_ref + 1));
    HIPCHK(c, s.d_lin.alloc(n_lin));
    HIPCHK(c, s.d_ref_cnt.alloc(2 * (size_t)n_ref));
    HIPCHK(c, s.d_acc.alloc(gd::IX_ACC_WORDS));
    if (n_ref) HIPCHK(c, hipMemcpyAsync(s.d_ref_len, len32.data(), (size_t)n_ref * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(s.d_lin_off, s.lin_off.data(), ((size_t)n_ref + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(s.d_lin, 0xff, std::max<size_t>(n_lin, 1) * sizeof(unsigned long long), c->stream));
    HIPCHK(c, hipMemsetAsync(s.d_ref_cnt, 0, std::max<size_t>(2 * (size_t)n_ref, 1) * sizeof(unsigned long long), c->stream));
    HIPCHK(c, hipMemsetAsync(s.d_acc, 0, gd::IX_ACC_WORDS * sizeof(unsigned long long), c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (double& t : c->idx_secs) t = 0;
    return GD_OK;
}

int gd_index_begin(gd_ctx* c, int32_t n_ref, const int64_t* ref_len, uint64_t first_voffset, uint64_t file_size)
{
    return idx_begin(c, n_ref, ref_len, first_voffset, file_size, false, 14, 5);
}

int gd_index_begin_csi(gd_ctx* c, int32_t n_ref, const int64_t* ref_len, uint64_t first_voffset, uint64_t file_size,
                       int32_t min_shift, int32_t depth)
{
    if (!c) return GD_E_INVALID;
    if (min_shift < 8 || min_shift > 24) return fail(c, GD_E_INVALID, "min_shift %d: a .csi is made with 8 to 24", min_shift);
    if (depth < 0 || depth > 8) return fail(c, GD_E_INVALID, "depth %d: a .csi is made with 0 to 8 levels", depth);
    return idx_begin(c, n_ref, ref_len, first_voffset, file_size, true, min_shift, depth);
}

int gd_index_decode(gd_ctx* c, int last_range, gd_index_counts* out)
{
    if (!c || !out) return GD_E_INVALID;
    if (!c->idx) return fail(c, GD_E_STATE, "gd_index_begin has not been called");
    if (c->idx->finished) return fail(c, GD_E_STATE, "the file's last range has been decoded");
    IngestGuard guard{c, false};
    IngestState* g = nullptr;
    if (int r = ingest_oldest(c, &guard, &g)) return r;
    IdxState& s = *c->idx;
    const uint64_t total = g->total;
    uint64_t b0 = 0;
    if (!ingest_voff(g, s.next_voff, &b0)) {
        // (every record of the range before was whole: the member behind it, which may be the file's end)
        if (s.next_voff == ((g->base + g->m_end[g->nm - 1]) << 16)) b0 = total;
        else return fail(c, GD_E_INVALID, "the next record (virtual offset %llu) is not inside a member of the range",
                         (unsigned long long)s.next_voff);
    }
    const double t0 = ing_now();
    if (int r = ingest_wait_inflated(c, g)) return r;
    const double t1 = ing_now();
    c->idx_secs[0] += t1 - t0;
    // ---- the members, for the virtual offsets ------------------------------------------------------------------
    if (!IngestBufs::fit(s.d_mtab, 2 * g->nm * sizeof(uint64_t)))
        return fail(c, GD_E_NOMEM, "device allocation for the index walk failed");
    uint64_t* const d_mout = s.d_mtab.as<uint64_t>();
    uint64_t* const d_mcoff = d_mout + g->nm;
    HIPCHK(c, hipMemcpyAsync(d_mout, g->out_off.data(), g->nm * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_mcoff, g->m_coff.data(), g->nm * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
    // ---- guesses: one per slice -------------------------------------------------------------------------------------
    const uint64_t slice = (uint64_t)c->idx_slice;
    const uint64_t n_slice64 = b0 < total ? (total - b0 + slice - 1) / slice : 0;
    if (n_slice64 > 0x7ffffff0ull) return fail(c, GD_E_RANGE, "too many slices in one range");
    const size_t n_slice = (size_t)n_slice64;
    if (int r = ingest_walk_table(c, n_slice * (5 * sizeof(uint64_t) + 2 * sizeof(uint32_t)) + 64, "index")) return r;
    uint64_t* const t_guess = c->h_walk.as<uint64_t>();
    uint64_t* const t_beg = t_guess + n_slice;
    uint64_t* const t_end = t_beg + n_slice;
    uint64_t* const t_slot = t_end + n_slice;            // (the compaction: record bases)
    uint64_t* const t_endoff = t_slot + n_slice;
    uint32_t* const t_nrec = reinterpret_cast<uint32_t*>(t_endoff + n_slice);
    uint32_t* const t_flags = t_nrec + n_slice;
    std::vector<IdxSeg> segs;
    int rounds = 0, guesses = 0;
    uint64_t N = 0, stopped = b0;
    const uint64_t n_slots = b0 < total ? (total - b0) / 36 + n_slice + 2 : 0;
    if (n_slice) {
        gd::GuessJob gj{};
        gj.data = g->d_out; gj.n_bytes = total; gj.first = b0; gj.slice = slice; gj.n_slice = (uint32_t)n_slice;
        gj.checks = (uint32_t)c->idx_checks; gj.n_ref = s.n_ref; gj.ref_len = s.d_ref_len; gj.guess = t_guess;
        hipLaunchKernelGGL(gd::gd_bam_guess_kernel, dim3((unsigned)n_slice), dim3(64), 0, c->stream, gj);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipStreamSynchronize(c->stream));
        const double t2 = ing_now();
        c->idx_secs[1] += t2 - t1;
        // ---- segments [guess, next guess); slot room by the bytes in front of a segment and its number ----------------
        for (size_t k = 0; k < n_slice; ++k) {
            const uint64_t gs = t_guess[k];
            if (gs == ~0ull || gs >= total || gs < b0 || (!segs.empty() && gs <= segs.back().beg)) continue;
            if (!segs.empty()) segs.back().end = gs;
            IdxSeg sg{};
            sg.beg = gs; sg.end = total; sg.slot = segs.size();   // (its number, for now)
            segs.push_back(sg);
        }
        guesses = (int)segs.size();
        if (!IngestBufs::fit(s.d_slots, (size_t)n_slots * sizeof(gd::IdxRec)))
            return fail(c, GD_E_NOMEM, "device allocation for the index walk failed");
        gd::IdxWalkJob wj{};
        wj.data = g->d_out; wj.n_bytes = total; wj.seg_beg = t_beg; wj.seg_end = t_end; wj.slot_base = t_slot;
        wj.open_end = last_range ? 0u : 1u; wj.slots = s.d_slots.as<gd::IdxRec>(); wj.n_slots = n_slots;
        wj.n_rec = t_nrec; wj.end_off = t_endoff; wj.flags = t_flags; wj.m_out = d_mout; wj.m_coff = d_mcoff;
        wj.n_mem = (uint32_t)g->nm; wj.n_ref = s.n_ref;
        wj.min_shift = s.min_shift; wj.depth = s.depth; wj.max_end = s.max_end;
        std::vector<size_t> which;
        for (int walk = 0;; ++walk) {
            // ---- walk what has not been walked from its present start ----------------------------------------------
            which.clear();
            for (size_t k = 0; k < segs.size(); ++k) {
                if (!segs[k].dirty) continue;
                const size_t m = which.size();
                t_beg[m] = segs[k].beg; t_end[m] = segs[k].end;
                t_slot[m] = (segs[k].beg - b0) / 36 + segs[k].slot;
                which.push_back(k);
            }
            if (which.empty()) break;
            if (walk) ++rounds;
            wj.n_seg = (uint32_t)which.size();
            hipLaunchKernelGGL(gd::gd_idx_walk_kernel, dim3(wj.n_seg), dim3(64), 0, c->stream, wj);
            HIPCHK(c, hipGetLastError());
            HIPCHK(c, hipStreamSynchronize(c->stream));
            for (size_t m = 0; m < which.size(); ++m) {
                IdxSeg& sg = segs[which[m]];
                sg.endoff = t_endoff[m]; sg.nrec = t_nrec[m]; sg.flags = t_flags[m]; sg.dirty = false;
            }
            // ---- confirm and repair ------------------------------------------------------------------------------------
            // Only a CONFIRMED walk is believed.  Along the confirmed chain: a segment that lies wholly inside the record the
            // chain's last walk stopped behind has no start in it and goes; the next one is confirmed when the chain stopped
            // exactly on it, else its start BECOMES where the chain stopped (forwards or, after a speculation, back) and the
            // chain ends there for this round.  Behind the chain nothing is dropped and nothing is decided: a segment whose
            // unconfirmed predecessor stopped inside it is moved there on speculation (walks resynchronise within a record
            // or two), so that the next round usually confirms many at once; the chain overrules it when it arrives.
            std::vector<IdxSeg> kept;
            kept.reserve(segs.size());
            bool chain = true;
            for (size_t k = 0; k < segs.size(); ++k) {
                IdxSeg sg = segs[k];
                if (kept.empty()) { sg.ok = true; kept.push_back(sg); continue; }
                const IdxSeg& p = kept.back();
                if (chain) {
                    if (p.flags & gd::BW_CORRUPT)
                        return fail(c, GD_E_INVALID, "corrupt BAM record between inflated offsets %llu and %llu of the range at file offset %llu",
                                    (unsigned long long)p.beg, (unsigned long long)p.end, (unsigned long long)g->base);
                    if (p.endoff < p.end) break;                                 // it met the record the range's end cuts: nothing behind it
                    if (p.endoff >= sg.end) continue;                            // one record spans the whole segment: no start in it
                    if (p.endoff == sg.beg && !sg.dirty) sg.ok = true;
                    else { sg.beg = p.endoff; sg.dirty = true; sg.ok = false; chain = false; }
                } else {
                    sg.ok = false;
                    const bool p_clean = !p.dirty && !(p.flags & gd::BW_CORRUPT) && p.endoff >= p.end;
                    if (p_clean && p.endoff > sg.beg && p.endoff < sg.end) { sg.beg = p.endoff; sg.dirty = true; }
                }
                kept.push_back(sg);
            }
            segs.swap(kept);
            // ---- after a few rounds: what is still unconfirmed becomes one segment behind the confirmed ones ----------
            if (rounds >= c->idx_repair_rounds) {
                size_t f = 0;
                while (f < segs.size() && segs[f].ok) ++f;
                if (f < segs.size()) {
                    // (the first unconfirmed segment is where the chain ended above: its start is where the chain stopped)
                    segs[f].end = total; segs[f].dirty = true;
                    segs.resize(f + 1);
                }
            }
        }
        for (const IdxSeg& sg : segs)
            if (!sg.ok) return fail(c, GD_E_INVALID, "a segment of the index walk was left unconfirmed (internal error)");
        for (size_t k = 0; k + 1 < segs.size(); ++k)
            if (segs[k].flags & gd::BW_CORRUPT)
                return fail(c, GD_E_INVALID, "corrupt BAM record between inflated offsets %llu and %llu of the range at file offset %llu",
                            (unsigned long long)segs[k].beg, (unsigned long long)segs[k].end, (unsigned long long)g->base);
        const IdxSeg& lastseg = segs.back();
        if (lastseg.flags & gd::BW_CORRUPT)
            return fail(c, GD_E_INVALID, last_range ? "corrupt BAM record, or a record cut by the end of the file (behind inflated offset %llu of the range at file offset %llu)"
                                                    : "corrupt BAM record behind inflated offset %llu of the range at file offset %llu",
                        (unsigned long long)lastseg.beg, (unsigned long long)g->base);
        for (size_t k = 0; k < segs.size(); ++k) {
            t_beg[k] = (segs[k].beg - b0) / 36 + segs[k].slot;                   // slot base
            t_slot[k] = N;                                                       // record base
            t_nrec[k] = segs[k].nrec;
            N += segs[k].nrec;
        }
        stopped = lastseg.endoff;
        c->idx_secs[2] += ing_now() - t2;
    }
    const double t3 = ing_now();
    const uint64_t resume = cov_at(g, stopped);
    if (last_range && stopped != total)
        return fail(c, GD_E_INVALID, "a record cut by the end of the file");
    if (last_range && resume != s.file_size << 16)
        return fail(c, GD_E_INVALID, "the last range ends at file offset %llu, the file at %llu", (unsigned long long)(resume >> 16),
                    (unsigned long long)s.file_size);
    // ---- dense records, runs, linear index -----------------------------------------------------------------------------
    uint64_t K = 0;
    unsigned long long acc[gd::IX_ACC_WORDS] = {};
    std::vector<gd_index_run> heads;
    // (the run that was open when the range before ended goes on to this range's first head, or through the whole range:
    // below, once the heads are known.  A range without a whole record only moves its end)
    if (!N && !s.runs.empty()) s.runs.back().end = resume;
    if (N) {
        const uint64_t n_tiles = (N + gd::IX_TILE - 1) / gd::IX_TILE;
        if (n_tiles > 0x7fffffffull) return fail(c, GD_E_RANGE, "too many records in one range");
        if (!IngestBufs::fit(s.d_recs, (size_t)N * sizeof(gd::IdxRec)) || !IngestBufs::fit(s.d_runs, (size_t)N * sizeof(gd::IdxRun)) ||
            !IngestBufs::fit(s.d_tile, (size_t)n_tiles * 12))
            return fail(c, GD_E_NOMEM, "device allocation for the index runs failed");
        hipLaunchKernelGGL(gd::gd_idx_compact_kernel, dim3((unsigned)segs.size()), dim3(256), 0, c->stream,
                           s.d_slots.as<const gd::IdxRec>(), (const uint64_t*)t_beg, (const uint64_t*)t_slot, (const uint32_t*)t_nrec,
                           (uint32_t)segs.size(), s.d_recs.as<gd::IdxRec>(), N);
        HIPCHK(c, hipGetLastError());
        unsigned long long reset[gd::IX_ACC_WORDS - gd::IX_ACC_HEADS];
        reset[0] = reset[1] = 0;                                 // heads, windows beyond the array
        for (size_t k = 2; k < gd::IX_ACC_WORDS - gd::IX_ACC_HEADS; ++k) reset[k] = ~0ull;
        HIPCHK(c, hipMemcpyAsync(s.d_acc + gd::IX_ACC_HEADS, reset, sizeof reset, hipMemcpyHostToDevice, c->stream));
        gd::IdxJob ij{};
        ij.rec = s.d_recs.as<const gd::IdxRec>(); ij.n = N; ij.rec0 = (uint64_t)s.tot.records;
        ij.has_prev = s.has_prev ? 1 : 0; ij.prev_ref = s.prev.ref; ij.prev_bin = (int32_t)(s.prev.bin & gd::IX_BIN); ij.prev_beg = s.prev.beg;
        ij.tile_base = s.d_tile.as<uint64_t>(); ij.tile_cnt = reinterpret_cast<uint32_t*>(ij.tile_base + n_tiles);
        ij.n_tiles = (uint32_t)n_tiles; ij.n_ref = s.n_ref; ij.runs = s.d_runs.as<gd::IdxRun>(); ij.runs_cap = N;
        ij.ref_cnt = s.d_ref_cnt; ij.acc = s.d_acc; ij.lin_off = s.d_lin_off; ij.lin = s.d_lin;
        ij.min_shift = s.min_shift;
        hipLaunchKernelGGL(gd::gd_idx_tile_kernel, dim3((unsigned)n_tiles), dim3(256), 0, c->stream, ij);
        hipLaunchKernelGGL(gd::gd_idx_tscan_kernel, dim3(1), dim3(256), 0, c->stream, ij);
        hipLaunchKernelGGL(gd::gd_idx_runs_kernel, dim3((unsigned)n_tiles), dim3(256), 0, c->stream, ij);
        hipLaunchKernelGGL(gd::gd_idx_linear_kernel, dim3((unsigned)n_tiles), dim3(256), 0, c->stream, ij);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(acc, s.d_acc, sizeof acc, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (acc[gd::IX_ACC_OVER]) {
            // a read hangs further over its reference's end than the array has windows: every reference gets that many more
            // (what was there is copied reference by reference; this happens once or twice a file, if ever), and the linear
            // kernel runs again over this range -- its minima are the same wherever they were taken before
            const std::vector<uint64_t> old_off = s.lin_off;
            s.slack = std::min<uint64_t>(s.slack + acc[gd::IX_ACC_OVER], idx_max_windows(s));
            idx_layout(s);
            DevArr<unsigned long long> grown;
            const size_t n_new = (size_t)s.lin_off[(size_t)s.n_ref];
            HIPCHK(c, grown.alloc(n_new));
            HIPCHK(c, hipMemsetAsync(grown, 0xff, std::max<size_t>(n_new, 1) * sizeof(unsigned long long), c->stream));
            for (int32_t r = 0; r < s.n_ref; ++r)
                if (old_off[(size_t)r + 1] > old_off[(size_t)r])
                    HIPCHK(c, hipMemcpyAsync(grown + s.lin_off[(size_t)r], s.d_lin + old_off[(size_t)r],
                                             (size_t)(old_off[(size_t)r + 1] - old_off[(size_t)r]) * sizeof(unsigned long long), hipMemcpyDeviceToDevice, c->stream));
            HIPCHK(c, hipMemcpyAsync(s.d_lin_off, s.lin_off.data(), ((size_t)s.n_ref + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
            const unsigned long long zero = 0;
            HIPCHK(c, hipMemcpyAsync(s.d_acc + gd::IX_ACC_OVER, &zero, sizeof zero, hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            s.d_lin = std::move(grown);
            ij.lin = s.d_lin;
            hipLaunchKernelGGL(gd::gd_idx_linear_kernel, dim3((unsigned)n_tiles), dim3(256), 0, c->stream, ij);
            HIPCHK(c, hipGetLastError());
            unsigned long long over = 0;
            HIPCHK(c, hipMemcpyAsync(&over, s.d_acc + gd::IX_ACC_OVER, sizeof over, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            if (over) return fail(c, GD_E_INVALID, "the linear index did not grow far enough (internal error)");
        }
        const double t4 = ing_now();
        c->idx_secs[3] += t4 - t3;
        // ---- refusals: the first offender of each kind, the earliest of them named -----------------------------------------
        char span_what[160] = "a placed record with a negative position or an end beyond 2^29: a .bai cannot hold it";
        if (s.csi)
            snprintf(span_what, sizeof span_what, "a placed record with a negative position or an end beyond %lld: an index with min_shift %u "
                     "and depth %u cannot hold it", (long long)s.max_end, s.min_shift, s.depth);
        const struct { uint32_t word; int code; const char* what; } kinds[] = {
            {gd::IX_ERR_SPAN, GD_E_INVALID, span_what},
            {gd::IX_ERR_PLACED, GD_E_UNSORTED, "a placed record after an unplaced one"},
            {gd::IX_ERR_RESUME, GD_E_UNSORTED, "a reference resumes after another began"},
            {gd::IX_ERR_BACK, GD_E_UNSORTED, "positions go backwards inside a reference"}};
        int worst = -1;
        for (int k = 0; k < 4; ++k)
            if (acc[kinds[k].word] != ~0ull && (worst < 0 || acc[kinds[k].word] < acc[kinds[worst].word])) worst = k;
        if (worst >= 0) {
            const uint64_t ord = acc[kinds[worst].word];
            gd::IdxRec bad{};
            if (ord >= ij.rec0 && ord - ij.rec0 < N)
                HIPCHK(c, hipMemcpy(&bad, s.d_recs.as<gd::IdxRec>() + (ord - ij.rec0), sizeof bad, hipMemcpyDeviceToHost));
            return fail(c, kinds[worst].code, "record %llu (reference %d, position %d, virtual offset %llu): %s", (unsigned long long)ord,
                        bad.ref, bad.beg, (unsigned long long)bad.vbeg, kinds[worst].what);
        }
        K = acc[gd::IX_ACC_HEADS];
        if (K > N) return fail(c, GD_E_INVALID, "more runs than records (internal error)");
        heads.resize((size_t)K);
        if (K) HIPCHK(c, hipMemcpy(heads.data(), s.d_runs.as<gd::IdxRun>(), (size_t)K * sizeof(gd_index_run), hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(&s.prev, s.d_recs.as<gd::IdxRec>() + (N - 1), sizeof s.prev, hipMemcpyDeviceToHost));
        s.has_prev = true;
        if (!s.runs.empty()) s.runs.back().end = K ? heads[0].beg : resume;
        if (K) {
            heads.back().end = resume;
            s.runs.insert(s.runs.end(), heads.begin(), heads.end());
        }
        s.tot.n_no_coor = (int64_t)acc[gd::IX_ACC_NO_COOR];
        c->idx_secs[4] += ing_now() - t4;
    }
    s.tot.records += (int64_t)N;
    s.tot.range_records = (int64_t)N;
    s.tot.runs = (int64_t)s.runs.size();
    s.tot.resume = resume;
    s.tot.slices = (int32_t)n_slice;
    s.tot.guesses = guesses;
    s.tot.rounds = rounds;
    s.next_voff = resume;
    if (last_range) s.finished = true;
    *out = s.tot;
    guard.on = false;
    ingest_pop(c);
    return GD_OK;
}

int gd_index_result(gd_ctx* c, gd_index_run* runs, size_t cap_runs, size_t* n_runs, uint64_t* linear, size_t cap_linear,
                    size_t* n_linear, gd_index_ref* refs, uint64_t* n_no_coor)
{
    if (!c) return GD_E_INVALID;
    if (!c->idx) return fail(c, GD_E_STATE, "gd_index_begin has not been called");
    if (int r = set_device(c)) return r;
    const IdxState& s = *c->idx;
    if (!s.finished && s.tot.records) return fail(c, GD_E_STATE, "the file's last range has not been decoded");
    size_t nr = 0;
    for (const gd_index_run& r : s.runs) nr += r.ref >= 0;
    const size_t nl = (size_t)s.lin_off[(size_t)s.n_ref];
    if (n_runs) *n_runs = nr;
    if (n_linear) *n_linear = nl;
    if (n_no_coor) *n_no_coor = (uint64_t)s.tot.n_no_coor;
    if ((runs && cap_runs < nr) || (linear && cap_linear < nl))
        return fail(c, GD_E_CAPACITY, "%zu runs and %zu linear entries, room for %zu and %zu", nr, nl, cap_runs, cap_linear);
    if (runs) {
        size_t k = 0;
        for (const gd_index_run& r : s.runs)
            if (r.ref >= 0) runs[k++] = r;
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (linear && nl) HIPCHK(c, hipMemcpy(linear, s.d_lin, nl * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (refs && s.n_ref) {
        std::vector<unsigned long long> cnt(2 * (size_t)s.n_ref);
        HIPCHK(c, hipMemcpy(cnt.data(), s.d_ref_cnt, cnt.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        for (int32_t r = 0; r < s.n_ref; ++r) refs[r] = gd_index_ref{0, 0, cnt[2 * (size_t)r], cnt[2 * (size_t)r + 1]};
        // a reference's records are one stretch of the file (the order checks): its first run begins it, its last ends it
        std::vector<char> seen((size_t)s.n_ref, 0);
        for (const gd_index_run& r : s.runs) {
            if (r.ref < 0 || r.ref >= s.n_ref) continue;
            if (!seen[(size_t)r.ref]) { refs[r.ref].first_beg = r.beg; seen[(size_t)r.ref] = 1; }
            refs[r.ref].last_end = r.end;
        }
    }
    return GD_OK;
}

int gd_index_windows(gd_ctx* c, uint64_t* lin_off, size_t cap)
{
    if (!c || !lin_off) return GD_E_INVALID;
    if (!c->idx) return fail(c, GD_E_STATE, "gd_index_begin has not been called");
    const IdxState& s = *c->idx;
    if (cap < s.lin_off.size()) return fail(c, GD_E_CAPACITY, "%zu offsets, room for %zu", s.lin_off.size(), cap);
    memcpy(lin_off, s.lin_off.data(), s.lin_off.size() * sizeof(uint64_t));
    return GD_OK;
}

int gd_index_timing(gd_ctx* c, double* out, size_t n)
{
    if (!c || (n && !out)) return GD_E_INVALID;
    for (size_t k = 0; k < n && k < 5; ++k) out[k] = c->idx_secs[k];
    return GD_OK;
}
