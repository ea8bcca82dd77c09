// gd_api_emcnv.inc -- emdepth.Cache on the device (part of gd_api.hip, inside extern "C"; after gd_api_emdepth.inc, whose
// checks and launch it uses): gd_emcnv_begin / add / add_cells / finish / read / end / timing.  The kernels are
// gd_emcnv.hpp's.  Between the blocks the context keeps, on the device: the positions, one member bit per cell, the
// members' values (depth, cn, log2fc: the arena), each row's offset into it, and the states of the last row.  Everything
// that joins members into CNVs runs in gd_emcnv_finish over those, so the result cannot depend on the blocks.

namespace {

struct EcState {
    int n = 0, words = 0;
    size_t R = 0;                                // rows so far
    uint64_t members = 0;                        // ... and their members
    int cur = 0;                                 // carry[cur]: the states of row R - 1
    bool finished = false;
    uint64_t n_cnvs = 0, n_members = 0;
    double secs[4] = {0, 0, 0, 0};               // upload, EM kernel, CNV kernels, read-back
    // kept for the whole run (grow-only)
    DevArr<uint8_t> carry[2];
    DevArr<uint32_t> start, end;
    DevArr<uint64_t> mbits, rowoff;
    DevArr<float> m_depth;
    DevArr<uint8_t> m_cn;
    DevArr<float> m_fc;
    // a block's temporaries (grow-only, nothing kept in them)
    DevArr<float> in, scale;
    DevArr<double> lambda;
    DevArr<uint8_t> cn;
    DevArr<float> fc;
    DevArr<uint32_t> rowcnt;
    DevArr<uint64_t> tiles;
    DevArr<uint64_t> total;                      // one word: a scan's total
    // the result (gd_emcnv_finish)
    DevArr<uint32_t> c_sample, c_psize, c_emit, c_count, c_last;
    DevArr<uint64_t> member_off;
    DevArr<uint32_t> o_row;
    DevArr<float> o_depth;
    DevArr<uint8_t> o_cn;
    DevArr<float> o_fc;
};

// workgroups of the two per-block kernels, which stride over the rows
static unsigned ec_grid(uint64_t items, uint64_t per_wg)
{
    return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((items + per_wg - 1) / per_wg, (uint64_t)gd::EMCNV_MAX_GRID));
}

// workgroups that cover `items`, `per_wg` each (the callers' bounds keep it below 2^31)
static unsigned ec_cover(uint64_t items, uint64_t per_wg) { return (unsigned)std::max<uint64_t>(1, (items + per_wg - 1) / per_wg); }

// out[i] = base + in[0] + .. + in[i - 1] for i < n; d_total[0] = base + all (both on the device); n >= 1
static int ec_scan(gd_ctx* c, EcState& s, const uint32_t* in, uint64_t n, uint64_t base, uint64_t* out, uint64_t* d_total)
{
    const uint64_t tiles = (n + gd::EMCNV_SCAN_TILE - 1) / gd::EMCNV_SCAN_TILE;
    if (int r = ensure_dev(c, s.tiles, (size_t)tiles)) return r;
    hipLaunchKernelGGL(gd::gd_emcnv_scan_tile_kernel, dim3((unsigned)tiles), dim3(gd::EMCNV_WG), 0, c->stream, in, n, s.tiles);
    hipLaunchKernelGGL(gd::gd_emcnv_scan_top_kernel, dim3(1), dim3(gd::EMCNV_WG), 0, c->stream, s.tiles, tiles, base, d_total);
    hipLaunchKernelGGL(gd::gd_emcnv_scan_apply_kernel, dim3((unsigned)tiles), dim3(gd::EMCNV_WG), 0, c->stream, in, n,
                       (const uint64_t*)s.tiles.get(), out);
    HIPCHK(c, hipGetLastError());
    return GD_OK;
}

static int ec_fetch(gd_ctx* c, const uint64_t* d_word, uint64_t* out)
{
    HIPCHK(c, hipMemcpyAsync(out, d_word, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return GD_OK;
}

// One block whose rows are on the device.  The state moves on only when everything has run.
static int ec_add(gd_ctx* c, EcState& s, bool cells, const void* d_in, const float* d_scale, size_t B, const uint32_t* starts,
                  const uint32_t* ends, uint8_t* cn_out)
{
    const size_t N = (size_t)s.n, W = (size_t)s.words, R = s.R;
    double t0 = ing_now();
    // (ensure_dev copies what is kept on the copy stream and waits for both streams: the copy stream is idle during a run,
    // and the compute stream has been waited for wherever an array that is kept grows)
    if (int r = ensure_dev(c, s.start, R + B, true, R)) return r;
    if (int r = ensure_dev(c, s.end, R + B, true, R)) return r;
    if (int r = ensure_dev(c, s.mbits, (R + B) * W, true, R * W)) return r;
    if (int r = ensure_dev(c, s.rowoff, R + B, true, R)) return r;
    if (int r = ensure_dev(c, s.lambda, B * gd::EM_CENTRES)) return r;
    if (int r = ensure_dev(c, s.cn, B * N)) return r;
    if (int r = ensure_dev(c, s.fc, B * N)) return r;
    if (int r = ensure_dev(c, s.rowcnt, B)) return r;
    HIPCHK(c, hipMemcpyAsync(s.start + R, starts, B * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(s.end + R, ends, B * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    s.secs[0] += ing_now() - t0;

    double em_s = 0;
    if (int r = em_launch(c, cells, d_in, d_scale, B, s.n, s.lambda, nullptr, s.cn, s.fc, &em_s)) return r;
    s.secs[1] += em_s;

    t0 = ing_now();
    gd::EmcnvBlock j{};
    j.cells = d_in; j.scale = d_scale; j.lambda = s.lambda; j.cn = s.cn; j.log2fc = s.fc;
    j.n_rows = (int64_t)B; j.row0 = (int64_t)R; j.n = s.n; j.words = s.words;
    j.carry_in = s.carry[s.cur]; j.carry_out = s.carry[s.cur ^ 1];
    j.mbits = s.mbits; j.rowcnt = s.rowcnt; j.rowoff = s.rowoff;
    const dim3 grid(ec_grid(B, gd::EMCNV_WAVES)), wg(gd::EMCNV_WG);
    if (cells) hipLaunchKernelGGL(gd::gd_emcnv_member_kernel<int64_t>, grid, wg, 0, c->stream, j);
    else hipLaunchKernelGGL(gd::gd_emcnv_member_kernel<float>, grid, wg, 0, c->stream, j);
    HIPCHK(c, hipGetLastError());
    if (int r = ec_scan(c, s, s.rowcnt, B, s.members, s.rowoff + R, s.total)) return r;
    uint64_t total = 0;
    if (int r = ec_fetch(c, s.total, &total)) return r;
    if (total > s.members) {
        if (int r = ensure_dev(c, s.m_depth, (size_t)total, true, (size_t)s.members)) return r;
        if (int r = ensure_dev(c, s.m_cn, (size_t)total, true, (size_t)s.members)) return r;
        if (int r = ensure_dev(c, s.m_fc, (size_t)total, true, (size_t)s.members)) return r;
        j.m_depth = s.m_depth; j.m_cn = s.m_cn; j.m_fc = s.m_fc;
        if (cells) hipLaunchKernelGGL(gd::gd_emcnv_gather_kernel<int64_t>, grid, wg, 0, c->stream, j);
        else hipLaunchKernelGGL(gd::gd_emcnv_gather_kernel<float>, grid, wg, 0, c->stream, j);
        HIPCHK(c, hipGetLastError());
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    s.secs[2] += ing_now() - t0;
    if (cn_out) {
        t0 = ing_now();
        HIPCHK(c, hipMemcpyAsync(cn_out, s.cn, B * N, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        s.secs[3] += ing_now() - t0;
    }
    s.R = R + B;
    s.members = total;
    s.cur ^= 1;
    return GD_OK;
}

#define EC_STATE(c)                                                                                       \
    if (!(c)) return GD_E_INVALID;                                                                        \
    if (!(c)->ec) return fail((c), GD_E_STATE, "gd_emcnv_begin has not been called");                     \
    if (int r_ = set_device(c)) return r_;                                                                \
    EcState& s = *(c)->ec

static int ec_check_add(gd_ctx* c, EcState& s, size_t n_rows, const void* rows, const uint32_t* starts, const uint32_t* ends)
{
    if (s.finished) return fail(c, GD_E_STATE, "emcnv: gd_emcnv_finish has run: gd_emcnv_begin starts another");
    if (n_rows == 0) return GD_OK;
    if (!rows || !starts || !ends) return GD_E_INVALID;
    // (F holds R + 1 in 32 bits)
    if (n_rows > 0xfffffffdull - s.R) return fail(c, GD_E_RANGE, "emcnv: more than 2^32 - 3 rows");
    return em_check_fit(c, "emcnv", n_rows, s.n);
}

}  // namespace

int gd_emcnv_begin(gd_ctx* c, int n_samples)
{
    if (!c) return GD_E_INVALID;
    if (int r = em_check_n(c, n_samples)) return r;      // (a refused begin leaves an earlier state alone)
    if (int r = set_device(c)) return r;
    drop_state(c, c->ec);
    c->ec.reset(new (std::nothrow) EcState());
    if (!c->ec) return GD_E_NOMEM;
    EcState& s = *c->ec;
    auto body = [&]() -> int {
        s.n = n_samples;
        s.words = (n_samples + 63) / 64;
        for (auto& p : s.carry) HIPCHK(c, p.alloc((size_t)s.words * 64));
        HIPCHK(c, s.scale.alloc((size_t)n_samples));
        HIPCHK(c, s.total.alloc(1));
        return GD_OK;
    };
    const int rc = body();
    if (rc != GD_OK) drop_state(c, c->ec);
    return rc;
}

int gd_emcnv_add(gd_ctx* c, const float* depths, size_t n_rows, const uint32_t* starts, const uint32_t* ends, uint8_t* cn_out)
{
    EC_STATE(c);
    if (int r = ec_check_add(c, s, n_rows, depths, starts, ends)) return r;
    if (n_rows == 0) return GD_OK;
    const size_t N = (size_t)s.n;
    if (int r = mat_check(c, "emcnv", depths, n_rows, s.n)) return r;
    const double t0 = ing_now();
    if (int r = ensure_dev(c, s.in, n_rows * N)) return r;
    HIPCHK(c, hipMemcpyAsync(s.in, depths, n_rows * N * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    s.secs[0] += ing_now() - t0;
    return ec_add(c, s, false, s.in, nullptr, n_rows, starts, ends, cn_out);
}

int gd_emcnv_add_cells(gd_ctx* c, const int64_t* d_cells, size_t n_rows, const float* scale, const uint32_t* starts,
                       const uint32_t* ends, uint8_t* cn_out)
{
    EC_STATE(c);
    const size_t N = (size_t)s.n;
    if (scale) if (int r = mat_check_scale(c, "emcnv", scale, s.n)) return r;
    if (int r = ec_check_add(c, s, n_rows, d_cells, starts, ends)) return r;
    if (n_rows == 0) return GD_OK;
    if (scale) {
        const double t0 = ing_now();
        HIPCHK(c, hipMemcpyAsync(s.scale, scale, N * sizeof(float), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        s.secs[0] += ing_now() - t0;
    }
    return ec_add(c, s, true, d_cells, scale ? s.scale.get() : nullptr, n_rows, starts, ends, cn_out);
}

// gd_emcnv_add for float32 rows that are in HBM already: gd_devmat.hpp's check in place of the host's, no upload
int gd_emcnv_add_device(gd_ctx* c, const float* d_depths, size_t n_rows, const uint32_t* starts, const uint32_t* ends,
                        uint8_t* cn_out)
{
    EC_STATE(c);
    if (int r = ec_check_add(c, s, n_rows, d_depths, starts, ends)) return r;
    if (n_rows == 0) return GD_OK;
    if (int r = dm_check(c, "emcnv", d_depths, n_rows, s.n)) return r;
    return ec_add(c, s, false, d_depths, nullptr, n_rows, starts, ends, cn_out);
}

int gd_emcnv_finish(gd_ctx* c, uint64_t* n_cnvs, uint64_t* n_members)
{
    EC_STATE(c);
    if (!s.finished && s.R > 0) {
        const double t0 = ing_now();
        const size_t R = s.R, W = (size_t)s.words, pad = W * 64;
        const size_t n_chunks = (R + gd::EMCNV_CHUNK - 1) / gd::EMCNV_CHUNK;
        DevList tmp;
        gd::EmcnvJob j{};
        j.R = (uint32_t)R; j.n = s.n; j.words = s.words; j.n_chunks = (uint32_t)n_chunks;
        j.start = s.start; j.end = s.end; j.mbits = s.mbits; j.rowoff = s.rowoff;
        j.m_depth = s.m_depth; j.m_cn = s.m_cn; j.m_fc = s.m_fc;
        uint32_t* ecnt = nullptr;
        uint64_t* eoff = nullptr;
        const size_t n1 = (R + 63) / 64, n2 = (n1 + 63) / 64;
        if (int r = tmp.alloc(c, &j.F, R)) return r;
        if (int r = tmp.alloc(c, &j.span1, n1 * 4)) return r;
        if (int r = tmp.alloc(c, &j.span2, n2 * 4)) return r;
        if (int r = tmp.alloc(c, &j.first, n_chunks * pad)) return r;
        if (int r = tmp.alloc(c, &j.last, n_chunks * pad)) return r;
        if (int r = tmp.alloc(c, &j.lastF, n_chunks * pad)) return r;
        if (int r = tmp.alloc(c, &j.tail, n_chunks * pad)) return r;
        if (int r = tmp.alloc(c, &j.psize, R + 1, true)) return r;
        if (int r = tmp.alloc(c, &ecnt, R + 1, true)) return r;
        if (int r = tmp.alloc(c, &j.ebits, (R + 1) * W, true)) return r;
        if (int r = tmp.alloc(c, &eoff, R + 1)) return r;
        j.ecnt = ecnt; j.eoff = eoff;
        const dim3 wg(gd::EMCNV_WG), walk(ec_cover(n_chunks * W, gd::EMCNV_WAVES));
        hipLaunchKernelGGL(gd::gd_emcnv_span_kernel<1>, dim3(ec_cover(n1, gd::EMCNV_WAVES)), wg, 0, c->stream, j);
        hipLaunchKernelGGL(gd::gd_emcnv_span_kernel<2>, dim3(ec_cover(n2, gd::EMCNV_WAVES)), wg, 0, c->stream, j);
        hipLaunchKernelGGL(gd::gd_emcnv_gap_kernel, dim3(ec_cover(R, gd::EMCNV_WG)), wg, 0, c->stream, j);
        hipLaunchKernelGGL(gd::gd_emcnv_chunk_kernel, walk, wg, 0, c->stream, j);
        hipLaunchKernelGGL(gd::gd_emcnv_carry_kernel, dim3((unsigned)((pad + gd::EMCNV_WG - 1) / gd::EMCNV_WG)), wg, 0, c->stream, j);
        hipLaunchKernelGGL(gd::gd_emcnv_emit_kernel<0>, walk, wg, 0, c->stream, j);
        HIPCHK(c, hipGetLastError());
        if (int r = ec_scan(c, s, ecnt, R + 1, 0, eoff, s.total)) return r;
        uint64_t n_c = 0, n_m = 0;
        if (int r = ec_fetch(c, s.total, &n_c)) return r;
        if (n_c > 0x7fffffffull * gd::EMCNV_WAVES) return fail(c, GD_E_RANGE, "emcnv: more than 2^33 - 4 CNVs");
        // the result is the state's only once it is whole (until then this call owns it, and frees it on return)
        DevArr<uint32_t> c_sample, c_psize, c_emit, c_count, c_last, o_row;
        DevArr<uint64_t> member_off;
        DevArr<float> o_depth, o_fc;
        DevArr<uint8_t> o_cn;
        HIPCHK(c, c_sample.alloc(n_c));
        HIPCHK(c, c_psize.alloc(n_c));
        HIPCHK(c, c_emit.alloc(n_c));
        HIPCHK(c, c_count.alloc(n_c));
        HIPCHK(c, c_last.alloc(n_c));
        HIPCHK(c, member_off.alloc(n_c + 1));
        HIPCHK(c, hipMemsetAsync(member_off, 0, (n_c + 1) * sizeof(uint64_t), c->stream));
        if (n_c > 0) {
            j.c_sample = c_sample; j.c_psize = c_psize; j.c_emit = c_emit; j.c_count = c_count; j.c_last = c_last;
            j.n_cnvs = n_c;
            hipLaunchKernelGGL(gd::gd_emcnv_emit_kernel<1>, walk, wg, 0, c->stream, j);
            HIPCHK(c, hipGetLastError());
            if (int r = ec_scan(c, s, c_count, n_c, 0, member_off, member_off + n_c)) return r;
            if (int r = ec_fetch(c, member_off + n_c, &n_m)) return r;
            HIPCHK(c, o_row.alloc(n_m));
            HIPCHK(c, o_depth.alloc(n_m));
            HIPCHK(c, o_cn.alloc(n_m));
            HIPCHK(c, o_fc.alloc(n_m));
            j.member_off = member_off;
            j.o_row = o_row; j.o_depth = o_depth; j.o_cn = o_cn; j.o_fc = o_fc;
            hipLaunchKernelGGL(gd::gd_emcnv_members_kernel, dim3(ec_cover(n_c, gd::EMCNV_WAVES)), wg, 0, c->stream, j);
            HIPCHK(c, hipGetLastError());
        }
        HIPCHK(c, hipStreamSynchronize(c->stream));
        // (onto empty owners -- this runs once per gd_emcnv_begin -- so the moves free nothing)
        s.c_sample = std::move(c_sample); s.c_psize = std::move(c_psize); s.c_emit = std::move(c_emit);
        s.c_count = std::move(c_count); s.c_last = std::move(c_last); s.member_off = std::move(member_off);
        s.o_row = std::move(o_row); s.o_depth = std::move(o_depth); s.o_cn = std::move(o_cn); s.o_fc = std::move(o_fc);
        s.n_cnvs = n_c; s.n_members = n_m;
        s.secs[2] += ing_now() - t0;
    }
    s.finished = true;
    if (n_cnvs) *n_cnvs = s.n_cnvs;
    if (n_members) *n_members = s.n_members;
    return GD_OK;
}

int gd_emcnv_read(gd_ctx* c, uint32_t* sample, uint32_t* psize, uint32_t* emit_row, uint64_t* member_off, uint32_t* member_row,
                  float* depth, uint8_t* cn, float* log2fc)
{
    EC_STATE(c);
    if (!s.finished) return fail(c, GD_E_STATE, "emcnv: gd_emcnv_finish has not been called");
    const double t0 = ing_now();
    const size_t nc = (size_t)s.n_cnvs, nm = (size_t)s.n_members;
    if (member_off && !s.member_off) member_off[0] = 0;      // (no rows at all)
    if (s.member_off) {
        if (sample && nc) HIPCHK(c, hipMemcpyAsync(sample, s.c_sample, nc * 4, hipMemcpyDeviceToHost, c->stream));
        if (psize && nc) HIPCHK(c, hipMemcpyAsync(psize, s.c_psize, nc * 4, hipMemcpyDeviceToHost, c->stream));
        if (emit_row && nc) HIPCHK(c, hipMemcpyAsync(emit_row, s.c_emit, nc * 4, hipMemcpyDeviceToHost, c->stream));
        if (member_off) HIPCHK(c, hipMemcpyAsync(member_off, s.member_off, (nc + 1) * 8, hipMemcpyDeviceToHost, c->stream));
        if (member_row && nm) HIPCHK(c, hipMemcpyAsync(member_row, s.o_row, nm * 4, hipMemcpyDeviceToHost, c->stream));
        if (depth && nm) HIPCHK(c, hipMemcpyAsync(depth, s.o_depth, nm * 4, hipMemcpyDeviceToHost, c->stream));
        if (cn && nm) HIPCHK(c, hipMemcpyAsync(cn, s.o_cn, nm, hipMemcpyDeviceToHost, c->stream));
        if (log2fc && nm) HIPCHK(c, hipMemcpyAsync(log2fc, s.o_fc, nm * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    s.secs[3] += ing_now() - t0;
    return GD_OK;
}

int gd_emcnv_end(gd_ctx* c)
{
    if (!c) return GD_E_INVALID;
    if (int r = set_device(c)) return r;
    drop_state(c, c->ec);
    return GD_OK;
}

int gd_emcnv_timing(gd_ctx* c, double* out, size_t n)
{
    EC_STATE(c);
    if (!out) return GD_E_INVALID;
    for (size_t i = 0; i < n && i < 4; ++i) out[i] = s.secs[i];
    return GD_OK;
}
