// gd_api_chunkdebias.inc -- dcnv's ChunkDebiaser per covariate chunk of a depth matrix (part of gd_api.hip, inside
// extern "C"; DESIGN.md section 3.13).  The argsort of the covariate and the chunk walk (debiaser.go:140-148) are host work
// inside the call (gd_matcheck.hpp); the medians and the division are gd_chunkdebias.hpp's kernels.  gd_chunk_debias_cells is the form for the
// int64 cells gd_depthwed_device leaves: gd_devmat.hpp's conversion into the caller's device matrix, then the same two
// kernels on it, the division in place (section 3.14).  Nothing is kept between calls but the timings.

namespace {

// what both forms check before anything else, in gd_chunk_debias's order
static int cd_check(gd_ctx* c, size_t n_rows, int n_samples, bool pointers, const double* vals, double score_window)
{
    if (n_samples < 1 || n_samples > gd::CD_MAX_N)
        return fail(c, GD_E_RANGE, "chunk debias: 1 .. %d samples, not %d", gd::CD_MAX_N, n_samples);
    if (n_rows < 1 || n_rows > 0x7fffffffull)
        return fail(c, GD_E_RANGE, "chunk debias: 1 .. 2^31 - 1 rows, not %zu", n_rows);
    if (!pointers || !vals) return GD_E_INVALID;
    if (!std::isfinite(score_window) || !(score_window > 0))
        return fail(c, GD_E_INVALID, "chunk debias: the score window must be a finite number > 0, not %g", score_window);
    for (size_t r = 0; r < n_rows; ++r)
        if (!std::isfinite(vals[r])) return fail(c, GD_E_INVALID, "chunk debias: the value of row %zu is not finite", r);
    return GD_OK;
}

// The host's share of a call (the chunking) and the device's, after the checks.  Host form (d_resident null): depths goes up
// into a buffer of the call's own, the quotients into another and back to out / out64.  Resident form: d_resident is the
// caller's device matrix; it gets (float)d_from first, the medians are taken on it, and the division runs on it in place
// (every thread reads and writes its own index only); depths, out and out64 are null.
static int cd_run(gd_ctx* c, const float* depths, const int64_t* d_from, float* d_resident, size_t n_rows, int n_samples,
                  const double* vals, double score_window, float* out, double* out64, uint32_t* chunk_of_row, size_t* n_chunks,
                  float* med, size_t med_rows)
{
    const size_t N = (size_t)n_samples;
    // the order of the rows and the chunks over it (gd_matcheck.hpp)
    const double t0 = ing_now();
    const std::vector<uint32_t> order = gdm::argsort(vals, n_rows);
    const gdm::Chunks ch = gdm::chunk_walk(vals, order, score_window);
    const size_t C = ch.count();
    if (med && med_rows < C) {
        if (n_chunks) *n_chunks = C;             // (what the medians need)
        return fail(c, GD_E_CAPACITY, "chunk debias: %zu chunks, the medians have room for %zu", C, med_rows);
    }
    if (int r = set_device(c)) return r;
    for (double& s : c->cd_secs) s = 0;
    c->cd_secs[0] = ing_now() - t0;
    c->cd_secs[4] = (double)C;
    c->cd_secs[5] = (double)ch.largest;

    DevBuf d_cells, d_order, d_slices, d_cor, d_med, d_out, d_out64, negative;
    const size_t cells = n_rows * N;
    const double t1 = ing_now();
    if (!d_resident) if (int r = d_cells.alloc(c, cells * sizeof(float))) return r;
    if (int r = d_order.alloc(c, n_rows * sizeof(uint32_t))) return r;
    if (int r = d_slices.alloc(c, (C + 1) * sizeof(uint32_t))) return r;
    if (int r = d_cor.alloc(c, n_rows * sizeof(uint32_t))) return r;
    if (int r = d_med.alloc(c, C * N * sizeof(uint32_t))) return r;
    if (!d_resident) if (int r = d_out.alloc(c, cells * sizeof(float))) return r;
    if (out64) if (int r = d_out64.alloc(c, cells * sizeof(double))) return r;
    if (!d_resident) HIPCHK(c, hipMemcpyAsync(d_cells.get(), depths, cells * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_order.get(), order.data(), n_rows * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_slices.get(), ch.slices.data(), (C + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_cor.get(), ch.chunk_of_row.data(), n_rows * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->cd_secs[1] = ing_now() - t1;

    gd::CdJob j{};
    j.cells = static_cast<const uint32_t*>(d_resident ? (void*)d_resident : d_cells.get());
    j.n_rows = (int64_t)n_rows; j.n = n_samples; j.n_chunks = (uint32_t)C;
    j.order = d_order.as<const uint32_t>(); j.slices = d_slices.as<const uint32_t>();
    j.chunk_of_row = d_cor.as<const uint32_t>(); j.med = d_med.as<uint32_t>();
    j.out = d_resident ? d_resident : d_out.as<float>(); j.out64 = d_out64.as<double>();
    const unsigned tiles = (unsigned)((N + gd::CD_COLS - 1) / gd::CD_COLS);
    const dim3 mgrid((unsigned)std::min<size_t>(C, (size_t)gd::CD_MAX_GRID), tiles), mwg(gd::CD_WG);
    const size_t turns = (n_rows + gd::CD_DIV_WAVES - 1) / gd::CD_DIV_WAVES;
    const dim3 dgrid((unsigned)std::min<size_t>(turns, (size_t)gd::CD_DIV_MAX_GRID), tiles), dwg(gd::CD_DIV_WAVES * 64);
    const double t2 = ing_now();
    if (d_resident) {
        // The conversion, and its verdict before anything else runs: a negative cell leaves the host outputs alone.
        if (int r = dm_from_cells(c, d_from, d_resident, n_rows, n_samples, negative)) return r;
        if (int r = dm_refuse_negative(c, "chunk debias", negative)) return r;
    }
    hipLaunchKernelGGL(gd::gd_chunkdebias_median_kernel, mgrid, mwg, 0, c->stream, j);
    HIPCHK(c, hipGetLastError());
    if (getenv("GOLEFT_CHUNKDEBIAS_SPLIT")) {    // (measurement: the two kernels timed apart)
        HIPCHK(c, hipStreamSynchronize(c->stream));
        c->cd_secs[6] = ing_now() - t2;
    }
    hipLaunchKernelGGL(gd::gd_chunkdebias_divide_kernel, dgrid, dwg, 0, c->stream, j);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->cd_secs[2] = ing_now() - t2;

    const double t3 = ing_now();
    if (out) HIPCHK(c, hipMemcpyAsync(out, d_out.get(), cells * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (out64) HIPCHK(c, hipMemcpyAsync(out64, d_out64.get(), cells * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (med) HIPCHK(c, hipMemcpyAsync(med, d_med.get(), C * N * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->cd_secs[3] = ing_now() - t3;
    if (chunk_of_row) memcpy(chunk_of_row, ch.chunk_of_row.data(), n_rows * sizeof(uint32_t));
    if (n_chunks) *n_chunks = C;
    return GD_OK;
}

}  // namespace

int gd_chunk_debias(gd_ctx* c, const float* depths, size_t n_rows, int n_samples, const double* vals, double score_window,
                    float* out, double* out64, uint32_t* chunk_of_row, size_t* n_chunks, float* med, size_t med_rows)
{
    if (!c) return GD_E_INVALID;
    if (int r = cd_check(c, n_rows, n_samples, depths && out, vals, score_window)) return r;
    if (int r = mat_check(c, "chunk debias", depths, n_rows, n_samples)) return r;
    return cd_run(c, depths, nullptr, nullptr, n_rows, n_samples, vals, score_window, out, out64, chunk_of_row, n_chunks, med,
                  med_rows);
}

int gd_chunk_debias_cells(gd_ctx* c, const int64_t* d_cells, size_t n_rows, int n_samples, const double* vals,
                          double score_window, float* d_out, uint32_t* chunk_of_row, size_t* n_chunks, float* med,
                          size_t med_rows)
{
    if (!c) return GD_E_INVALID;
    if (int r = cd_check(c, n_rows, n_samples, d_cells && d_out, vals, score_window)) return r;
    const size_t cells = n_rows * (size_t)n_samples;
    if (gdm::overlap(d_cells, cells * sizeof(int64_t), d_out, cells * sizeof(float)))
        return fail(c, GD_E_INVALID, "chunk debias: the quotients would overlap the cells they are made of");
    return cd_run(c, nullptr, d_cells, d_out, n_rows, n_samples, vals, score_window, nullptr, nullptr, chunk_of_row, n_chunks,
                  med, med_rows);
}

int gd_chunk_debias_timing(gd_ctx* c, double* out, size_t n)
{
    if (!c || !out) return GD_E_INVALID;
    for (size_t i = 0; i < n && i < 7; ++i) out[i] = c->cd_secs[i];
    return GD_OK;
}
