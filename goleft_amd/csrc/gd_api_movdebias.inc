// gd_api_movdebias.inc -- dcnv's GeneralDebiaser, a moving median over the rows in covariate order (part of gd_api.hip,
// inside extern "C"; DESIGN.md section 3.15).  The argsort of the covariate (debiaser.go:56-76; ties by row) is host work
// inside the call (gd_matcheck.hpp), the windows and the division are gd_movdebias.hpp's kernel.  gd_moving_debias_cells is the form for the
// int64 cells gd_depthwed_device leaves: gd_devmat.hpp's conversion into a buffer of the call's own (a window reads rows
// other workgroups divide, so the division cannot run in place), then the same kernel into the caller's device matrix.
// Nothing is kept between calls but the timings.

namespace {

// what both forms check before anything else, in gd_moving_debias's order
static int md_check(gd_ctx* c, size_t n_rows, int n_samples, bool pointers, const double* vals, int window)
{
    if (n_samples < 1 || n_samples > gd::MD_MAX_N)
        return fail(c, GD_E_RANGE, "moving debias: 1 .. %d samples, not %d", gd::MD_MAX_N, n_samples);
    if (window < 1 || window > gd::MD_MAX_W || (window & 1) == 0)
        return fail(c, GD_E_RANGE, "moving debias: the window must be odd and 1 .. %d, not %d", gd::MD_MAX_W, window);
    if (n_rows < (size_t)((window - 1) / 2 + 1) || n_rows > 0x7fffffffull)
        return fail(c, GD_E_RANGE, "moving debias: %d .. 2^31 - 1 rows for a window of %d, not %zu", (window - 1) / 2 + 1, window,
                    n_rows);
    if (!pointers || !vals) return GD_E_INVALID;
    for (size_t r = 0; r < n_rows; ++r)
        if (!std::isfinite(vals[r])) return fail(c, GD_E_INVALID, "moving debias: the value of row %zu is not finite", r);
    return GD_OK;
}

// The host's share of a call (the order) and the device's, after the checks.  Host form (d_from null): depths goes up into
// a buffer of the call's own, the quotients into another and back to out / med.  Resident form: the buffer of the call's own
// gets (float)d_from, the quotients go to d_resident; depths, out and med are null.
static int md_run(gd_ctx* c, const float* depths, const int64_t* d_from, float* d_resident, size_t n_rows, int n_samples,
                  const double* vals, int window, float* out, double* med)
{
    const size_t N = (size_t)n_samples;
    const double t0 = ing_now();
    const std::vector<uint32_t> order = gdm::argsort(vals, n_rows);
    if (int r = set_device(c)) return r;
    for (double& s : c->md_secs) s = 0;
    c->md_secs[0] = ing_now() - t0;

    DevBuf d_cells, d_order, d_out, d_med, negative;
    const size_t cells = n_rows * N;
    const double t1 = ing_now();
    if (int r = d_cells.alloc(c, cells * sizeof(float))) return r;
    if (int r = d_order.alloc(c, n_rows * sizeof(uint32_t))) return r;
    if (!d_resident) if (int r = d_out.alloc(c, cells * sizeof(float))) return r;
    if (med) if (int r = d_med.alloc(c, cells * sizeof(double))) return r;
    if (!d_resident) HIPCHK(c, hipMemcpyAsync(d_cells.get(), depths, cells * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_order.get(), order.data(), n_rows * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->md_secs[1] = ing_now() - t1;

    gd::MdJob j{};
    j.cells = d_cells.as<const uint32_t>();
    j.n_rows = (int64_t)n_rows; j.n = n_samples; j.window = window;
    j.segment = c->md_segment > 0 ? c->md_segment : window <= gd::MD_CAP_MID ? gd::MD_SEG_SMALL : gd::MD_SEG_BIG;
    j.order = d_order.as<const uint32_t>();
    j.out = d_resident ? d_resident : d_out.as<float>(); j.med = d_med.as<double>();
    const dim3 grid((unsigned)(((int64_t)n_rows + j.segment - 1) / j.segment), (unsigned)((N + gd::MD_COLS - 1) / gd::MD_COLS));
    const dim3 wg(gd::MD_COLS);
    const double t2 = ing_now();
    if (d_resident) {
        // The conversion, and its verdict before anything else runs: a negative cell leaves the caller's matrix alone.
        if (int r = dm_from_cells(c, d_from, d_cells.as<float>(), n_rows, n_samples, negative)) return r;
        if (int r = dm_refuse_negative(c, "moving debias", negative)) return r;
    }
    if (window <= gd::MD_CAP_SMALL) hipLaunchKernelGGL(gd::gd_movdebias_kernel<gd::MD_CAP_SMALL>, grid, wg, 0, c->stream, j);
    else if (window <= gd::MD_CAP_MID) hipLaunchKernelGGL(gd::gd_movdebias_kernel<gd::MD_CAP_MID>, grid, wg, 0, c->stream, j);
    else hipLaunchKernelGGL(gd::gd_movdebias_kernel<gd::MD_CAP_BIG>, grid, wg, 0, c->stream, j);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->md_secs[2] = ing_now() - t2;

    const double t3 = ing_now();
    if (out) HIPCHK(c, hipMemcpyAsync(out, d_out.get(), cells * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (med) HIPCHK(c, hipMemcpyAsync(med, d_med.get(), cells * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->md_secs[3] = ing_now() - t3;
    return GD_OK;
}

}  // namespace

int gd_moving_debias(gd_ctx* c, const float* depths, size_t n_rows, int n_samples, const double* vals, int window, float* out,
                     double* med)
{
    if (!c) return GD_E_INVALID;
    if (int r = md_check(c, n_rows, n_samples, depths && out, vals, window)) return r;
    if (int r = mat_check(c, "moving debias", depths, n_rows, n_samples)) return r;
    return md_run(c, depths, nullptr, nullptr, n_rows, n_samples, vals, window, out, med);
}

int gd_moving_debias_cells(gd_ctx* c, const int64_t* d_cells, size_t n_rows, int n_samples, const double* vals, int window,
                           float* d_out)
{
    if (!c) return GD_E_INVALID;
    if (int r = md_check(c, n_rows, n_samples, d_cells && d_out, vals, window)) return r;
    const size_t cells = n_rows * (size_t)n_samples;
    if (gdm::overlap(d_cells, cells * sizeof(int64_t), d_out, cells * sizeof(float)))
        return fail(c, GD_E_INVALID, "moving debias: the quotients would overlap the cells they are made of");
    return md_run(c, nullptr, d_cells, d_out, n_rows, n_samples, vals, window, nullptr, nullptr);
}

int gd_moving_debias_timing(gd_ctx* c, double* out, size_t n)
{
    if (!c || !out) return GD_E_INVALID;
    for (size_t i = 0; i < n && i < 4; ++i) out[i] = c->md_secs[i];
    return GD_OK;
}
