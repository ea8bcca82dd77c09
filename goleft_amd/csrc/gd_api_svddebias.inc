// gd_api_svddebias.inc -- dcnv's SVD debiaser and its z-score scaler (part of gd_api.hip, inside extern "C"; DESIGN.md
// section 3.16).  The row statistics, the Gram matrix and the projection are gd_svddebias.hpp's kernels, the last two
// instantiated with the scaler's policy; the eigenpairs of
// the samples x samples Gram matrix, the spectrum and the cut are host work inside the call (gd_eigh.hpp).  The three forms
// run the same kernels on the same float32 bits: the host form on an upload of its own, the cells form on d_out once
// gd_devmat.hpp's conversion has filled it, the device form from d_depths into d_out (which may be d_depths).  Nothing is
// kept between calls but the timings.  The gd_svd_debias_scaled* entries name the scaler (none, z-score, or dcnv's Log2
// scaler: gd_svdlog2.hpp, DESIGN.md section 3.17) and return the centre cells; the older three forward to them.

namespace {

static int sv_check(gd_ctx* c, size_t n_rows, int n_samples, double pct)
{
    if (n_samples < gd::SV_MIN_N || n_samples > gd::SV_MAX_N)
        return fail(c, GD_E_RANGE, "svd debias: %d .. %d samples, not %d", gd::SV_MIN_N, gd::SV_MAX_N, n_samples);
    if (n_rows < 1 || n_rows > 0x7fffffffull) return fail(c, GD_E_RANGE, "svd debias: 1 .. 2^31 - 1 rows, not %zu", n_rows);
    if (!(pct >= 0.0) || !std::isfinite(pct))
        return fail(c, GD_E_RANGE, "svd debias: the variance share must be a finite number >= 0, not %g", pct);
    return GD_OK;
}

static int sv_scaler(int zscore) { return zscore ? GD_SVD_SCALER_ZSCORE : GD_SVD_SCALER_NONE; }

static int sv_check_scaler(gd_ctx* c, int scaler)
{
    if (scaler != GD_SVD_SCALER_NONE && scaler != GD_SVD_SCALER_ZSCORE && scaler != GD_SVD_SCALER_LOG2)
        return fail(c, GD_E_RANGE, "svd debias: the scaler is 0 (none), 1 (z-score) or 2 (log2), not %d", scaler);
    return GD_OK;
}

// the projection of scaler policy P, with a row's z in NV = 1, 2, 4, 8 or 16 registers a lane (a template has C++ linkage)
extern "C++" template <class P>
void sv_project(gd_ctx* c, const gd::SvJob& j, unsigned row_grid)
{
    const int nv = (j.n + 63) / 64;
    const dim3 pgrid(row_grid), pwg(gd::SV_WG);
    if (nv <= 1) hipLaunchKernelGGL((gd::gd_svd_project_kernel<P, 1>), pgrid, pwg, 0, c->stream, j);
    else if (nv <= 2) hipLaunchKernelGGL((gd::gd_svd_project_kernel<P, 2>), pgrid, pwg, 0, c->stream, j);
    else if (nv <= 4) hipLaunchKernelGGL((gd::gd_svd_project_kernel<P, 4>), pgrid, pwg, 0, c->stream, j);
    else if (nv <= 8) hipLaunchKernelGGL((gd::gd_svd_project_kernel<P, 8>), pgrid, pwg, 0, c->stream, j);
    else hipLaunchKernelGGL((gd::gd_svd_project_kernel<P, 16>), pgrid, pwg, 0, c->stream, j);
}

// After the checks: d_src (checked, on the device) to d_dst.  s, n_removed and centre_cells may be null; scaler is a
// GD_SVD_SCALER_*.  With the log2 scaler gd_colselect.hpp's select finds the centre cell of every sample first,
// gd_svdlog2.hpp's centre kernel takes the place of the row statistics, and the Gram kernel and the projection are
// instantiated with its policy.
static int sv_run(gd_ctx* c, const float* d_src, float* d_dst, size_t n_rows, int n_samples, double pct, int scaler, double* s,
                  int* n_removed, float* centre_cells)
{
    const size_t N = (size_t)n_samples;
    const int T = (n_samples + gd::SV_TILE - 1) / gd::SV_TILE;
    const size_t pairs = (size_t)T * (size_t)(T + 1) / 2;
    const size_t slabs = (n_rows + gd::SV_SLAB - 1) / gd::SV_SLAB;
    const unsigned row_grid = (unsigned)std::min<size_t>((n_rows + 3) / 4, (size_t)gd::SV_MAX_GRID);
    const bool zscore = scaler == GD_SVD_SCALER_ZSCORE, log2s = scaler == GD_SVD_SCALER_LOG2;

    DevBuf d_stats, d_part, d_gram, d_vt, d_keys, d_centre;
    const double t1 = ing_now();
    if (zscore) if (int r = d_stats.alloc(c, n_rows * 2 * sizeof(double))) return r;
    if (log2s) {
        if (int r = d_keys.alloc(c, N * sizeof(uint64_t))) return r;
        if (int r = d_centre.alloc(c, N * sizeof(double))) return r;
    }
    if (int r = d_part.alloc(c, pairs * slabs * (size_t)(gd::SV_TILE * gd::SV_TILE) * sizeof(double))) return r;
    if (int r = d_gram.alloc(c, N * N * sizeof(double))) return r;
    if (int r = d_vt.alloc(c, (size_t)gd::SV_MAX_K * N * sizeof(double))) return r;

    gd::SvJob j{};
    j.cells = d_src; j.out = d_dst; j.n_rows = (int64_t)n_rows; j.n = n_samples; j.zscore = zscore ? 1 : 0;
    j.stats = d_stats.as<double>(); j.part = d_part.as<double>(); j.gram = d_gram.as<double>(); j.vt = d_vt.as<const double>();
    j.slabs = (int32_t)slabs; j.keys = d_keys.as<const uint64_t>(); j.centre = d_centre.as<double>();
    std::vector<uint64_t> keys(log2s ? N : 0);
    const dim3 ggrid((unsigned)slabs, (unsigned)pairs), gwg(gd::SV_WG);
    if (log2s) {
        // the select is gd_sample_medians' with another rank; the seconds of the last gd_sample_medians* call stay its own
        double sm[3] = {c->sm_secs[0], c->sm_secs[1], c->sm_secs[2]};
        const int sm_passes = c->sm_passes;
        const int r = cs_run(c, false, d_src, n_rows, n_samples, keys.data(), nullptr, true, d_keys.as<uint64_t>());
        std::copy(sm, sm + 3, c->sm_secs);
        c->sm_passes = sm_passes;
        if (r) return r;
        hipLaunchKernelGGL(gd::gd_svl_centre_kernel, dim3((unsigned)((N + gd::SV_WG - 1) / gd::SV_WG)), gwg, 0, c->stream, j);
        hipLaunchKernelGGL(gd::gd_svd_gram_kernel<gd::SvLog2>, ggrid, gwg, 0, c->stream, j);
    } else {
        if (zscore) hipLaunchKernelGGL(gd::gd_svd_rowstats_kernel, dim3(row_grid), gwg, 0, c->stream, j);
        hipLaunchKernelGGL(gd::gd_svd_gram_kernel<gd::SvLinear>, ggrid, gwg, 0, c->stream, j);
    }
    hipLaunchKernelGGL(gd::gd_svd_gram_sum_kernel, dim3(gd::SV_TILE * gd::SV_TILE / gd::SV_WG, (unsigned)pairs), dim3(gd::SV_WG), 0,
                       c->stream, j);
    HIPCHK(c, hipGetLastError());
    std::vector<double> V(N * N), w;             // G is symmetric to the bit: row-major is gd_eigh.hpp's column-major
    HIPCHK(c, hipMemcpyAsync(V.data(), d_gram.get(), N * N * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->sv_secs[1] = ing_now() - t1;

    // the spectrum, descending, and the cut (debiaser.go:185-191, capped at what there is)
    const double t2 = ing_now();
    if (gde::sym_eigen(N, V, w) != 0) return fail(c, GD_E_INVALID, "svd debias: the eigenvalues of the Gram matrix did not converge");
    std::vector<uint32_t> order(N);
    for (size_t i = 0; i < N; ++i) order[i] = (uint32_t)i;
    std::stable_sort(order.begin(), order.end(), [&w](uint32_t a, uint32_t b) { return w[a] > w[b]; });
    const size_t L = std::min(n_rows, N);
    std::vector<double> sv(L);
    double sum = 0;
    for (size_t i = 0; i < L; ++i) { sv[i] = std::sqrt(std::max(w[order[i]], 0.0)); sum += sv[i]; }
    const size_t cap = std::min<size_t>((size_t)gd::SV_MAX_K, L);
    size_t n = 0;
    while (n < cap && 100.0 * sv[n] / sum > pct) ++n;
    std::vector<double> vt(std::max<size_t>(n, 1) * N);
    for (size_t k = 0; k < n; ++k) std::copy(&V[(size_t)order[k] * N], &V[(size_t)order[k] * N] + N, &vt[k * N]);
    c->sv_secs[2] = ing_now() - t2;

    const double t3 = ing_now();
    if (n) HIPCHK(c, hipMemcpyAsync(d_vt.get(), vt.data(), n * N * sizeof(double), hipMemcpyHostToDevice, c->stream));
    j.n_removed = (int32_t)n;
    if (log2s) sv_project<gd::SvLog2>(c, j, row_grid);
    else sv_project<gd::SvLinear>(c, j, row_grid);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->sv_secs[3] = ing_now() - t3;
    if (s) std::copy(sv.begin(), sv.end(), s);
    if (n_removed) *n_removed = (int)n;
    if (log2s && centre_cells) mat_keys_to_float(keys, centre_cells);
    return GD_OK;
}

}  // namespace

int gd_svd_debias_scaled(gd_ctx* c, const float* depths, size_t n_rows, int n_samples, double min_variance_pct, int scaler,
                         float* out, double* s, int* n_removed, float* centre_cells)
{
    if (!c) return GD_E_INVALID;
    if (int r = sv_check(c, n_rows, n_samples, min_variance_pct)) return r;
    if (int r = sv_check_scaler(c, scaler)) return r;
    if (!depths || !out) return GD_E_INVALID;
    if (int r = mat_check(c, "svd debias", depths, n_rows, n_samples)) return r;
    if (int r = set_device(c)) return r;
    for (double& t : c->sv_secs) t = 0;
    const size_t bytes = n_rows * (size_t)n_samples * sizeof(float);
    DevBuf d;
    const double t0 = ing_now();
    if (int r = d.alloc(c, bytes)) return r;
    HIPCHK(c, hipMemcpyAsync(d.get(), depths, bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->sv_secs[0] = ing_now() - t0;
    if (int r = sv_run(c, d.as<const float>(), d.as<float>(), n_rows, n_samples, min_variance_pct, scaler, s, n_removed, centre_cells))
        return r;
    const double t4 = ing_now();
    HIPCHK(c, hipMemcpyAsync(out, d.get(), bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->sv_secs[4] = ing_now() - t4;
    return GD_OK;
}

int gd_svd_debias(gd_ctx* c, const float* depths, size_t n_rows, int n_samples, double min_variance_pct, int zscore, float* out,
                  double* s, int* n_removed)
{
    return gd_svd_debias_scaled(c, depths, n_rows, n_samples, min_variance_pct, sv_scaler(zscore), out, s, n_removed, nullptr);
}

int gd_svd_debias_scaled_cells(gd_ctx* c, const int64_t* d_cells, size_t n_rows, int n_samples, double min_variance_pct, int scaler,
                               float* d_out, double* s, int* n_removed, float* centre_cells)
{
    if (!c) return GD_E_INVALID;
    if (int r = sv_check(c, n_rows, n_samples, min_variance_pct)) return r;
    if (int r = sv_check_scaler(c, scaler)) return r;
    if (!d_cells || !d_out) return GD_E_INVALID;
    const size_t cells = n_rows * (size_t)n_samples;
    if (gdm::overlap(d_cells, cells * sizeof(int64_t), d_out, cells * sizeof(float)))
        return fail(c, GD_E_INVALID, "svd debias: the result would overlap the cells it is made of");
    if (int r = set_device(c)) return r;
    for (double& t : c->sv_secs) t = 0;
    // the conversion into d_out, then the one check of a device matrix: it names a negative cell by row and sample
    const double t0 = ing_now();
    DevBuf negative;
    if (int r = dm_from_cells(c, d_cells, d_out, n_rows, n_samples, negative)) return r;
    if (int r = dm_check(c, "svd debias", d_out, n_rows, n_samples)) return r;
    c->sv_secs[0] = ing_now() - t0;
    return sv_run(c, d_out, d_out, n_rows, n_samples, min_variance_pct, scaler, s, n_removed, centre_cells);
}

int gd_svd_debias_cells(gd_ctx* c, const int64_t* d_cells, size_t n_rows, int n_samples, double min_variance_pct, int zscore,
                        float* d_out, double* s, int* n_removed)
{
    return gd_svd_debias_scaled_cells(c, d_cells, n_rows, n_samples, min_variance_pct, sv_scaler(zscore), d_out, s, n_removed, nullptr);
}

int gd_svd_debias_scaled_device(gd_ctx* c, const float* d_depths, size_t n_rows, int n_samples, double min_variance_pct, int scaler,
                                float* d_out, double* s, int* n_removed, float* centre_cells)
{
    if (!c) return GD_E_INVALID;
    if (int r = sv_check(c, n_rows, n_samples, min_variance_pct)) return r;
    if (int r = sv_check_scaler(c, scaler)) return r;
    if (!d_depths || !d_out) return GD_E_INVALID;
    const size_t bytes = n_rows * (size_t)n_samples * sizeof(float);
    if (d_out != d_depths && gdm::overlap(d_depths, bytes, d_out, bytes))
        return fail(c, GD_E_INVALID, "svd debias: the result may be the matrix itself, not a part of it");
    if (int r = set_device(c)) return r;
    for (double& t : c->sv_secs) t = 0;
    const double t0 = ing_now();
    if (int r = dm_check(c, "svd debias", d_depths, n_rows, n_samples)) return r;
    c->sv_secs[0] = ing_now() - t0;
    return sv_run(c, d_depths, d_out, n_rows, n_samples, min_variance_pct, scaler, s, n_removed, centre_cells);
}

int gd_svd_debias_device(gd_ctx* c, const float* d_depths, size_t n_rows, int n_samples, double min_variance_pct, int zscore,
                         float* d_out, double* s, int* n_removed)
{
    return gd_svd_debias_scaled_device(c, d_depths, n_rows, n_samples, min_variance_pct, sv_scaler(zscore), d_out, s, n_removed, nullptr);
}

int gd_svd_debias_timing(gd_ctx* c, double* out, size_t n)
{
    if (!c || !out) return GD_E_INVALID;
    for (size_t i = 0; i < n && i < 5; ++i) out[i] = c->sv_secs[i];
    return GD_OK;
}
