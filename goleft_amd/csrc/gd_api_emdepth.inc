// gd_api_emdepth.inc -- emdepth.EMDepth per row of a depth matrix (part of gd_api.hip, inside extern "C"): the host
// float32 form, the device int64 form (the cells gd_depthwed_device leaves) and the seconds of the last call.  The kernel
// is gd_emdepth.hpp's.  Nothing is kept between calls but the three timings.

namespace {

static int em_check_n(gd_ctx* c, int n_samples)
{
    if (n_samples == 2)
        return fail(c, GD_E_RANGE, "emdepth: 2 samples: the reference's median of an even row reads b[N/2 + 1], which two values do not have");
    if (n_samples < 1 || n_samples > gd::EM_MAX_N)
        return fail(c, GD_E_RANGE, "emdepth: 1 or 3 .. %d samples, not %d", gd::EM_MAX_N, n_samples);
    return GD_OK;
}

// (the largest array of a call: nine centres a row in float64, or a value a sample)
static int em_check_fit(gd_ctx* c, const char* who, size_t n_rows, int n_samples)
{
    if (gdm::fits(n_rows, (size_t)n_samples, gd::EM_CENTRES)) return GD_OK;
    return fail(c, GD_E_RANGE, "%s: %zu rows of %d samples do not fit an allocation", who, n_rows, n_samples);
}

// the kernel on rows already on the device (float32 when !cells, int64 otherwise); every output is a device pointer or
// nullptr.  Returns once the stream has run it; *secs is its wall time.
static int em_launch(gd_ctx* c, bool cells, const void* d_in, const float* d_scale, size_t n_rows, int n_samples,
                     double* d_lambda, uint8_t* d_iters, uint8_t* d_cn, float* d_log2fc, double* secs)
{
    gd::EmJob j{};
    j.cells = d_in; j.scale = d_scale; j.n_rows = (int64_t)n_rows; j.n = n_samples;
    // the initial centres' factors (:136), from the host's libm as the oracle's are
    for (int i = 0; i < gd::EM_CENTRES; ++i) j.pw[i] = std::pow((double)i / 2.0, 1.1);
    j.lambda = d_lambda; j.iters = d_iters; j.cn = d_cn; j.log2fc = d_log2fc;
    const unsigned grid = (unsigned)std::min<size_t>((n_rows + gd::EM_WAVES - 1) / gd::EM_WAVES, (size_t)gd::EM_MAX_GRID);
    const dim3 wg(gd::EM_WAVES * 64);
    const bool regs = n_samples <= gd::EM_REG_MAX;
    const double t0 = ing_now();
    if (cells) {
        if (regs) hipLaunchKernelGGL((gd::gd_emdepth_kernel<int64_t, true>), dim3(grid), wg, 0, c->stream, j);
        else hipLaunchKernelGGL((gd::gd_emdepth_kernel<int64_t, false>), dim3(grid), wg, 0, c->stream, j);
    } else {
        if (regs) hipLaunchKernelGGL((gd::gd_emdepth_kernel<float, true>), dim3(grid), wg, 0, c->stream, j);
        else hipLaunchKernelGGL((gd::gd_emdepth_kernel<float, false>), dim3(grid), wg, 0, c->stream, j);
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *secs = ing_now() - t0;
    return GD_OK;
}

// d_in: the rows on the device (float32 when !cells, int64 otherwise); d_scale: device or nullptr
static int em_run(gd_ctx* c, bool cells, const void* d_in, const float* d_scale, size_t n_rows, int n_samples,
                  double* lambda, uint8_t* iters, uint8_t* cn, float* log2fc)
{
    const size_t N = (size_t)n_samples, cellsN = n_rows * N;
    DevBuf b_lambda, b_iters, b_cn, b_fc;
    if (lambda) if (int r = b_lambda.alloc(c, n_rows * gd::EM_CENTRES * sizeof(double))) return r;
    if (iters) if (int r = b_iters.alloc(c, n_rows)) return r;
    if (cn) if (int r = b_cn.alloc(c, cellsN)) return r;
    if (log2fc) if (int r = b_fc.alloc(c, cellsN * sizeof(float))) return r;
    if (int r = em_launch(c, cells, d_in, d_scale, n_rows, n_samples, b_lambda.as<double>(), b_iters.as<uint8_t>(),
                          b_cn.as<uint8_t>(), b_fc.as<float>(), &c->em_secs[1]))
        return r;
    const double t1 = ing_now();
    if (lambda) HIPCHK(c, hipMemcpyAsync(lambda, b_lambda.get(), n_rows * gd::EM_CENTRES * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (iters) HIPCHK(c, hipMemcpyAsync(iters, b_iters.get(), n_rows, hipMemcpyDeviceToHost, c->stream));
    if (cn) HIPCHK(c, hipMemcpyAsync(cn, b_cn.get(), cellsN, hipMemcpyDeviceToHost, c->stream));
    if (log2fc) HIPCHK(c, hipMemcpyAsync(log2fc, b_fc.get(), cellsN * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->em_secs[2] = ing_now() - t1;
    return GD_OK;
}

}  // namespace

int gd_emdepth(gd_ctx* c, const float* depths, size_t n_rows, int n_samples, double* lambda, uint8_t* iters, uint8_t* cn,
               float* log2fc)
{
    if (!c) return GD_E_INVALID;
    if (int r = em_check_n(c, n_samples)) return r;
    if (n_rows == 0) return GD_OK;
    if (!depths) return GD_E_INVALID;
    if (int r = em_check_fit(c, "emdepth", n_rows, n_samples)) return r;
    if (int r = mat_check(c, "emdepth", depths, n_rows, n_samples)) return r;
    if (int r = set_device(c)) return r;
    c->em_secs[0] = c->em_secs[1] = c->em_secs[2] = 0;
    const size_t bytes = n_rows * (size_t)n_samples * sizeof(float);
    DevBuf in;
    const double t0 = ing_now();
    if (int r = in.alloc(c, bytes)) return r;
    HIPCHK(c, hipMemcpyAsync(in.get(), depths, bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->em_secs[0] = ing_now() - t0;
    return em_run(c, false, in.get(), nullptr, n_rows, n_samples, lambda, iters, cn, log2fc);
}

int gd_emdepth_cells(gd_ctx* c, const int64_t* d_cells, size_t n_rows, int n_samples, const float* scale, double* lambda,
                     uint8_t* iters, uint8_t* cn, float* log2fc)
{
    if (!c) return GD_E_INVALID;
    if (int r = em_check_n(c, n_samples)) return r;
    if (scale) if (int r = mat_check_scale(c, "emdepth", scale, n_samples)) return r;
    if (n_rows == 0) return GD_OK;
    if (!d_cells) return GD_E_INVALID;
    if (int r = em_check_fit(c, "emdepth", n_rows, n_samples)) return r;
    if (int r = set_device(c)) return r;
    c->em_secs[0] = c->em_secs[1] = c->em_secs[2] = 0;
    DevBuf d_scale;
    if (scale) {
        const double t0 = ing_now();
        if (int r = d_scale.alloc(c, (size_t)n_samples * sizeof(float))) return r;
        HIPCHK(c, hipMemcpyAsync(d_scale.get(), scale, (size_t)n_samples * sizeof(float), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        c->em_secs[0] = ing_now() - t0;
    }
    return em_run(c, true, d_cells, d_scale.as<float>(), n_rows, n_samples, lambda, iters, cn, log2fc);
}

// gd_emdepth for a float32 matrix that is in HBM already: gd_devmat.hpp's check in place of the host's, no upload
int gd_emdepth_device(gd_ctx* c, const float* d_depths, size_t n_rows, int n_samples, double* lambda, uint8_t* iters,
                      uint8_t* cn, float* log2fc)
{
    if (!c) return GD_E_INVALID;
    if (int r = em_check_n(c, n_samples)) return r;
    if (n_rows == 0) return GD_OK;
    if (!d_depths) return GD_E_INVALID;
    if (int r = em_check_fit(c, "emdepth", n_rows, n_samples)) return r;
    if (int r = set_device(c)) return r;
    if (int r = dm_check(c, "emdepth", d_depths, n_rows, n_samples)) return r;
    c->em_secs[0] = c->em_secs[1] = c->em_secs[2] = 0;
    return em_run(c, false, d_depths, nullptr, n_rows, n_samples, lambda, iters, cn, log2fc);
}

int gd_emdepth_timing(gd_ctx* c, double* out, size_t n)
{
    if (!c || !out) return GD_E_INVALID;
    for (size_t i = 0; i < n && i < 3; ++i) out[i] = c->em_secs[i];
    return GD_OK;
}
