// gd_api_emdepth.inc -- emdepth.EMDepth per row of a depth matrix (part of gd_api.hip, inside extern "C"): the host
// float32 form, the device int64 form (the cells gd_depthwed_device leaves) and the seconds of the last call.  The kernel
// is gd_emdepth.hpp's.  Nothing is kept between calls but the three timings.

namespace {

// the device buffers of one call, freed when it returns
struct EmBufs {
    void* in = nullptr;
    float* scale = nullptr;
    double* lambda = nullptr;
    uint8_t* iters = nullptr;
    uint8_t* cn = nullptr;
    float* log2fc = nullptr;
    ~EmBufs()
    {
        for (void* p : {in, (void*)scale, (void*)lambda, (void*)iters, (void*)cn, (void*)log2fc})
            if (p) (void)hipFree(p);
    }
};

static int em_check_n(gd_ctx* c, int n_samples)
{
    if (n_samples == 2)
        return fail(c, GD_E_RANGE, "emdepth: 2 samples: the reference's median of an even row reads b[N/2 + 1], which two values do not have");
    if (n_samples < 1 || n_samples > gd::EM_MAX_N)
        return fail(c, GD_E_RANGE, "emdepth: 1 or 3 .. %d samples, not %d", gd::EM_MAX_N, n_samples);
    return GD_OK;
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
                  double* lambda, uint8_t* iters, uint8_t* cn, float* log2fc, EmBufs& b)
{
    const size_t N = (size_t)n_samples, cellsN = n_rows * N;
    if (lambda) HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&b.lambda), n_rows * gd::EM_CENTRES * sizeof(double)));
    if (iters) HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&b.iters), n_rows));
    if (cn) HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&b.cn), cellsN));
    if (log2fc) HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&b.log2fc), cellsN * sizeof(float)));
    if (int r = em_launch(c, cells, d_in, d_scale, n_rows, n_samples, b.lambda, b.iters, b.cn, b.log2fc, &c->em_secs[1])) return r;
    const double t1 = ing_now();
    if (lambda) HIPCHK(c, hipMemcpyAsync(lambda, b.lambda, n_rows * gd::EM_CENTRES * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (iters) HIPCHK(c, hipMemcpyAsync(iters, b.iters, n_rows, hipMemcpyDeviceToHost, c->stream));
    if (cn) HIPCHK(c, hipMemcpyAsync(cn, b.cn, cellsN, hipMemcpyDeviceToHost, c->stream));
    if (log2fc) HIPCHK(c, hipMemcpyAsync(log2fc, b.log2fc, cellsN * sizeof(float), hipMemcpyDeviceToHost, c->stream));
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
    const size_t N = (size_t)n_samples;
    if (n_rows > (SIZE_MAX / sizeof(double)) / (N > gd::EM_CENTRES ? N : gd::EM_CENTRES))
        return fail(c, GD_E_RANGE, "emdepth: %zu rows of %d samples do not fit an allocation", n_rows, n_samples);
    for (size_t i = 0; i < n_rows * N; ++i)
        if (!(depths[i] >= 0.0f) || !std::isfinite(depths[i]))
            return fail(c, GD_E_INVALID, "emdepth: the depth of row %zu, sample %zu is not a finite number >= 0", i / N, i % N);
    if (int r = set_device(c)) return r;
    c->em_secs[0] = c->em_secs[1] = c->em_secs[2] = 0;
    EmBufs b;
    const double t0 = ing_now();
    HIPCHK(c, hipMalloc(&b.in, n_rows * N * sizeof(float)));
    HIPCHK(c, hipMemcpyAsync(b.in, depths, n_rows * N * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->em_secs[0] = ing_now() - t0;
    return em_run(c, false, b.in, nullptr, n_rows, n_samples, lambda, iters, cn, log2fc, b);
}

int gd_emdepth_cells(gd_ctx* c, const int64_t* d_cells, size_t n_rows, int n_samples, const float* scale, double* lambda,
                     uint8_t* iters, uint8_t* cn, float* log2fc)
{
    if (!c) return GD_E_INVALID;
    if (int r = em_check_n(c, n_samples)) return r;
    const size_t N = (size_t)n_samples;
    if (scale)
        for (size_t s = 0; s < N; ++s)
            if (!(scale[s] >= 0.0f) || !std::isfinite(scale[s]))
                return fail(c, GD_E_INVALID, "emdepth: the scale of sample %zu is not a finite number >= 0", s);
    if (n_rows == 0) return GD_OK;
    if (!d_cells) return GD_E_INVALID;
    if (n_rows > (SIZE_MAX / sizeof(double)) / (N > gd::EM_CENTRES ? N : gd::EM_CENTRES))
        return fail(c, GD_E_RANGE, "emdepth: %zu rows of %d samples do not fit an allocation", n_rows, n_samples);
    if (int r = set_device(c)) return r;
    c->em_secs[0] = c->em_secs[1] = c->em_secs[2] = 0;
    EmBufs b;
    if (scale) {
        const double t0 = ing_now();
        HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&b.scale), N * sizeof(float)));
        HIPCHK(c, hipMemcpyAsync(b.scale, scale, N * sizeof(float), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        c->em_secs[0] = ing_now() - t0;
    }
    return em_run(c, true, d_cells, b.scale, n_rows, n_samples, lambda, iters, cn, log2fc, b);
}

// gd_emdepth for a float32 matrix that is in HBM already: gd_devmat.hpp's check in place of the host's, no upload
int gd_emdepth_device(gd_ctx* c, const float* d_depths, size_t n_rows, int n_samples, double* lambda, uint8_t* iters,
                      uint8_t* cn, float* log2fc)
{
    if (!c) return GD_E_INVALID;
    if (int r = em_check_n(c, n_samples)) return r;
    if (n_rows == 0) return GD_OK;
    if (!d_depths) return GD_E_INVALID;
    const size_t N = (size_t)n_samples;
    if (n_rows > (SIZE_MAX / sizeof(double)) / (N > gd::EM_CENTRES ? N : gd::EM_CENTRES))
        return fail(c, GD_E_RANGE, "emdepth: %zu rows of %d samples do not fit an allocation", n_rows, n_samples);
    if (int r = set_device(c)) return r;
    if (int r = dm_check(c, "emdepth", d_depths, n_rows, n_samples)) return r;
    c->em_secs[0] = c->em_secs[1] = c->em_secs[2] = 0;
    EmBufs b;
    return em_run(c, false, d_depths, nullptr, n_rows, n_samples, lambda, iters, cn, log2fc, b);
}

int gd_emdepth_timing(gd_ctx* c, double* out, size_t n)
{
    if (!c || !out) return GD_E_INVALID;
    for (size_t i = 0; i < n && i < 3; ++i) out[i] = c->em_secs[i];
    return GD_OK;
}
