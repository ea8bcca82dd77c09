// gd_api_devmat.inc -- a depth matrix that stays in HBM between its consumers (part of gd_api.hip, inside extern "C";
// before gd_api_emdepth.inc: the *_device entries of the files after it use dm_check, gd_chunk_debias_cells uses
// dm_from_cells; DESIGN.md section 3.14).  The kernels are gd_devmat.hpp's.  Nothing is kept between calls.

namespace {

// a small device buffer of one call (the word a kernel reports through, the factors), freed when the call returns
struct DmWord {
    void* p = nullptr;
    ~DmWord() { if (p) (void)hipFree(p); }
};

static void dm_grids(size_t n_rows, int n_samples, dim3* grid, dim3* wg)
{
    const unsigned tiles = (unsigned)(((size_t)n_samples + gd::DM_COLS - 1) / gd::DM_COLS);
    const size_t turns = (n_rows + gd::DM_WAVES - 1) / gd::DM_WAVES;
    *grid = dim3((unsigned)std::max<size_t>(1, std::min<size_t>(turns, (size_t)gd::DM_MAX_GRID)), tiles);
    *wg = dim3(gd::DM_WG);
}

// whether [a, a + na) and [b, b + nb) share a byte
static bool dm_overlap(const void* a, size_t na, const void* b, size_t nb)
{
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

// d_out = (float)d_cells, enqueued on the context's stream; *d_flag (a device word this call allocates into w and zeroes)
// becomes 1 when a cell is negative.  Nothing is waited for.
static int dm_from_cells(gd_ctx* c, const int64_t* d_cells, float* d_out, size_t n_rows, int n_samples, DmWord& w)
{
    HIPCHK(c, hipMalloc(&w.p, sizeof(uint32_t)));
    HIPCHK(c, hipMemsetAsync(w.p, 0, sizeof(uint32_t), c->stream));
    gd::DmJob j{};
    j.cells = d_cells; j.depths = d_out; j.n_rows = (int64_t)n_rows; j.n = n_samples; j.flag = static_cast<uint32_t*>(w.p);
    dim3 grid, wg;
    dm_grids(n_rows, n_samples, &grid, &wg);
    hipLaunchKernelGGL(gd::gd_devmat_from_cells_kernel, grid, wg, 0, c->stream, j);
    HIPCHK(c, hipGetLastError());
    return GD_OK;
}

// A device float32 matrix held to what the host entry points hold theirs to: every cell finite and >= 0.  Runs the check
// kernel and waits for it; GD_E_INVALID names the first cell that is not.  n_rows >= 1.
static int dm_check(gd_ctx* c, const char* who, const float* d_depths, size_t n_rows, int n_samples)
{
    DmWord w;
    HIPCHK(c, hipMalloc(&w.p, sizeof(unsigned long long)));
    HIPCHK(c, hipMemsetAsync(w.p, 0xff, sizeof(unsigned long long), c->stream));
    gd::DmJob j{};
    j.depths = const_cast<float*>(d_depths); j.n_rows = (int64_t)n_rows; j.n = n_samples;
    j.first = static_cast<unsigned long long*>(w.p);
    dim3 grid, wg;
    dm_grids(n_rows, n_samples, &grid, &wg);
    hipLaunchKernelGGL(gd::gd_devmat_check_kernel, grid, wg, 0, c->stream, j);
    HIPCHK(c, hipGetLastError());
    unsigned long long first = 0;
    HIPCHK(c, hipMemcpyAsync(&first, w.p, sizeof first, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (first != ~0ull)
        return fail(c, GD_E_INVALID, "%s: the depth of row %zu, sample %zu is not a finite number >= 0", who,
                    (size_t)(first / (unsigned long long)n_samples), (size_t)(first % (unsigned long long)n_samples));
    return GD_OK;
}

}  // namespace

int gd_device_scale(gd_ctx* c, float* d_depths, size_t n_rows, int n_samples, const float* scale)
{
    if (!c) return GD_E_INVALID;
    if (n_samples < 1 || n_samples > gd::DM_MAX_N)
        return fail(c, GD_E_RANGE, "device scale: 1 .. %d samples, not %d", gd::DM_MAX_N, n_samples);
    if (!scale) return GD_E_INVALID;
    const size_t N = (size_t)n_samples;
    for (size_t s = 0; s < N; ++s)
        if (!(scale[s] >= 0.0f) || !std::isfinite(scale[s]))
            return fail(c, GD_E_INVALID, "device scale: the scale of sample %zu is not a finite number >= 0", s);
    if (n_rows == 0) return GD_OK;
    if (!d_depths) return GD_E_INVALID;
    if (int r = set_device(c)) return r;
    DmWord f;
    HIPCHK(c, hipMalloc(&f.p, N * sizeof(float)));
    HIPCHK(c, hipMemcpyAsync(f.p, scale, N * sizeof(float), hipMemcpyHostToDevice, c->stream));
    gd::DmJob j{};
    j.depths = d_depths; j.scale = static_cast<const float*>(f.p); j.n_rows = (int64_t)n_rows; j.n = n_samples;
    dim3 grid, wg;
    dm_grids(n_rows, n_samples, &grid, &wg);
    hipLaunchKernelGGL(gd::gd_devmat_scale_kernel, grid, wg, 0, c->stream, j);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return GD_OK;
}
