// gd_api_devmat.inc -- a depth matrix that stays in HBM between its consumers (part of gd_api.hip, inside extern "C";
// before gd_api_emdepth.inc: the files after it use the checks of a depth matrix that are here, on the host -- mat_* over
// gd_matcheck.hpp -- and on the device -- dm_*; DESIGN.md section 3.14).  The kernels are gd_devmat.hpp's.  Nothing is kept
// between calls.

namespace {

static void dm_grids(size_t n_rows, int n_samples, dim3* grid, dim3* wg)
{
    const unsigned tiles = (unsigned)(((size_t)n_samples + gd::DM_COLS - 1) / gd::DM_COLS);
    const size_t turns = (n_rows + gd::DM_WAVES - 1) / gd::DM_WAVES;
    *grid = dim3((unsigned)std::max<size_t>(1, std::min<size_t>(turns, (size_t)gd::DM_MAX_GRID)), tiles);
    *wg = dim3(gd::DM_WG);
}

// ---- the checks every consumer of a depth matrix shares (gd_matcheck.hpp), in the caller's name ----

// GD_E_INVALID naming cell `first` of a matrix of n_samples columns, unless there is none (gdm::kNone)
static int mat_refuse_cell(gd_ctx* c, const char* who, size_t first, int n_samples)
{
    if (first == gdm::kNone) return GD_OK;
    return fail(c, GD_E_INVALID, "%s: the depth of row %zu, sample %zu is not a finite number >= 0", who, first / (size_t)n_samples,
                first % (size_t)n_samples);
}

// a host float32 matrix: every cell finite and >= 0
static int mat_check(gd_ctx* c, const char* who, const float* depths, size_t n_rows, int n_samples)
{
    return mat_refuse_cell(c, who, gdm::first_bad(depths, n_rows * (size_t)n_samples), n_samples);
}

// the per-sample scales: every one finite and >= 0
static int mat_check_scale(gd_ctx* c, const char* who, const float* scale, int n_samples)
{
    const size_t s = gdm::first_bad(scale, (size_t)n_samples);
    if (s == gdm::kNone) return GD_OK;
    return fail(c, GD_E_INVALID, "%s: the scale of sample %zu is not a finite number >= 0", who, s);
}

// the answers of the median kernels, a float's bits in a key's low word
static void mat_keys_to_float(const std::vector<uint64_t>& keys, float* med)
{
    for (size_t s = 0; s < keys.size(); ++s) {
        const uint32_t bits = (uint32_t)keys[s];
        memcpy(&med[s], &bits, sizeof bits);
    }
}

// d_out = (float)d_cells, enqueued on the context's stream; the device word this call allocates into `flag` and zeroes
// becomes 1 when a cell is negative.  Nothing is waited for.
static int dm_from_cells(gd_ctx* c, const int64_t* d_cells, float* d_out, size_t n_rows, int n_samples, DevBuf& flag)
{
    if (int r = flag.alloc(c, sizeof(uint32_t))) return r;
    HIPCHK(c, hipMemsetAsync(flag.get(), 0, sizeof(uint32_t), c->stream));
    gd::DmJob j{};
    j.cells = d_cells; j.depths = d_out; j.n_rows = (int64_t)n_rows; j.n = n_samples; j.flag = flag.as<uint32_t>();
    dim3 grid, wg;
    dm_grids(n_rows, n_samples, &grid, &wg);
    hipLaunchKernelGGL(gd::gd_devmat_from_cells_kernel, grid, wg, 0, c->stream, j);
    HIPCHK(c, hipGetLastError());
    return GD_OK;
}

// dm_from_cells' verdict, waited for: GD_E_INVALID when a cell was negative
static int dm_refuse_negative(gd_ctx* c, const char* who, const DevBuf& flag)
{
    uint32_t negative = 0;
    HIPCHK(c, hipMemcpyAsync(&negative, flag.get(), sizeof negative, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (negative) return fail(c, GD_E_INVALID, "%s: a cell of the device matrix is negative", who);
    return GD_OK;
}

// mat_check for a matrix on the device.  Runs the check kernel and waits for it; n_rows >= 1.
static int dm_check(gd_ctx* c, const char* who, const float* d_depths, size_t n_rows, int n_samples)
{
    DevBuf w;
    if (int r = w.alloc(c, sizeof(unsigned long long))) return r;
    HIPCHK(c, hipMemsetAsync(w.get(), 0xff, sizeof(unsigned long long), c->stream));
    gd::DmJob j{};
    j.depths = const_cast<float*>(d_depths); j.n_rows = (int64_t)n_rows; j.n = n_samples;
    j.first = w.as<unsigned long long>();
    dim3 grid, wg;
    dm_grids(n_rows, n_samples, &grid, &wg);
    hipLaunchKernelGGL(gd::gd_devmat_check_kernel, grid, wg, 0, c->stream, j);
    HIPCHK(c, hipGetLastError());
    unsigned long long first = 0;
    HIPCHK(c, hipMemcpyAsync(&first, w.get(), sizeof first, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    static_assert(sizeof(size_t) == sizeof first, "the kernel's `none` is gdm::kNone");
    return mat_refuse_cell(c, who, (size_t)first, n_samples);
}

}  // namespace

int gd_device_scale(gd_ctx* c, float* d_depths, size_t n_rows, int n_samples, const float* scale)
{
    if (!c) return GD_E_INVALID;
    if (n_samples < 1 || n_samples > gd::DM_MAX_N)
        return fail(c, GD_E_RANGE, "device scale: 1 .. %d samples, not %d", gd::DM_MAX_N, n_samples);
    if (!scale) return GD_E_INVALID;
    if (int r = mat_check_scale(c, "device scale", scale, n_samples)) return r;
    if (n_rows == 0) return GD_OK;
    if (!d_depths) return GD_E_INVALID;
    if (int r = set_device(c)) return r;
    const size_t N = (size_t)n_samples;
    DevBuf f;
    if (int r = f.alloc(c, N * sizeof(float))) return r;
    HIPCHK(c, hipMemcpyAsync(f.get(), scale, N * sizeof(float), hipMemcpyHostToDevice, c->stream));
    gd::DmJob j{};
    j.depths = d_depths; j.scale = f.as<const float>(); j.n_rows = (int64_t)n_rows; j.n = n_samples;
    dim3 grid, wg;
    dm_grids(n_rows, n_samples, &grid, &wg);
    hipLaunchKernelGGL(gd::gd_devmat_scale_kernel, grid, wg, 0, c->stream, j);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return GD_OK;
}
