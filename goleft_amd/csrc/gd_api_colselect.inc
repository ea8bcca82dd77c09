// gd_api_colselect.inc -- dcnv's SampleMedians per column of a depth matrix (part of gd_api.hip, inside extern "C"): the
// host float32 form, the device int64 form (the cells gd_depthwed_device leaves) and the seconds of the last call.  The
// kernels are gd_colselect.hpp's.  Nothing is kept between calls but the three timings.

namespace {

static int cs_check(gd_ctx* c, size_t n_rows, int n_samples)
{
    if (n_samples < 1 || n_samples > gd::CS_MAX_N)
        return fail(c, GD_E_RANGE, "sample medians: 1 .. %d samples, not %d", gd::CS_MAX_N, n_samples);
    if (n_rows < 1 || n_rows > 0x7fffffffull)
        return fail(c, GD_E_RANGE, "sample medians: 1 .. 2^31 - 1 rows, not %zu", n_rows);
    return GD_OK;
}

// d_in: the matrix on the device (float32 when !cells, int64 otherwise).  prefix_out: host [n_samples], the answers as
// keys (a float's bits or the cell); nonzero_out: host [n_samples] or nullptr.  mid (float32 only): the rank is rows / 2
// over all cells, the centre of dcnv's Log2 scaler, in place of SampleMedians'; d_prefix_out: device [n_samples] or nullptr,
// the keys once more, for the kernels that follow on the stream.
static int cs_run(gd_ctx* c, bool cells, const void* d_in, size_t n_rows, int n_samples, uint64_t* prefix_out,
                  uint64_t* nonzero_out, bool mid = false, uint64_t* d_prefix_out = nullptr)
{
    const size_t N = (size_t)n_samples;
    DevBuf counts, zeros, prefix, rem, rank, nonzero, flags;
    if (int r = counts.alloc(c, N * gd::CS_BINS * sizeof(uint32_t))) return r;
    if (int r = zeros.alloc(c, N * sizeof(uint32_t))) return r;
    if (int r = prefix.alloc(c, N * sizeof(uint64_t))) return r;
    if (int r = rem.alloc(c, N * sizeof(int32_t))) return r;
    if (int r = rank.alloc(c, N * sizeof(uint32_t))) return r;
    if (int r = nonzero.alloc(c, N * sizeof(uint64_t))) return r;
    if (int r = flags.alloc(c, 2 * sizeof(uint32_t))) return r;
    const double t0 = ing_now();
    HIPCHK(c, hipMemsetAsync(counts.get(), 0, N * gd::CS_BINS * sizeof(uint32_t), c->stream));
    HIPCHK(c, hipMemsetAsync(zeros.get(), 0, N * sizeof(uint32_t), c->stream));
    HIPCHK(c, hipMemsetAsync(flags.get(), 0, 2 * sizeof(uint32_t), c->stream));
    gd::CsJob j{};
    j.cells = d_in; j.n_rows = (int64_t)n_rows; j.n = n_samples;
    j.counts = counts.as<uint32_t>(); j.zeros = zeros.as<uint32_t>(); j.prefix = prefix.as<uint64_t>(); j.rem = rem.as<int32_t>();
    j.rank = rank.as<uint32_t>(); j.nonzero = nonzero.as<uint64_t>(); j.flags = flags.as<uint32_t>();
    // the column tiles share CS_MAX_GRID workgroups; each strides over the slabs of rows
    const unsigned tiles = (unsigned)((N + gd::CS_COLS - 1) / gd::CS_COLS);
    const size_t slabs = (n_rows + gd::CS_SLAB - 1) / gd::CS_SLAB;
    const unsigned gx = (unsigned)std::min<size_t>(slabs, std::max<unsigned>(1u, (unsigned)gd::CS_MAX_GRID / tiles));
    const dim3 grid(gx, tiles), wg(gd::CS_WG);
    const dim3 pgrid((unsigned)((N + gd::CS_PICK_WAVES - 1) / gd::CS_PICK_WAVES)), pwg(gd::CS_PICK_WAVES * 64);
    int passes = 3;                              // float: the digits after the first
    if (cells) {
        hipLaunchKernelGGL((gd::gd_colselect_hist_kernel<int64_t, true>), grid, wg, 0, c->stream, j);
        hipLaunchKernelGGL((gd::gd_colselect_pick_kernel<gd::CS_PICK_LENGTH>), pgrid, pwg, 0, c->stream, j);
        HIPCHK(c, hipGetLastError());
        uint32_t seen[2] = {0, 0};
        HIPCHK(c, hipMemcpyAsync(seen, flags.get(), sizeof seen, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (seen[1]) return fail(c, GD_E_INVALID, "sample medians: a cell of the device matrix is negative");
        passes = (int)seen[0];                  // the longest answer, in bytes
    } else {
        hipLaunchKernelGGL((gd::gd_colselect_hist_kernel<float, true>), grid, wg, 0, c->stream, j);
        if (mid) hipLaunchKernelGGL(gd::gd_colmid_pick_kernel, pgrid, pwg, 0, c->stream, j);
        else hipLaunchKernelGGL((gd::gd_colselect_pick_kernel<gd::CS_PICK_FLOAT_FIRST>), pgrid, pwg, 0, c->stream, j);
    }
    for (int p = 0; p < passes; ++p) {
        if (cells) hipLaunchKernelGGL((gd::gd_colselect_hist_kernel<int64_t, false>), grid, wg, 0, c->stream, j);
        else hipLaunchKernelGGL((gd::gd_colselect_hist_kernel<float, false>), grid, wg, 0, c->stream, j);
        hipLaunchKernelGGL((gd::gd_colselect_pick_kernel<gd::CS_PICK_DIGIT>), pgrid, pwg, 0, c->stream, j);
    }
    HIPCHK(c, hipGetLastError());
    if (d_prefix_out) HIPCHK(c, hipMemcpyAsync(d_prefix_out, prefix.get(), N * sizeof(uint64_t), hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->sm_secs[1] = ing_now() - t0;
    c->sm_passes = 1 + passes;
    const double t1 = ing_now();
    HIPCHK(c, hipMemcpyAsync(prefix_out, prefix.get(), N * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    if (nonzero_out) HIPCHK(c, hipMemcpyAsync(nonzero_out, nonzero.get(), N * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->sm_secs[2] = ing_now() - t1;
    return GD_OK;
}

}  // namespace

int gd_sample_medians(gd_ctx* c, const float* depths, size_t n_rows, int n_samples, float* med, uint64_t* n_nonzero)
{
    if (!c) return GD_E_INVALID;
    if (int r = cs_check(c, n_rows, n_samples)) return r;
    if (!depths || !med) return GD_E_INVALID;
    if (int r = mat_check(c, "sample medians", depths, n_rows, n_samples)) return r;
    if (int r = set_device(c)) return r;
    c->sm_secs[0] = c->sm_secs[1] = c->sm_secs[2] = 0;
    c->sm_passes = 0;
    const size_t bytes = n_rows * (size_t)n_samples * sizeof(float);
    DevBuf in;
    const double t0 = ing_now();
    if (int r = in.alloc(c, bytes)) return r;
    HIPCHK(c, hipMemcpyAsync(in.get(), depths, bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->sm_secs[0] = ing_now() - t0;
    std::vector<uint64_t> keys((size_t)n_samples);
    if (int r = cs_run(c, false, in.get(), n_rows, n_samples, keys.data(), n_nonzero)) return r;
    mat_keys_to_float(keys, med);
    return GD_OK;
}

int gd_sample_medians_cells(gd_ctx* c, const int64_t* d_cells, size_t n_rows, int n_samples, int64_t* med, uint64_t* n_nonzero)
{
    if (!c) return GD_E_INVALID;
    if (int r = cs_check(c, n_rows, n_samples)) return r;
    if (!d_cells || !med) return GD_E_INVALID;
    if (int r = set_device(c)) return r;
    c->sm_secs[0] = c->sm_secs[1] = c->sm_secs[2] = 0;
    c->sm_passes = 0;
    std::vector<uint64_t> keys((size_t)n_samples);
    if (int r = cs_run(c, true, d_cells, n_rows, n_samples, keys.data(), n_nonzero)) return r;
    for (size_t s = 0; s < keys.size(); ++s) med[s] = (int64_t)keys[s];
    return GD_OK;
}

// gd_sample_medians for a float32 matrix that is in HBM already: gd_devmat.hpp's check in place of the host's, no upload
int gd_sample_medians_device(gd_ctx* c, const float* d_depths, size_t n_rows, int n_samples, float* med, uint64_t* n_nonzero)
{
    if (!c) return GD_E_INVALID;
    if (int r = cs_check(c, n_rows, n_samples)) return r;
    if (!d_depths || !med) return GD_E_INVALID;
    if (int r = set_device(c)) return r;
    if (int r = dm_check(c, "sample medians", d_depths, n_rows, n_samples)) return r;
    c->sm_secs[0] = c->sm_secs[1] = c->sm_secs[2] = 0;
    c->sm_passes = 0;
    std::vector<uint64_t> keys((size_t)n_samples);
    if (int r = cs_run(c, false, d_depths, n_rows, n_samples, keys.data(), n_nonzero)) return r;
    mat_keys_to_float(keys, med);
    return GD_OK;
}

int gd_sample_medians_timing(gd_ctx* c, double* out, size_t n)
{
    if (!c || !out) return GD_E_INVALID;
    for (size_t i = 0; i < n && i < 3; ++i) out[i] = c->sm_secs[i];
    if (n > 3) out[3] = (double)c->sm_passes;
    return GD_OK;
}
