// gd_api_indexsplit.inc -- the cohort sum of `goleft indexsplit` on the device: begin (the cell vector, zeroed), add a
// batch of samples (as often as needed), read the sums back (part of gd_api.hip, inside extern "C").  The kernel is
// gd_indexsplit.hpp's.

namespace {

struct IsState {
    int32_t R = 0;
    int64_t n_cells = 0;
    std::vector<int32_t> longest;
    int32_t most = 0;                          // the largest of longest
    DevArr<int32_t> d_longest;
    DevArr<int64_t> d_cell_off;
    DevArr<double> d_sums;
    double secs[3] = {0, 0, 0};                // upload, kernel, read-back: summed over the calls since begin
};

constexpr int32_t kIsMaxTiles = 1 << 24;       // per reference (a .bai ends at 2^29 bases: 32 768 tiles)

}  // namespace

int gd_indexsplit_begin(gd_ctx* c, int32_t n_refs, const int32_t* longest)
{
    if (!c || !longest) return GD_E_INVALID;
    if (int r = set_device(c)) return r;
    drop_state(c, c->isp);
    if (n_refs < 1 || n_refs > (1 << 20)) return fail(c, GD_E_RANGE, "indexsplit: 1 .. 2^20 references, not %d", n_refs);
    const size_t R = (size_t)n_refs;
    std::vector<int64_t> cell_off(R);
    int64_t cells = 0;
    int32_t most = 0;
    for (size_t r = 0; r < R; ++r) {
        if (longest[r] < 0 || longest[r] > kIsMaxTiles)
            return fail(c, GD_E_RANGE, "indexsplit: reference %zu has %d tiles (0 .. 2^24)", r, longest[r]);
        cell_off[r] = cells;
        cells += longest[r];
        most = std::max(most, longest[r]);
    }
    c->isp.reset(new (std::nothrow) IsState());
    if (!c->isp) return GD_E_NOMEM;
    IsState& s = *c->isp;
    // a failure below leaves no half-built state behind
    auto body = [&]() -> int {
        s.R = n_refs; s.n_cells = cells; s.most = most;
        s.longest.assign(longest, longest + R);
        HIPCHK(c, s.d_longest.alloc(R));
        HIPCHK(c, s.d_cell_off.alloc(R));
        HIPCHK(c, s.d_sums.alloc((size_t)cells));
        HIPCHK(c, hipMemcpyAsync(s.d_longest, s.longest.data(), R * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(s.d_cell_off, cell_off.data(), R * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemsetAsync(s.d_sums, 0, std::max<size_t>((size_t)cells, 1) * sizeof(double), c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));      // (cell_off is read by the copy until here)
        return GD_OK;
    };
    const int rc = body();
    if (rc != GD_OK) drop_state(c, c->isp);
    return rc;
}

#define IS_STATE(c)                                                                                       \
    if (!(c)) return GD_E_INVALID;                                                                        \
    if (!(c)->isp) return fail((c), GD_E_STATE, "gd_indexsplit_begin has not been called");               \
    if (int r_ = set_device(c)) return r_;                                                                \
    IsState& s = *(c)->isp

int gd_indexsplit_add(gd_ctx* c, int32_t n_samples, const int64_t* sample_off, const int64_t* sizes, const int64_t* tile_off,
                      const int32_t* tile_cnt)
{
    IS_STATE(c);
    if (!sample_off || !tile_off || !tile_cnt) return GD_E_INVALID;
    if (n_samples < 1 || n_samples > 65535) return fail(c, GD_E_RANGE, "indexsplit: 1 .. 65535 samples in a batch, not %d", n_samples);
    const size_t N = (size_t)n_samples, R = (size_t)s.R;
    // everything is checked before anything is added: a refused batch leaves the sums as they were
    if (sample_off[0] != 0) return fail(c, GD_E_INVALID, "indexsplit: sample_off must start at 0");
    for (size_t k = 0; k < N; ++k) {
        if (sample_off[k + 1] < sample_off[k]) return fail(c, GD_E_INVALID, "indexsplit: sample_off decreases at sample %zu", k);
        for (size_t r = 0; r < R; ++r) {
            const int64_t o = tile_off[k * R + r], n = tile_cnt[k * R + r];
            if (n < 0 || o < sample_off[k] || o + n > sample_off[k + 1])
                return fail(c, GD_E_RANGE, "indexsplit: the tiles of sample %zu, reference %zu are outside the sample", k, r);
            if (n > s.longest[r])
                return fail(c, GD_E_RANGE, "indexsplit: sample %zu has %lld tiles on reference %zu, gd_indexsplit_begin was told %d",
                            k, (long long)n, r, s.longest[r]);
        }
    }
    const int64_t T = sample_off[N];
    if (T > 0 && !sizes) return GD_E_INVALID;
    for (int64_t i = 0; i < T; ++i)
        if (sizes[i] < 0) return fail(c, GD_E_INVALID, "indexsplit: negative tile size at %lld", (long long)i);
    if (T == 0 || s.n_cells == 0) return GD_OK;
    const double t0 = ing_now();
    DevBuf d_sizes, d_tile_off, d_tile_cnt;              // the device copies of the batch
    if (int r = d_sizes.alloc(c, (size_t)T * sizeof(int64_t))) return r;
    if (int r = d_tile_off.alloc(c, N * R * sizeof(int64_t))) return r;
    if (int r = d_tile_cnt.alloc(c, N * R * sizeof(int32_t))) return r;
    HIPCHK(c, hipMemcpyAsync(d_sizes, sizes, (size_t)T * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_tile_off, tile_off, N * R * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_tile_cnt, tile_cnt, N * R * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const double t1 = ing_now();
    gd::IsJob j{};
    j.n_samples = n_samples; j.n_refs = s.R;
    j.sizes = d_sizes.as<int64_t>(); j.tile_off = d_tile_off.as<int64_t>(); j.tile_cnt = d_tile_cnt.as<int32_t>();
    j.longest = s.d_longest; j.cell_off = s.d_cell_off; j.sums = s.d_sums;
    const unsigned gx = (unsigned)std::min<int64_t>(((int64_t)s.most + gd::IS_WG - 1) / gd::IS_WG, 1024);
    const unsigned gy = (unsigned)std::min<size_t>(R, 65535);
    hipLaunchKernelGGL(gd::gd_is_sum_kernel, dim3(gx, gy), dim3(gd::IS_WG), 0, c->stream, j);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));          // (the batch's buffers are freed on return)
    s.secs[0] += t1 - t0;
    s.secs[1] += ing_now() - t1;
    return GD_OK;
}

int gd_indexsplit_sums(gd_ctx* c, double* out, size_t cap)
{
    IS_STATE(c);
    if (cap < (size_t)s.n_cells) return fail(c, GD_E_CAPACITY, "%lld cells, room for %zu", (long long)s.n_cells, cap);
    if (s.n_cells == 0) return GD_OK;
    if (!out) return GD_E_INVALID;
    const double t0 = ing_now();
    HIPCHK(c, hipMemcpyAsync(out, s.d_sums, (size_t)s.n_cells * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    s.secs[2] += ing_now() - t0;
    return GD_OK;
}

int gd_indexsplit_timing(gd_ctx* c, double* out, size_t n)
{
    IS_STATE(c);
    if (!out) return GD_E_INVALID;
    for (size_t i = 0; i < n && i < 3; ++i) out[i] = s.secs[i];
    return GD_OK;
}
