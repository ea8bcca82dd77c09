// gd_api_indexcov.inc -- `goleft indexcov` on the device: upload the tile sizes of a cohort (medians and depths follow
// at once), optionally replace the depths (the host's -n pass), compute, read back (part of gd_api.hip, inside
// extern "C").  The kernels are gd_indexcov.hpp's.

namespace {

struct IcState {
    int32_t N = 0, R = 0;
    int64_t n_tiles = 0, n_cells = 0, m = 0, m_pad = 0;
    int32_t n_pad = 0;
    bool computed = false, gram = false;
    std::vector<int64_t> sample_off, tile_off, cell_off, col_off, median;
    std::vector<int32_t> tile_cnt, longest;
    std::vector<uint8_t> is_sex;
    DevList dev;                               // every device allocation: job's arrays and the four below point into it
    gd::IcJob job{};
    long long *d_P = nullptr, *d_G = nullptr, *d_sums = nullptr;
    const int2* d_pairs = nullptr; size_t n_pairs = 0;   // the upper triangle of 32-sample blocks, built once
    bool uploaded = false, buffers = false;      // upload finished; the result buffers of compute exist
    double secs[5] = {0, 0, 0, 0, 0};          // upload, median + depth, cells / slots / counters / pca8, CN, Gram
};

static int ic_alloc_bytes(gd_ctx* c, IcState& s, void** p, size_t bytes)
{
    uint8_t* q = nullptr;
    if (int r = s.dev.alloc(c, &q, bytes)) return r;
    *p = q;
    return GD_OK;
}

static int ic_put_bytes(gd_ctx* c, IcState& s, const void** p, const void* src, size_t bytes)
{
    void* q = nullptr;
    if (int r = ic_alloc_bytes(c, s, &q, bytes)) return r;
    if (bytes) HIPCHK(c, hipMemcpyAsync(q, src, bytes, hipMemcpyHostToDevice, c->stream));
    *p = q;
    return GD_OK;
}

#define ic_alloc(c, s, p, n) ic_alloc_bytes((c), (s), reinterpret_cast<void**>(p), (size_t)(n) * sizeof(**(p)))
#define ic_put(c, s, p, src, n) ic_put_bytes((c), (s), reinterpret_cast<const void**>(p), (src), (size_t)(n) * sizeof(**(p)))

static double ic_now() { return ing_now(); }

}  // namespace

int gd_indexcov_upload(gd_ctx* c, int32_t n_samples, int32_t n_refs, const int64_t* sample_off, const int64_t* sizes,
                       const int64_t* tile_off, const int32_t* tile_cnt, const uint8_t* is_sex)
{
    if (!c || !sample_off || !tile_off || !tile_cnt || !is_sex) return GD_E_INVALID;
    if (n_samples < 1 || n_samples > 65535) return fail(c, GD_E_RANGE, "indexcov: 1 .. 65535 samples, not %d", n_samples);
    if (n_refs < 1 || n_refs > (1 << 20)) return fail(c, GD_E_RANGE, "indexcov: 1 .. 2^20 references, not %d", n_refs);
    const size_t N = (size_t)n_samples, R = (size_t)n_refs;
    if (sample_off[0] != 0) return fail(c, GD_E_INVALID, "indexcov: sample_off must start at 0");
    for (size_t s = 0; s < N; ++s) {
        if (sample_off[s + 1] <= sample_off[s]) return fail(c, GD_E_INVALID, "indexcov: sample %zu has no tiles", s);
        for (size_t r = 0; r < R; ++r) {
            const int64_t o = tile_off[s * R + r], n = tile_cnt[s * R + r];
            if (n < 0 || o < sample_off[s] || o + n > sample_off[s + 1])
                return fail(c, GD_E_RANGE, "indexcov: the tiles of sample %zu, reference %zu are outside the sample", s, r);
        }
    }
    const int64_t T = sample_off[N];
    if (!sizes) return GD_E_INVALID;
    for (int64_t i = 0; i < T; ++i)
        if (sizes[i] < 0) return fail(c, GD_E_INVALID, "indexcov: negative tile size at %lld", (long long)i);
    if (int r = set_device(c)) return r;
    drop_state(c, c->ic);
    c->ic.reset(new (std::nothrow) IcState());
    if (!c->ic) return GD_E_NOMEM;
    IcState& s = *c->ic;
    // a failure below leaves no half-built state behind: the context is as before the first upload
    auto body = [&]() -> int {
    const double t0 = ic_now();
    s.N = n_samples; s.R = n_refs; s.n_tiles = T;
    s.sample_off.assign(sample_off, sample_off + N + 1);
    s.tile_off.assign(tile_off, tile_off + N * R);
    s.tile_cnt.assign(tile_cnt, tile_cnt + N * R);
    s.is_sex.assign(is_sex, is_sex + R);
    gd::IcJob& j = s.job;
    j.n_samples = n_samples; j.n_refs = n_refs;
    if (int r = ic_put(c, s, &j.sizes, sizes, (size_t)T)) return r;
    if (int r = ic_put(c, s, &j.sample_off, s.sample_off.data(), N + 1)) return r;
    if (int r = ic_put(c, s, &j.tile_off, s.tile_off.data(), N * R)) return r;
    if (int r = ic_put(c, s, &j.is_sex, s.is_sex.data(), R)) return r;
    if (int r = ic_alloc(c, s, &j.median, N)) return r;
    if (int r = ic_alloc(c, s, &j.depth, (size_t)T)) return r;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const double t1 = ic_now();
    hipLaunchKernelGGL(gd::gd_ic_median_kernel, dim3((unsigned)N), dim3(gd::IC_WG), 0, c->stream, j);
    int64_t most = 0;
    for (size_t k = 0; k < N; ++k) most = std::max(most, sample_off[k + 1] - sample_off[k]);
    const unsigned gx = (unsigned)std::min<int64_t>((most + gd::IC_WG - 1) / gd::IC_WG, 1024);
    hipLaunchKernelGGL(gd::gd_ic_depth_kernel, dim3(gx, (unsigned)N), dim3(gd::IC_WG), 0, c->stream, j);
    HIPCHK(c, hipGetLastError());
    s.median.resize(N);
    HIPCHK(c, hipMemcpyAsync(s.median.data(), j.median, N * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const double t2 = ic_now();
    // a sample whose median is 0 has no tiles on any reference (NormalizedDepth :140-142)
    for (size_t k = 0; k < N; ++k)
        if (s.median[k] <= 0)
            for (size_t r = 0; r < R; ++r) s.tile_cnt[k * R + r] = 0;
    s.longest.assign(R, 0);
    s.cell_off.assign(R, 0);
    s.col_off.assign(R, 0);
    int64_t cells = 0, cols = 0;
    for (size_t r = 0; r < R; ++r) {
        for (size_t k = 0; k < N; ++k) s.longest[r] = std::max(s.longest[r], s.tile_cnt[k * R + r]);
        s.cell_off[r] = cells;
        cells += (int64_t)s.longest[r] * (int64_t)N;
        s.col_off[r] = cols;
        if (!s.is_sex[r]) cols += (int64_t)s.longest[r] + 1;       // the sample's tiles, then zeros: longest + 1 bytes (:690-702)
    }
    s.n_cells = cells;
    s.m = cols;
    s.m_pad = std::max<int64_t>((cols + gd::IC_KSTEP - 1) / gd::IC_KSTEP * gd::IC_KSTEP, gd::IC_KSTEP);
    s.n_pad = (n_samples + gd::IC_BLOCK - 1) / gd::IC_BLOCK * gd::IC_BLOCK;
    if (int r = ic_put(c, s, &j.tile_cnt, s.tile_cnt.data(), N * R)) return r;
    if (int r = ic_put(c, s, &j.longest, s.longest.data(), R)) return r;
    if (int r = ic_put(c, s, &j.cell_off, s.cell_off.data(), R)) return r;
    if (int r = ic_put(c, s, &j.col_off, s.col_off.data(), R)) return r;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    j.m_pad = s.m_pad;
    s.secs[0] = t1 - t0 + (ic_now() - t2);
    s.secs[1] = t2 - t1;
    return GD_OK;
    };
    const int rc = body();
    if (rc != GD_OK) drop_state(c, c->ic);
    else s.uploaded = true;
    return rc;
}

#define IC_STATE(c)                                                                        \
    if (!(c)) return GD_E_INVALID;                                                         \
    if (!(c)->ic || !(c)->ic->uploaded) return fail((c), GD_E_STATE, "gd_indexcov_upload has not been called"); \
    if (int r_ = set_device(c)) return r_;                                                 \
    IcState& s = *(c)->ic

int gd_indexcov_get_dims(gd_ctx* c, gd_indexcov_dims* out, int32_t* longest, int64_t* cell_off, int64_t* col_off)
{
    IC_STATE(c);
    if (out) {
        out->n_tiles = s.n_tiles; out->n_cells = s.n_cells; out->m = s.m; out->m_pad = s.m_pad;
        out->n_samples = s.N; out->n_refs = s.R;
    }
    for (int r = 0; r < s.R; ++r) {
        if (longest) longest[r] = s.longest[(size_t)r];
        if (cell_off) cell_off[r] = s.cell_off[(size_t)r];
        if (col_off) col_off[r] = s.col_off[(size_t)r];
    }
    return GD_OK;
}

int gd_indexcov_medians(gd_ctx* c, int64_t* out)
{
    IC_STATE(c);
    if (!out) return GD_E_INVALID;
    memcpy(out, s.median.data(), s.median.size() * sizeof(int64_t));
    return GD_OK;
}

int gd_indexcov_depths(gd_ctx* c, float* out, size_t cap)
{
    IC_STATE(c);
    if (!out || cap < (size_t)s.n_tiles) return fail(c, GD_E_CAPACITY, "%lld depths, room for %zu", (long long)s.n_tiles, cap);
    HIPCHK(c, hipMemcpyAsync(out, s.job.depth, (size_t)s.n_tiles * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return GD_OK;
}

int gd_indexcov_set_depths(gd_ctx* c, const float* in, size_t n)
{
    IC_STATE(c);
    if (!in || n != (size_t)s.n_tiles) return fail(c, GD_E_INVALID, "%lld depths expected, %zu given", (long long)s.n_tiles, n);
    HIPCHK(c, hipMemcpyAsync(s.job.depth, in, n * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    s.computed = false;
    return GD_OK;
}

int gd_indexcov_compute(gd_ctx* c, int with_gram)
{
    IC_STATE(c);
    gd::IcJob& j = s.job;
    const size_t N = (size_t)s.N, R = (size_t)s.R;
    if (!s.buffers) {
        // the result buffers, once per upload; a failed allocation drops the whole state (the next call says so) rather
        // than leave some of them null behind a pointer that is set
        auto make = [&]() -> int {
            if (int r = ic_alloc(c, s, &j.cells, (size_t)s.n_cells)) return r;
            if (int r = ic_alloc(c, s, &j.slots, R * N * gd::IC_SLOTS)) return r;
            if (int r = ic_alloc(c, s, &j.counters, N * 4)) return r;
            if (int r = ic_alloc(c, s, &j.cn, R * N)) return r;
            if (int r = ic_alloc(c, s, &j.X, (size_t)s.n_pad * (size_t)s.m_pad)) return r;
            if (int r = ic_alloc(c, s, &s.d_sums, (size_t)s.n_pad)) return r;
            if (int r = ic_alloc(c, s, &s.d_P, (size_t)s.n_pad * (size_t)s.n_pad)) return r;
            if (int r = ic_alloc(c, s, &s.d_G, N * N)) return r;
            const int nb = s.n_pad / gd::IC_BLOCK;
            std::vector<int2> pairs;
            for (int a = 0; a < nb; ++a)
                for (int b = a; b < nb; ++b) pairs.push_back(make_int2(a, b));
            if (int r = ic_put(c, s, &s.d_pairs, pairs.data(), pairs.size())) return r;
            HIPCHK(c, hipStreamSynchronize(c->stream));    // (pairs is read by the copy until here)
            s.n_pairs = pairs.size();
            return GD_OK;
        };
        if (const int r = make()) { drop_state(c, c->ic); return r; }
        s.buffers = true;
    }
    HIPCHK(c, hipMemsetAsync(j.counters, 0, N * 4 * sizeof(unsigned long long), c->stream));
    HIPCHK(c, hipMemsetAsync(j.cn, 0, R * N * sizeof(double), c->stream));
    HIPCHK(c, hipMemsetAsync(j.X, 0, (size_t)s.n_pad * (size_t)s.m_pad, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const double t0 = ic_now();
    hipLaunchKernelGGL(gd::gd_ic_pass_kernel, dim3((unsigned)R, (unsigned)N), dim3(gd::IC_WG), 0, c->stream, j);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const double t1 = ic_now();
    hipLaunchKernelGGL(gd::gd_ic_cn_kernel, dim3((unsigned)R, (unsigned)N), dim3(gd::IC_WG), 0, c->stream, j);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const double t2 = ic_now();
    s.gram = false;
    if (with_gram && s.m > 0) {
        HIPCHK(c, hipMemsetAsync(s.d_P, 0, (size_t)s.n_pad * (size_t)s.n_pad * sizeof(long long), c->stream));
        hipLaunchKernelGGL(gd::gd_ic_rowsum_kernel, dim3((unsigned)s.n_pad), dim3(gd::IC_WG), 0, c->stream, j.X, s.m_pad, s.d_sums);
        const unsigned chunks = (unsigned)((s.m_pad + gd::IC_KCHUNK - 1) / gd::IC_KCHUNK);
        hipLaunchKernelGGL(gd::gd_ic_gram_kernel, dim3((unsigned)s.n_pairs, chunks), dim3(gd::IC_WG), 0, c->stream,
                           j.X, s.m_pad, (int)s.n_pad, s.d_pairs, s.d_P);
        hipLaunchKernelGGL(gd::gd_ic_gram_fin_kernel, dim3((unsigned)((N * N + gd::IC_WG - 1) / gd::IC_WG)), dim3(gd::IC_WG), 0,
                           c->stream, s.d_P, s.d_sums, (int)s.N, (int)s.n_pad, s.m_pad, s.d_G);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipStreamSynchronize(c->stream));
        s.gram = true;
    }
    s.secs[2] = t1 - t0; s.secs[3] = t2 - t1; s.secs[4] = ic_now() - t2;
    s.computed = true;
    return GD_OK;
}

#define IC_COMPUTED(c) \
    IC_STATE(c);       \
    if (!s.computed) return fail((c), GD_E_STATE, "gd_indexcov_compute has not been called")

int gd_indexcov_cells(gd_ctx* c, int64_t first, int64_t n, uint32_t* out)
{
    IC_COMPUTED(c);
    if (!out || first < 0 || n < 0 || first + n > s.n_cells) return fail(c, GD_E_RANGE, "cells %lld + %lld of %lld", (long long)first, (long long)n, (long long)s.n_cells);
    if (n) HIPCHK(c, hipMemcpy(out, s.job.cells + first, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return GD_OK;
}

int gd_indexcov_slots(gd_ctx* c, int32_t* out)
{
    IC_COMPUTED(c);
    if (!out) return GD_E_INVALID;
    HIPCHK(c, hipMemcpy(out, s.job.slots, (size_t)s.R * s.N * gd::IC_SLOTS * sizeof(int32_t), hipMemcpyDeviceToHost));
    return GD_OK;
}

int gd_indexcov_counters(gd_ctx* c, int64_t* out)
{
    IC_COMPUTED(c);
    if (!out) return GD_E_INVALID;
    HIPCHK(c, hipMemcpy(out, s.job.counters, (size_t)s.N * 4 * sizeof(int64_t), hipMemcpyDeviceToHost));
    return GD_OK;
}

int gd_indexcov_cn(gd_ctx* c, double* out)
{
    IC_COMPUTED(c);
    if (!out) return GD_E_INVALID;
    HIPCHK(c, hipMemcpy(out, s.job.cn, (size_t)s.R * s.N * sizeof(double), hipMemcpyDeviceToHost));
    return GD_OK;
}

int gd_indexcov_pca8(gd_ctx* c, uint8_t* out)
{
    IC_COMPUTED(c);
    if (!out) return GD_E_INVALID;
    if (s.m)
        HIPCHK(c, hipMemcpy2D(out, (size_t)s.m, s.job.X, (size_t)s.m_pad, (size_t)s.m, (size_t)s.N, hipMemcpyDeviceToHost));
    return GD_OK;
}

int gd_indexcov_gram(gd_ctx* c, int64_t* out)
{
    IC_COMPUTED(c);
    if (!out) return GD_E_INVALID;
    if (!s.gram) return fail(c, GD_E_STATE, "the Gram matrix was not computed");
    HIPCHK(c, hipMemcpy(out, s.d_G, (size_t)s.N * s.N * sizeof(int64_t), hipMemcpyDeviceToHost));
    return GD_OK;
}

int gd_indexcov_timing(gd_ctx* c, double* out, size_t n)
{
    IC_STATE(c);
    if (!out) return GD_E_INVALID;
    for (size_t i = 0; i < n && i < 5; ++i) out[i] = s.secs[i];
    return GD_OK;
}
