// gd_api_crai.inc -- the tile sizes of .crai slices (part of gd_api.hip, inside extern "C"): check, upload, the count pass,
// the scan of the counts, the write pass, read-back.  The kernels are gd_crai.hpp's.  Nothing is kept between calls.

namespace {

struct CraiBufs {
    int64_t *seq_off = nullptr, *start = nullptr, *span = nullptr, *tile_off = nullptr, *sizes = nullptr;
    int32_t *len = nullptr, *status = nullptr;
    ~CraiBufs()
    {
        void* all[] = {seq_off, start, span, tile_off, sizes, len, status};
        for (void* p : all) if (p) (void)hipFree(p);
    }
};

constexpr int64_t kCraiMaxPos = 0x7fffffffLL;    // |alnStart| and alnSpan: what a BAM coordinate can hold

}  // namespace

int gd_crai_sizes(gd_ctx* c, int32_t n_seq, const int64_t* seq_off, const int64_t* aln_start, const int64_t* aln_span,
                  const int32_t* slice_len, int64_t* tile_off, int32_t* status, int64_t* sizes, size_t cap)
{
    if (!c || n_seq < 0) return GD_E_INVALID;
    if (n_seq == 0) { if (tile_off) tile_off[0] = 0; return GD_OK; }
    if (!seq_off || !tile_off || !status) return GD_E_INVALID;
    if (int r = set_device(c)) return r;
    // everything is checked before anything is launched
    const size_t S = (size_t)n_seq;
    if (seq_off[0] != 0) return fail(c, GD_E_INVALID, "crai: seq_off must start at 0");
    for (size_t s = 0; s < S; ++s)
        if (seq_off[s + 1] < seq_off[s]) return fail(c, GD_E_INVALID, "crai: seq_off decreases at sequence %zu", s);
    const int64_t L = seq_off[S];
    if (L > 0 && (!aln_start || !aln_span || !slice_len)) return GD_E_INVALID;
    for (int64_t i = 0; i < L; ++i) {
        if (aln_start[i] < -kCraiMaxPos || aln_start[i] > kCraiMaxPos)
            return fail(c, GD_E_RANGE, "crai: alignment start %lld of slice %lld is outside +-(2^31 - 1)", (long long)aln_start[i], (long long)i);
        if (aln_span[i] < 0 || aln_span[i] > kCraiMaxPos)
            return fail(c, GD_E_RANGE, "crai: alignment span %lld of slice %lld is outside 0 .. 2^31 - 1", (long long)aln_span[i], (long long)i);
    }
    CraiBufs b;
    const size_t nl = std::max<size_t>((size_t)L, 1);
    HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&b.seq_off), (S + 1) * sizeof(int64_t)));
    HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&b.tile_off), (S + 1) * sizeof(int64_t)));
    HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&b.status), S * sizeof(int32_t)));
    HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&b.start), nl * sizeof(int64_t)));
    HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&b.span), nl * sizeof(int64_t)));
    HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&b.len), nl * sizeof(int32_t)));
    HIPCHK(c, hipMemcpyAsync(b.seq_off, seq_off, (S + 1) * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    if (L > 0) {
        HIPCHK(c, hipMemcpyAsync(b.start, aln_start, (size_t)L * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(b.span, aln_span, (size_t)L * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(b.len, slice_len, (size_t)L * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    }
    gd::CraiJob j{};
    j.n_seq = n_seq;
    j.seq_off = b.seq_off; j.aln_start = b.start; j.aln_span = b.span; j.slice_len = b.len;
    j.tile_off = b.tile_off; j.status = b.status;
    const unsigned grid = (unsigned)std::min<size_t>((S + gd::CRAI_WAVES - 1) / gd::CRAI_WAVES, 2048);
    hipLaunchKernelGGL(gd::gd_crai_kernel<false>, dim3(grid), dim3(gd::CRAI_WAVES * 64), 0, c->stream, j);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(tile_off, b.tile_off, (S + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(status, b.status, S * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    // the scan: the total decides whether the write pass runs at all, so it is needed here either way
    tile_off[0] = 0;
    for (size_t s = 0; s < S; ++s) tile_off[s + 1] += tile_off[s];
    const int64_t total = tile_off[S];
    if (!sizes) return GD_OK;                                  // count only
    if ((uint64_t)total > (uint64_t)cap) return fail(c, GD_E_CAPACITY, "crai: %lld tiles, room for %zu", (long long)total, cap);
    if (total == 0) return GD_OK;
    HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&b.sizes), (size_t)total * sizeof(int64_t)));
    HIPCHK(c, hipMemcpyAsync(b.tile_off, tile_off, (S + 1) * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    j.sizes = b.sizes;
    hipLaunchKernelGGL(gd::gd_crai_kernel<true>, dim3(grid), dim3(gd::CRAI_WAVES * 64), 0, c->stream, j);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(sizes, b.sizes, (size_t)total * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));              // (the buffers are freed on return)
    return GD_OK;
}
