// gd_api_crai.inc -- the tile sizes of .crai slices (part of gd_api.hip, inside extern "C"): check, upload, the count pass,
// the scan of the counts, the write pass, read-back.  The kernels are gd_crai.hpp's.  Nothing is kept between calls.

namespace {

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
    DevBuf d_seq_off, d_tile_off, d_status, d_start, d_span, d_len, d_sizes;
    if (int r = d_seq_off.alloc(c, (S + 1) * sizeof(int64_t))) return r;
    if (int r = d_tile_off.alloc(c, (S + 1) * sizeof(int64_t))) return r;
    if (int r = d_status.alloc(c, S * sizeof(int32_t))) return r;
    if (int r = d_start.alloc(c, (size_t)L * sizeof(int64_t))) return r;
    if (int r = d_span.alloc(c, (size_t)L * sizeof(int64_t))) return r;
    if (int r = d_len.alloc(c, (size_t)L * sizeof(int32_t))) return r;
    HIPCHK(c, hipMemcpyAsync(d_seq_off.get(), seq_off, (S + 1) * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    if (L > 0) {
        HIPCHK(c, hipMemcpyAsync(d_start.get(), aln_start, (size_t)L * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(d_span.get(), aln_span, (size_t)L * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(d_len.get(), slice_len, (size_t)L * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    }
    gd::CraiJob j{};
    j.n_seq = n_seq;
    j.seq_off = d_seq_off.as<int64_t>(); j.aln_start = d_start.as<int64_t>(); j.aln_span = d_span.as<int64_t>();
    j.slice_len = d_len.as<int32_t>(); j.tile_off = d_tile_off.as<int64_t>(); j.status = d_status.as<int32_t>();
    const unsigned grid = (unsigned)std::min<size_t>((S + gd::CRAI_WAVES - 1) / gd::CRAI_WAVES, 2048);
    hipLaunchKernelGGL(gd::gd_crai_kernel<false>, dim3(grid), dim3(gd::CRAI_WAVES * 64), 0, c->stream, j);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(tile_off, d_tile_off.get(), (S + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(status, d_status.get(), S * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    // the scan: the total decides whether the write pass runs at all, so it is needed here either way
    tile_off[0] = 0;
    for (size_t s = 0; s < S; ++s) tile_off[s + 1] += tile_off[s];
    const int64_t total = tile_off[S];
    if (!sizes) return GD_OK;                                  // count only
    if ((uint64_t)total > (uint64_t)cap) return fail(c, GD_E_CAPACITY, "crai: %lld tiles, room for %zu", (long long)total, cap);
    if (total == 0) return GD_OK;
    if (int r = d_sizes.alloc(c, (size_t)total * sizeof(int64_t))) return r;
    HIPCHK(c, hipMemcpyAsync(d_tile_off.get(), tile_off, (S + 1) * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    j.sizes = d_sizes.as<int64_t>();
    hipLaunchKernelGGL(gd::gd_crai_kernel<true>, dim3(grid), dim3(gd::CRAI_WAVES * 64), 0, c->stream, j);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(sizes, d_sizes.get(), (size_t)total * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));              // (the buffers are freed on return)
    return GD_OK;
}
