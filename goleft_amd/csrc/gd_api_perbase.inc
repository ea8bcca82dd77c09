// gd_api_perbase.inc -- the per-base vector of a region as runs of equal depth, or of equal depth bin (part of gd_api.hip,
// inside extern "C"; DESIGN.md section 3.21).  The kernels are gd_perbase_runs.hpp's: count, scan, emit on the context's
// stream.  Everything is checked before anything is allocated or launched; what is kept between calls is the scratch (the
// chunk counts, their scan and the device run arrays: grow-only, freed with the context) and the timings.

int gd_perbase_runs(gd_ctx* c, int32_t tid, int64_t start, int64_t end, int n_cuts, const int32_t* cuts, uint32_t* run_start,
                    int32_t* run_value, size_t cap, size_t* n)
{
    if (!c || !n) return GD_E_INVALID;
    if (int r = in_flight(c)) return r;
    if (int r = check_result_tid(c, tid)) return r;
    const ContigHost& h = c->contigs[tid];
    if (start < 0 || end < start || end > h.length)
        return fail(c, GD_E_RANGE, "region [%lld,%lld) outside contig of length %lld", (long long)start, (long long)end, (long long)h.length);
    if (n_cuts < 0 || n_cuts > GD_PERBASE_MAX_CUTS) return fail(c, GD_E_INVALID, "perbase runs: 0 .. %d cuts, not %d", GD_PERBASE_MAX_CUTS, n_cuts);
    if (n_cuts > 0 && !cuts) return GD_E_INVALID;
    for (int k = 0; k < n_cuts; ++k) {
        if (cuts[k] < 1) return fail(c, GD_E_INVALID, "perbase runs: cut %d is %d: a cut is at least 1", k, cuts[k]);
        if (k && cuts[k] <= cuts[k - 1]) return fail(c, GD_E_INVALID, "perbase runs: cut %d (%d) is not above cut %d (%d)", k, cuts[k], k - 1, cuts[k - 1]);
    }
    if (!c->d_perbase) return fail(c, GD_E_STATE, "the per-base vector was not kept (gd_set_outputs)");
    *n = 0;
    if (end == start) return GD_OK;
    if (int r = set_device(c)) return r;

    gd::PbJob j{};
    j.d = c->d_perbase + h.base_off;
    j.start = start; j.end = end;
    j.g0 = start - (int64_t)((reinterpret_cast<uintptr_t>(j.d + start) >> 2) & 3u);
    const uint64_t n_chunks = (uint64_t)(end - j.g0 + gd::PB_CHUNK - 1) / gd::PB_CHUNK;       // < 2^20: a contig is below 2^31
    j.n_chunks = (uint32_t)n_chunks;
    j.n_cuts = n_cuts;
    for (int k = 0; k < n_cuts; ++k) j.cuts[k] = cuts[k];
    if (int r = ensure_dev(c, c->d_pb_cnt, n_chunks)) return r;
    if (int r = ensure_dev(c, c->d_pb_base, n_chunks + 1)) return r;
    j.chunk_cnt = c->d_pb_cnt; j.chunk_base = c->d_pb_base;
    c->pb_secs[0] = c->pb_secs[1] = c->pb_secs[2] = c->pb_secs[3] = 0;

    const double t0 = ing_now();
    if (n_cuts) hipLaunchKernelGGL(gd::gd_pb_count_kernel<true>, dim3(j.n_chunks), dim3(gd::PB_WG), 0, c->stream, j);
    else hipLaunchKernelGGL(gd::gd_pb_count_kernel<false>, dim3(j.n_chunks), dim3(gd::PB_WG), 0, c->stream, j);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));                // (only so that the kernels are timed apart)
    c->pb_secs[0] = ing_now() - t0;
    const double t1 = ing_now();
    hipLaunchKernelGGL(gd::gd_pb_scan_kernel, dim3(1), dim3(gd::PB_WG), 0, c->stream, j);
    HIPCHK(c, hipGetLastError());
    uint32_t total = 0;
    HIPCHK(c, hipMemcpyAsync(&total, j.chunk_base + j.n_chunks, sizeof total, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->pb_secs[1] = ing_now() - t1;
    *n = total;
    if (cap < total || !run_start || !run_value) return fail(c, GD_E_CAPACITY, "need room for %u runs", total);

    if (int r = ensure_dev(c, c->d_pb_start, total)) return r;
    if (int r = ensure_dev(c, c->d_pb_value, total)) return r;
    j.run_start = c->d_pb_start; j.run_value = c->d_pb_value;
    j.cap = std::min(c->d_pb_start.cap(), c->d_pb_value.cap());
    const double t2 = ing_now();
    if (n_cuts) hipLaunchKernelGGL(gd::gd_pb_emit_kernel<true>, dim3(j.n_chunks), dim3(gd::PB_WG), 0, c->stream, j);
    else hipLaunchKernelGGL(gd::gd_pb_emit_kernel<false>, dim3(j.n_chunks), dim3(gd::PB_WG), 0, c->stream, j);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->pb_secs[2] = ing_now() - t2;
    const double t3 = ing_now();
    HIPCHK(c, hipMemcpyAsync(run_start, j.run_start, (size_t)total * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(run_value, j.run_value, (size_t)total * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->pb_secs[3] = ing_now() - t3;
    return GD_OK;
}

int gd_perbase_runs_timing(gd_ctx* c, double* out, size_t n)
{
    if (!c || !out) return GD_E_INVALID;
    for (size_t i = 0; i < n && i < 4; ++i) out[i] = c->pb_secs[i];
    return GD_OK;
}
