// gd_api_cnveval.inc -- cnveval.Evaluate on the device (part of gd_api.hip, inside extern "C"): the one host form and the
// seconds of the last call.  The kernels are gd_cnveval.hpp's.  Everything is checked before anything is allocated or
// launched; nothing is kept between calls but the timings.

namespace {

static int ce_check_interval(gd_ctx* c, const char* what, size_t i, int32_t chrom, int32_t start, int32_t end)
{
    if (chrom < 0) return fail(c, GD_E_RANGE, "cnveval: %s %zu: chromosome rank %d is negative", what, i, chrom);
    if (start < 0) return fail(c, GD_E_RANGE, "cnveval: %s %zu: start %d is negative", what, i, start);
    if (end < start) return fail(c, GD_E_RANGE, "cnveval: %s %zu: end %d is before start %d", what, i, end, start);
    return GD_OK;
}

// a CSR of n rows: from 0, never decreasing, at most `limit` entries
static int ce_check_offsets(gd_ctx* c, const char* what, const int64_t* off, size_t n, int64_t limit)
{
    if (off[0] != 0) return fail(c, GD_E_INVALID, "cnveval: %s offsets: offset 0 is %lld, not 0", what, (long long)off[0]);
    for (size_t i = 0; i < n; ++i)
        if (off[i + 1] < off[i])
            return fail(c, GD_E_INVALID, "cnveval: %s offsets: offset %zu (%lld) is below offset %zu (%lld)", what, i + 1,
                        (long long)off[i + 1], i, (long long)off[i]);
    if (off[n] > limit) return fail(c, GD_E_RANGE, "cnveval: %lld %s entries, at most %lld", (long long)off[n], what, (long long)limit);
    return GD_OK;
}

// n elements of `size` bytes on the device (at least one byte), owned by *mem, filled from src on the context's stream
static int ce_upload(gd_ctx* c, DevList* mem, void* dst_ptr, const void* src, size_t n, size_t size)
{
    uint8_t* d = nullptr;
    if (int r = mem->alloc(c, &d, n * size)) return r;
    if (n) HIPCHK(c, hipMemcpyAsync(d, src, n * size, hipMemcpyHostToDevice, c->stream));
    memcpy(dst_ptr, &d, sizeof d);
    return GD_OK;
}

}  // namespace

int gd_cnveval(gd_ctx* c, int32_t n_samples, const int64_t* cnv_off, const int32_t* cnv_chrom, const int32_t* cnv_start,
               const int32_t* cnv_end, const int32_t* cnv_cn, size_t n_truths, const int32_t* t_chrom, const int32_t* t_start,
               const int32_t* t_end, const int32_t* t_cn, const int64_t* t_off, const int32_t* t_samples, double min_overlap,
               int64_t* stats)
{
    if (!c) return GD_E_INVALID;
    if (!(min_overlap > 0 && min_overlap <= 1)) return fail(c, GD_E_RANGE, "cnveval: the minimum overlap is above 0 and at most 1, not %g", min_overlap);
    if (n_samples < 0 || n_samples > GD_CNVEVAL_MAX_SAMPLES)
        return fail(c, GD_E_RANGE, "cnveval: 0 .. %d samples, not %d", GD_CNVEVAL_MAX_SAMPLES, n_samples);
    if (n_truths > (size_t)GD_CNVEVAL_MAX_TRUTHS) return fail(c, GD_E_RANGE, "cnveval: %zu truths, at most %d", n_truths, GD_CNVEVAL_MAX_TRUTHS);
    if (!cnv_off || !t_off || (n_samples > 0 && !stats)) return GD_E_INVALID;
    const size_t S = (size_t)n_samples;
    if (int r = ce_check_offsets(c, "call", cnv_off, S, GD_CNVEVAL_MAX_CNVS)) return r;
    if (int r = ce_check_offsets(c, "truth sample", t_off, n_truths, GD_CNVEVAL_MAX_ENTRIES)) return r;
    const size_t n_cnvs = (size_t)cnv_off[S], n_entries = (size_t)t_off[n_truths];
    if (n_cnvs && (!cnv_chrom || !cnv_start || !cnv_end || !cnv_cn)) return GD_E_INVALID;
    if (n_truths && (!t_chrom || !t_start || !t_end || !t_cn)) return GD_E_INVALID;
    if (n_entries && !t_samples) return GD_E_INVALID;
    const size_t words = (S + 31) / 32;
    if (words * n_truths > (size_t)GD_CNVEVAL_MAX_MEMBER_WORDS)
        return fail(c, GD_E_RANGE, "cnveval: %zu truths of %d samples need %zu membership words, at most %d", n_truths, n_samples,
                    words * n_truths, GD_CNVEVAL_MAX_MEMBER_WORDS);
    const double t0 = ing_now();
    // the calls: in range, in order within a sample; key[] and the samples that have calls fall out of the same pass
    std::vector<int64_t> key(n_cnvs);
    std::vector<int32_t> active;
    for (size_t s = 0; s < S; ++s) {
        if (cnv_off[s + 1] > cnv_off[s]) active.push_back((int32_t)s);
        int32_t reach = 0;
        for (size_t i = (size_t)cnv_off[s]; i < (size_t)cnv_off[s + 1]; ++i) {
            if (int r = ce_check_interval(c, "call", i, cnv_chrom[i], cnv_start[i], cnv_end[i])) return r;
            const bool first = i == (size_t)cnv_off[s];
            if (!first && (cnv_chrom[i] < cnv_chrom[i - 1] || (cnv_chrom[i] == cnv_chrom[i - 1] && cnv_start[i] < cnv_start[i - 1])))
                return fail(c, GD_E_UNSORTED, "cnveval: call %zu of sample %zu sorts before call %zu: a sample's calls are in (chromosome rank, start) order", i, s, i - 1);
            reach = first || cnv_chrom[i] != cnv_chrom[i - 1] ? cnv_end[i] : std::max(reach, cnv_end[i]);
            key[i] = ((int64_t)cnv_chrom[i] << 32) | (int64_t)reach;
        }
    }
    for (size_t t = 0; t < n_truths; ++t)
        if (int r = ce_check_interval(c, "truth", t, t_chrom[t], t_start[t], t_end[t])) return r;
    // the entries turned round: per sample the truths that name it, one per naming
    std::vector<int64_t> st_off(S + 1, 0);
    for (size_t k = 0; k < n_entries; ++k) {
        if (t_samples[k] < 0 || t_samples[k] >= n_samples)
            return fail(c, GD_E_RANGE, "cnveval: truth sample entry %zu: id %d is not one of the %d samples", k, t_samples[k], n_samples);
        ++st_off[(size_t)t_samples[k] + 1];
    }
    for (size_t s = 0; s < S; ++s) st_off[s + 1] += st_off[s];
    std::vector<int32_t> st_truth(n_entries);
    {
        std::vector<int64_t> at(st_off.begin(), st_off.end() - 1);
        for (size_t t = 0; t < n_truths; ++t)
            for (int64_t k = t_off[t]; k < t_off[t + 1]; ++k) st_truth[(size_t)at[(size_t)t_samples[k]]++] = (int32_t)t;
    }
    c->ce_secs[0] = c->ce_secs[1] = c->ce_secs[2] = c->ce_secs[3] = 0;
    if (S) memset(stats, 0, S * gd::CE_CELLS * sizeof(int64_t));
    if (active.empty()) return GD_OK;                          // no calls: no sample is evaluated
    if (int r = set_device(c)) return r;
    DevList mem;
    gd::CeJob j{};
    {
        int64_t *d_off, *d_key, *d_st_off;
        int32_t *d_cs, *d_ce, *d_cn, *d_tc, *d_ts, *d_te, *d_tn, *d_active, *d_st_truth;
        if (int r = ce_upload(c, &mem, &d_off, cnv_off, S + 1, sizeof *d_off)) return r;
        if (int r = ce_upload(c, &mem, &d_key, key.data(), n_cnvs, sizeof *d_key)) return r;
        if (int r = ce_upload(c, &mem, &d_cs, cnv_start, n_cnvs, sizeof *d_cs)) return r;
        if (int r = ce_upload(c, &mem, &d_ce, cnv_end, n_cnvs, sizeof *d_ce)) return r;
        if (int r = ce_upload(c, &mem, &d_cn, cnv_cn, n_cnvs, sizeof *d_cn)) return r;
        if (int r = ce_upload(c, &mem, &d_tc, t_chrom, n_truths, sizeof *d_tc)) return r;
        if (int r = ce_upload(c, &mem, &d_ts, t_start, n_truths, sizeof *d_ts)) return r;
        if (int r = ce_upload(c, &mem, &d_te, t_end, n_truths, sizeof *d_te)) return r;
        if (int r = ce_upload(c, &mem, &d_tn, t_cn, n_truths, sizeof *d_tn)) return r;
        if (int r = ce_upload(c, &mem, &d_active, active.data(), active.size(), sizeof *d_active)) return r;
        if (int r = ce_upload(c, &mem, &d_st_off, st_off.data(), S + 1, sizeof *d_st_off)) return r;
        if (int r = ce_upload(c, &mem, &d_st_truth, st_truth.data(), n_entries, sizeof *d_st_truth)) return r;
        j.cnv_off = d_off; j.key = d_key; j.c_start = d_cs; j.c_end = d_ce; j.c_cn = d_cn;
        j.t_chrom = d_tc; j.t_start = d_ts; j.t_end = d_te; j.t_cn = d_tn; j.n_truths = (int64_t)n_truths;
        j.active = d_active; j.st_off = d_st_off; j.st_truth = d_st_truth; j.po = min_overlap;
        if (int r = mem.alloc(c, &j.flags, n_cnvs, true)) return r;
        if (int r = mem.alloc(c, &j.member, words * n_truths, true)) return r;
        if (int r = mem.alloc(c, &j.stats, S * gd::CE_CELLS, true)) return r;
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->ce_secs[0] = ing_now() - t0;
    const double t1 = ing_now();
    const unsigned gx = (unsigned)active.size();
    hipLaunchKernelGGL(gd::gd_cnveval_positive_kernel, dim3(gx), dim3(gd::CE_WG), 0, c->stream, j);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));                // (only so that the two kernels are timed apart)
    c->ce_secs[3] = ing_now() - t1;
    if (n_truths) {
        const size_t passes = (n_truths + gd::CE_WG - 1) / gd::CE_WG;
        const unsigned gy = (unsigned)std::min<size_t>(passes, std::max<size_t>(1, (size_t)gd::CE_TARGET_BLOCKS / gx));
        hipLaunchKernelGGL(gd::gd_cnveval_pairs_kernel, dim3(gx, gy), dim3(gd::CE_WG), 0, c->stream, j);
        HIPCHK(c, hipGetLastError());
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->ce_secs[1] = ing_now() - t1;
    const double t2 = ing_now();
    HIPCHK(c, hipMemcpyAsync(stats, j.stats, S * gd::CE_CELLS * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->ce_secs[2] = ing_now() - t2;
    return GD_OK;
}

int gd_cnveval_timing(gd_ctx* c, double* out, size_t n)
{
    if (!c || !out) return GD_E_INVALID;
    for (size_t i = 0; i < n && i < 4; ++i) out[i] = c->ce_secs[i];
    return GD_OK;
}
