// gd_api_ingest.inc -- the BAM read on the device: BGZF inflate, member listing, the streaming ingest
// (begin / feed / decode / release) and page-locked host memory (part of gd_api.hip, inside extern "C").

int gd_inflate_bgzf(gd_ctx* c, const uint8_t* data, size_t n_bytes, size_t n_members, const uint64_t* in_off,
                    const uint32_t* in_len, const uint64_t* out_off, const uint32_t* out_len, const uint32_t* crc,
                    uint8_t* out, size_t out_bytes, uint32_t* status)
{
    if (!c || !data || !in_off || !in_len || !out_off || !out_len || !out || !status) return GD_E_INVALID;
    if (int r = set_device(c)) return r;
    if (n_members == 0) return GD_OK;
    if (n_members > 0xffffffffull) return fail(c, GD_E_RANGE, "too many BGZF members");
    for (size_t m = 0; m < n_members; ++m)
        if (in_off[m] + in_len[m] > n_bytes || out_off[m] + out_len[m] > out_bytes)
            return fail(c, GD_E_RANGE, "BGZF member %zu outside the given buffers", m);
    DevBuf b_in, b_out, b_tab;
    const size_t tab_bytes = n_members * (2 * sizeof(uint64_t) + 4 * sizeof(uint32_t));
    if (int r = b_in.alloc(c, n_bytes + gd::INF_SLACK)) return r;
    if (int r = b_out.alloc(c, out_bytes + gd::INF_SLACK)) return r;
    if (int r = b_tab.alloc(c, tab_bytes)) return r;
    uint8_t *d_in = b_in.as<uint8_t>(), *d_out = b_out.as<uint8_t>();
    uint64_t* t_in_off = b_tab.as<uint64_t>();
    uint64_t* t_out_off = t_in_off + n_members;
    uint32_t* t_in_len = reinterpret_cast<uint32_t*>(t_out_off + n_members);
    uint32_t* t_out_len = t_in_len + n_members;
    uint32_t* t_status = t_out_len + n_members;
    uint32_t* t_crc = t_status + n_members;
    if (crc && hipMemcpyAsync(t_crc, crc, n_members * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream) != hipSuccess) crc = nullptr;
    hipError_t e1 = hipMemcpyAsync(d_in, data, n_bytes, hipMemcpyHostToDevice, c->stream);
    hipError_t e2 = hipMemcpyAsync(t_in_off, in_off, n_members * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream);
    hipError_t e3 = hipMemcpyAsync(t_out_off, out_off, n_members * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream);
    hipError_t e4 = hipMemcpyAsync(t_in_len, in_len, n_members * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream);
    hipError_t e5 = hipMemcpyAsync(t_out_len, out_len, n_members * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream);
    gd::InflateJob j{};
    j.comp = d_in; j.in_off = t_in_off; j.in_len = t_in_len; j.out_off = t_out_off; j.out_len = t_out_len;
    j.crc = crc ? t_crc : nullptr;
    j.out = d_out; j.status = t_status; j.n = (uint32_t)n_members;
    if (c->profiling) (void)hipEventRecord(c->ev[0], c->stream);
    gd::inflate_launch(j, c->stream, c->inflate_kernel);
    if (c->profiling) (void)hipEventRecord(c->ev[1], c->stream);
    hipError_t e6 = hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, c->stream);
    hipError_t e7 = hipMemcpyAsync(status, t_status, n_members * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream);
    hipError_t e8 = hipStreamSynchronize(c->stream);
    if (c->profiling && e8 == hipSuccess) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, c->ev[0], c->ev[1]) == hipSuccess) c->kernel_ms[GD_K_INFLATE] = ms;
    }
    for (hipError_t x : {e1, e2, e3, e4, e5, e6, e7, e8})
        if (x != hipSuccess) return fail(c, GD_E_HIP, "BGZF inflate kernel failed: %s", hipGetErrorString(x));
    return GD_OK;
}

int gd_host_alloc(gd_ctx* c, size_t bytes, void** out)
{
    if (!c || !out) return GD_E_INVALID;
    if (int r = set_device(c)) return r;
    *out = nullptr;
    if (hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess)
        return fail(c, GD_E_NOMEM, "cannot page-lock %zu bytes", bytes);
    return GD_OK;
}

int gd_host_free(gd_ctx* c, void* p)
{
    if (!c) return GD_E_INVALID;
    if (int r = set_device(c)) return r;
    if (p) HIPCHK(c, hipHostFree(p));
    return GD_OK;
}

// ---- device BAM read: begin (member tables, allocations) / feed (bytes) / finish (records) ----
static double ing_now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

int gd_ingest_timing(gd_ctx* c, double* out, size_t n)
{
    if (!c || (n && !out)) return GD_E_INVALID;
    for (size_t k = 0; k < n && k < 7; ++k) out[k] = c->ing_secs[k];
    return GD_OK;
}

// Waits for the read gd_ingest_feed_fd started; its status.
static int ingest_join(gd_ctx* c)
{
    if (!c->ing_feeder.joinable()) return GD_OK;
    c->ing_feeder.join();
    const int rc = c->ing_feeder_rc;
    c->ing_feeder_rc = GD_OK;
    c->ing_secs[0] += c->ing_feeder_secs[0]; c->ing_secs[1] += c->ing_feeder_secs[1];
    c->ing_feeder_secs[0] = c->ing_feeder_secs[1] = 0;
    if (rc != GD_OK && !c->ing_feeder_err.empty()) c->err = c->ing_feeder_err;
    c->ing_feeder_err.clear();
    return rc;
}

int gd_ingest_abort(gd_ctx* c)
{
    if (!c) return GD_E_INVALID;
    (void)ingest_join(c);
    if (c->ing_n == 0) return GD_OK;
    (void)hipSetDevice(c->device);
    if (c->ing_hp) (void)hipStreamSynchronize(c->ing_hp);
    (void)hipStreamSynchronize(c->copy_stream);
    (void)hipStreamSynchronize(c->stream);
    for (hipStream_t s : c->ing_stream)
        if (s) (void)hipStreamSynchronize(s);
    for (int i = 0; i < c->ing_n; ++i) { delete c->ing_q[i]; c->ing_q[i] = nullptr; }
    c->ing_n = 0;
    return GD_OK;
}

// Drops the oldest pending range (its device work must be complete: the caller decoded it).
static void ingest_pop(gd_ctx* c)
{
    if (c->ing_n == 0) return;
    (void)hipStreamSynchronize(c->stream);               // the record walks read its inflated bytes
    delete c->ing_q[0];
    for (int i = 0; i + 1 < gd_ctx::kIngestDepth; ++i) c->ing_q[i] = c->ing_q[i + 1];
    c->ing_q[gd_ctx::kIngestDepth - 1] = nullptr;
    --c->ing_n;
}

int gd_ingest_release(gd_ctx* c)
{
    if (!c) return GD_E_INVALID;
    if (c->ing_n < 2)
        if (int r = ingest_join(c)) { (void)gd_ingest_abort(c); return r; }
    if (int r = set_device(c)) return r;
    if (c->ing_n == 0) return fail(c, GD_E_STATE, "no fed range is pending");
    IngestState* g = c->ing_q[0];
    if (g->next != g->nm) return fail(c, GD_E_STATE, "the oldest range is still being fed (gd_ingest_abort drops it)");
    for (hipEvent_t e : g->inf_done) HIPCHK(c, hipEventSynchronize(e));   // its inflate kernels write its buffers
    ingest_pop(c);
    return GD_OK;
}

int gd_ingest_begin(gd_ctx* c, uint64_t n_bytes, uint64_t base_coffset, size_t n_members, const uint64_t* member_off,
                    const uint32_t* member_size, const uint16_t* header_size, const uint32_t* isize, const uint32_t* crc)
{
    if (int r = in_flight(c)) return r;
    if (!c || n_members == 0 || !member_off || !member_size || !header_size || !isize || !crc) return GD_E_INVALID;
    // (a read in progress -- gd_ingest_feed_fd -- fills the newest range meanwhile: this call touches neither that
    // range nor the staging buffers; its error surfaces at the next gd_ingest_feed*)
    const bool reading = c->ing_feeder.joinable();
    if (int r = set_device(c)) return r;
    struct Tb { gd_ctx* c; double t0; ~Tb() { c->ing_secs[2] += ing_now() - t0; } } tb{c, ing_now()};
    if (n_members > 0xfffffff0ull) return fail(c, GD_E_RANGE, "too many BGZF members");
    // a range that was not fed to its end is an abandoned read: start over.  A completely fed one may
    // wait for its decode while this one is fed.
    if (!reading && c->ing_n && c->ing_q[c->ing_n - 1]->next != c->ing_q[c->ing_n - 1]->nm) (void)gd_ingest_abort(c);
    if (c->ing_n == gd_ctx::kIngestDepth) return fail(c, GD_E_STATE, "%d fed ranges are pending: decode and release the oldest first", c->ing_n);
    IngestState* g = new (std::nothrow) IngestState();
    if (!g) return GD_E_NOMEM;
    c->ing_q[c->ing_n++] = g;
    auto bail = [&](int code, const char* msg) { (void)gd_ingest_abort(c); return fail(c, code, "%s", msg); };
    g->n_bytes = n_bytes;
    g->base = base_coffset;
    g->nm = n_members;
    g->m_coff.resize(n_members); g->m_end.resize(n_members);
    g->out_off.resize(n_members); g->out_len.assign(isize, isize + n_members);
    const size_t tab_bytes = n_members * (2 * sizeof(uint64_t) + 4 * sizeof(uint32_t));
    g->bufs = nullptr;
    for (IngestBufs& b : c->ing_bufs)
        if (!b.busy) { g->bufs = &b; break; }
    if (!g->bufs) return bail(GD_E_STATE, "no free range buffers (internal error)");
    g->bufs->busy = true;
    if (!IngestBufs::fit_host(g->bufs->tab, tab_bytes))
        return bail(GD_E_NOMEM, "cannot page-lock the BGZF member table");
    g->t_in_off = g->bufs->tab.as<uint64_t>();
    g->t_out_off = g->t_in_off + n_members;
    g->t_in_len = reinterpret_cast<uint32_t*>(g->t_out_off + n_members);
    g->t_out_len = g->t_in_len + n_members;
    g->t_status = g->t_out_len + n_members;
    g->t_crc = g->t_status + n_members;
    uint64_t total = 0;
    for (size_t m = 0; m < n_members; ++m) {
        if (member_size[m] < (uint32_t)header_size[m] + 8u || member_off[m] + member_size[m] > n_bytes ||
            (m && member_off[m] < member_off[m - 1] + member_size[m - 1]))
            return bail(GD_E_INVALID, "inconsistent BGZF member table");
        g->m_coff[m] = base_coffset + member_off[m];
        g->m_end[m] = member_off[m] + member_size[m];
        g->t_in_off[m] = member_off[m] + header_size[m];
        g->t_in_len[m] = member_size[m] - header_size[m] - 8u;
        g->t_out_off[m] = total;
        g->t_out_len[m] = isize[m];
        g->t_crc[m] = crc[m];
        g->t_status[m] = 0xffffffffu;                       // (not inflated yet)
        g->out_off[m] = total;
        total += isize[m];
    }
    g->total = total;
    // GD_OPT_INGEST_RANGE_HINT: the caller knows the largest range it is going to feed -- both buffer sets are allocated
    // for THAT on their first use (the inflated size scaled by this range's ratio), so that no later, larger range frees and
    // allocates again (a hipFree waits for the whole device, the other range's kernels included; and on some boxes
    // hipMalloc costs 50 ms per gigabyte)
    size_t want_in = (size_t)n_bytes, want_out = (size_t)total;
    if (c->ing_range_hint && n_bytes > 0) {
        // (15 % on top of this range's ratio, also when this range IS the largest: ranges of one compressed size differ by a
        // few per cent in what they inflate to, and a set that has to GROW is freed first -- a hipFree that waits for the
        // other ranges' kernels: 0.02-0.09 s each on a quiet device, 0.7 s in a process that started while the driver
        // was still clearing what its predecessor had released, twice per genome read with the 3 % of round 4;
        // profiles/r12p_...)
        const double scale = std::max(1.0, (double)c->ing_range_hint / (double)n_bytes);
        want_in = (size_t)std::max<uint64_t>(c->ing_range_hint, n_bytes);
        want_out = (size_t)((double)total * scale * 1.15);
    }
    // (what exists and holds THIS range stays -- whatever the estimate says now: an estimate 0.1 % above the last one is no
    // reason to free ten gigabytes)
    if ((size_t)n_bytes + gd::INF_SLACK <= g->bufs->in.cap()) want_in = (size_t)n_bytes;
    if ((size_t)total + gd::INF_SLACK <= g->bufs->out.cap()) want_out = (size_t)total;
    if (!IngestBufs::fit(g->bufs->in, std::max<size_t>(want_in, (size_t)n_bytes) + gd::INF_SLACK) ||
        !IngestBufs::fit(g->bufs->out, std::max<size_t>(want_out, (size_t)total) + gd::INF_SLACK))
        return bail(GD_E_NOMEM, "device allocation for the BAM decode failed");
    g->d_in = g->bufs->in;
    g->d_out = g->bufs->out;
    for (int k = 0; k < 2; ++k)
        if ((!c->ing_stage[k] && c->ing_stage[k].alloc(IngestState::kStage) != hipSuccess) ||
            (!c->ing_staged[k] && c->ing_staged[k].create(hipEventDisableTiming | hipEventBlockingSync) != hipSuccess))
            return bail(GD_E_NOMEM, "cannot allocate the page-locked staging buffers");
    // GD_OPT_INGEST_CU_SPLIT = n > 0 (with GD_OPT_INGEST_DMA = 0): every n-th CU belongs to the copy kernel that pulls the
    // staged pieces over the link, the others to the inflate launches -- a copy kernel reaches twice a copy engine's rate
    // on an idle device and loses to it only because the inflate workgroups leave it no room
    std::vector<uint32_t> mask_copy, mask_rest;
    if (c->ing_cu_split > 0 && !c->ing_copy_engine) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, c->device) == hipSuccess && prop.multiProcessorCount >= 2 * c->ing_cu_split) {
            const int ncu = prop.multiProcessorCount, words = (ncu + 31) / 32;
            mask_copy.assign((size_t)words, 0u); mask_rest.assign((size_t)words, 0u);
            for (int i = 0; i < ncu; ++i) ((i % c->ing_cu_split) == 0 ? mask_copy : mask_rest)[(size_t)i / 32] |= 1u << (i % 32);
        }
    }
    for (Stream& s : c->ing_stream)
        if (!s) {
            hipStream_t made = nullptr;
            const hipError_t e = mask_rest.empty() ? hipStreamCreateWithFlags(&made, hipStreamNonBlocking)
                                                   : hipExtStreamCreateWithCUMask(&made, (uint32_t)mask_rest.size(), mask_rest.data());
            if (e != hipSuccess) return bail(GD_E_HIP, "cannot create a stream");
            s.adopt(made);
        }
    if (!mask_copy.empty() && !c->ing_hp) {
        hipStream_t made = nullptr;
        if (hipExtStreamCreateWithCUMask(&made, (uint32_t)mask_copy.size(), mask_copy.data()) != hipSuccess)
            return bail(GD_E_HIP, "cannot create a CU-masked stream");
        c->ing_hp.adopt(made);
    }
    return GD_OK;
}

// Fills staging buffer k with the next `piece` bytes: from memory (bytes != nullptr; the caller's pointer is not
// retained), else from `offset` of `fd`.
static int ingest_fill(gd_ctx* c, int k, const uint8_t* bytes, int fd, uint64_t offset, size_t piece)
{
    if (!bytes) {
        FillPool* pool = ctx_pool(c);
        const size_t nt = (size_t)std::max(1, c->push_threads);
        const size_t slice = ((piece / nt) + 4095) & ~(size_t)4095;
        std::vector<FillPool::Item> items;
        for (size_t b = 0; b < piece; b += std::max<size_t>(slice, 4096)) {
            const size_t e = std::min(piece, b + std::max<size_t>(slice, 4096));
            items.push_back(FillPool::Item{c->ing_stage[k] + b, reinterpret_cast<const void*>((uintptr_t)(offset + b)), e - b,
                                           (uint32_t)fd, FillPool::PREAD, 0});
        }
        if (pool) pool->spin_limit.store(500, std::memory_order_relaxed);
        const uint32_t bad = FillPool::run_items(pool, std::move(items));
        if (pool) pool->spin_limit.store(20000, std::memory_order_relaxed);
        if (bad) return fail(c, GD_E_INVALID, "the file ended early or could not be read");
    } else if (c->ing_copy_threads > 1 && piece >= (8u << 20)) {
        const int nt = c->ing_copy_threads;
        const size_t slice = ((piece / (size_t)nt) + 4095) & ~(size_t)4095;
        std::vector<std::thread> th;
        for (int t = 1; t < nt; ++t) {
            const size_t b = std::min(piece, slice * t), e = std::min(piece, slice * (t + 1));
            if (e > b) th.emplace_back([=]() { memcpy(c->ing_stage[k] + b, bytes + b, e - b); });
        }
        memcpy(c->ing_stage[k], bytes, std::min(piece, slice));
        for (auto& t : th) t.join();
    } else {
        memcpy(c->ing_stage[k], bytes, piece);
    }
    return GD_OK;
}

// Sends staging buffer k's piece behind the bytes the range already holds; ing_staged[k] on the copy stream says it has
// arrived.  A copy command (the library's default), or with GD_OPT_INGEST_DMA = 0 a copy kernel on ing_hp -- a
// high-priority stream, or with GD_OPT_INGEST_CU_SPLIT the CU-masked one gd_ingest_begin made (a copy kernel reaches twice
// a copy engine's rate on an idle device and loses to it only where the inflate workgroups leave it no room).
static int ingest_send(gd_ctx* c, IngestState* g, int k, size_t piece)
{
    if (c->ing_copy_engine) {
        HIPCHK(c, hipMemcpyAsync(g->d_in + g->fed, c->ing_stage[k], piece, hipMemcpyHostToDevice, c->copy_stream));
    } else {
        if (!c->ing_hp) {
            int lo = 0, hi = 0;
            (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
            hipStream_t made = nullptr;
            HIPCHK(c, hipStreamCreateWithPriority(&made, hipStreamNonBlocking, hi));
            c->ing_hp.adopt(made);
        }
        gd::H2DJob hj{};
        hj.seg[0] = gd::H2DSeg{g->d_in + g->fed, c->ing_stage[k], piece};
        hipLaunchKernelGGL(gd::gd_h2d_kernel, dim3(c->ing_copy_grid), dim3(256), 0, c->ing_hp, hj);
        if (!c->ing_hp_done[k]) HIPCHK(c, c->ing_hp_done[k].create(hipEventDisableTiming));
        HIPCHK(c, hipEventRecord(c->ing_hp_done[k], c->ing_hp));
        HIPCHK(c, hipStreamWaitEvent(c->copy_stream, c->ing_hp_done[k], 0));
    }
    HIPCHK(c, hipEventRecord(c->ing_staged[k], c->copy_stream));
    c->ing_stage_used[k] = true;
    g->fed += piece;
    return GD_OK;
}

// Inflates the members that are now completely on the device, behind the copy: an eighth of the range at a time (or
// whatever is left once every byte is in).
static int ingest_inflate_complete(gd_ctx* c, IngestState* g)
{
    size_t last = g->next;
    while (last < g->nm && g->m_end[last] <= g->fed) ++last;
    const size_t quota = std::max<size_t>((g->nm + 7) / 8, 1);
    if (last == g->next || (last - g->next < quota && last != g->nm)) return GD_OK;
    hipStream_t is = c->ing_stream[c->ing_launch_seq++ % 8u];
    ++g->n_launch;
    for (int b = 0; b < 2; ++b)                              // (both pieces that may still be in flight)
        if (c->ing_stage_used[b]) HIPCHK(c, hipStreamWaitEvent(is, c->ing_staged[b], 0));
    gd::InflateJob ij{};
    ij.comp = g->d_in;
    ij.in_off = g->t_in_off + g->next; ij.in_len = g->t_in_len + g->next;
    ij.out_off = g->t_out_off + g->next; ij.out_len = g->t_out_len + g->next;
    ij.crc = c->ingest_crc ? g->t_crc + g->next : nullptr; ij.out = g->d_out; ij.status = g->t_status + g->next;
    ij.n = (uint32_t)(last - g->next);
    gd::inflate_launch(ij, is, c->inflate_kernel);
    hipEvent_t done = nullptr;
    HIPCHK(c, hipEventCreateWithFlags(&done, hipEventDisableTiming | hipEventBlockingSync));   // (waited for by the decoding thread for tens of milliseconds: asleep, not spinning)
    g->inf_done.emplace_back();
    g->inf_done.back().adopt(done);
    HIPCHK(c, hipEventRecord(done, is));
    g->next = last;
    return GD_OK;
}

// The bytes go through the two page-locked staging buffers in turn, a piece of at most IngestState::kStage each.
// bytes != nullptr: from memory; else n bytes from `offset` of `fd`
static int ingest_feed(gd_ctx* c, IngestState* g, const uint8_t* bytes, int fd, uint64_t offset, size_t n)
{
    if (int r = set_device(c)) return r;
    // (the feeder thread keeps its own timers: the caller's thread adds to ing_secs meanwhile)
    double* const secs = tl_ingest_feeder ? c->ing_feeder_secs : c->ing_secs;
    for (size_t done = 0; done < n;) {
        const size_t piece = std::min(n - done, IngestState::kStage);
        const int k = c->ing_cur;
        const double tw0 = ing_now();
        if (c->ing_stage_used[k]) HIPCHK(c, hipEventSynchronize(c->ing_staged[k]));   // its previous H2D has left the buffer
        const double tw1 = ing_now();
        secs[1] += tw1 - tw0;
        if (int r = ingest_fill(c, k, bytes ? bytes + done : nullptr, fd, offset + done, piece)) return r;
        secs[0] += ing_now() - tw1;
        if (int r = ingest_send(c, g, k, piece)) return r;
        c->ing_cur ^= 1;
        done += piece;
        if (int r = ingest_inflate_complete(c, g)) return r;
    }
    return GD_OK;
}

// What gd_ingest_feed and gd_ingest_feed_fd begin with: the read in progress has ended, and the newest range has room
// for n more bytes.
static int ingest_feed_target(gd_ctx* c, size_t n, IngestState** out)
{
    if (int r = ingest_join(c)) { (void)gd_ingest_abort(c); return r; }
    if (int r = in_flight(c)) return r;
    IngestState* g = c->ing_n ? c->ing_q[c->ing_n - 1] : nullptr;
    if (!g) return fail(c, GD_E_STATE, "gd_ingest_begin has not been called");
    if (g->fed + n > g->n_bytes) return fail(c, GD_E_RANGE, "more bytes fed than announced");
    *out = g;
    return GD_OK;
}

int gd_ingest_feed(gd_ctx* c, const uint8_t* bytes, size_t n)
{
    if (!c || (n && !bytes)) return GD_E_INVALID;
    IngestState* g = nullptr;
    if (int r = ingest_feed_target(c, n, &g)) return r;
    return ingest_feed(c, g, bytes, -1, 0, n);
}

// The read runs on a thread of the context and the call returns at once: the caller decodes the range before this
// one meanwhile.  Every other gd_ingest_* call waits for the read first (and reports its error).
int gd_ingest_feed_fd(gd_ctx* c, int fd, uint64_t offset, size_t n)
{
    if (!c || fd < 0) return GD_E_INVALID;
    IngestState* g = nullptr;
    if (int r = ingest_feed_target(c, n, &g)) return r;
    c->ing_feeder_rc = GD_OK;
    c->ing_feeder = std::thread([c, g, fd, offset, n]() { tl_ingest_feeder = true; c->ing_feeder_rc = ingest_feed(c, g, nullptr, fd, offset, n); });
    return GD_OK;
}

// ---- what every decode of a fed range begins with (ingest_decode here, gd_covstats_decode) ----------------------
// Drops everything pending when a decode fails, unless disarmed.
struct IngestGuard { gd_ctx* c; bool on; ~IngestGuard() { if (on) (void)gd_ingest_abort(c); } };

// The oldest pending range, ready to decode (every member fed).  From the moment there is a range the guard is armed.
static int ingest_oldest(gd_ctx* c, IngestGuard* guard, IngestState** out)
{
    if (int r = in_flight(c)) return r;
    if (c->ing_n < 2)                                                 // (with two ranges pending a read in progress fills the newer one)
        if (int r = ingest_join(c)) { (void)gd_ingest_abort(c); return r; }
    if (int r = set_device(c)) return r;
    IngestState* g = c->ing_n ? c->ing_q[0] : nullptr;
    if (!g) return fail(c, GD_E_STATE, "gd_ingest_begin has not been called");
    guard->on = true;
    if (g->next != g->nm) return fail(c, GD_E_STATE, "only %zu of %zu BGZF members were fed", g->next, g->nm);
    *out = g;
    return GD_OK;
}

// Every member of the range is inflated, and inflated well.
static int ingest_wait_inflated(gd_ctx* c, IngestState* g)
{
    const double t0 = ing_now();
    if (!g->inflated) {
        for (hipEvent_t e : g->inf_done) HIPCHK(c, hipEventSynchronize(e));
        for (size_t m = 0; m < g->nm; ++m)                            // (the status words are host memory)
            if (g->t_status[m] != 0)
                return fail(c, GD_E_INVALID, "BGZF member at file offset %llu %s (decoder code %u)",
                            (unsigned long long)g->m_coff[m], g->t_status[m] == 18 ? "fails its CRC32" : "does not inflate", g->t_status[m]);
        g->inflated = true;
    }
    c->ing_secs[3] += ing_now() - t0;
    return GD_OK;
}

// The byte offset in the inflated range of virtual offset v; false: v is not inside a member of the range.
static bool ingest_voff(const IngestState* g, uint64_t v, uint64_t* out)
{
    const uint64_t coff = v >> 16, uoff = v & 0xffffu;
    const size_t k = (size_t)(std::lower_bound(g->m_coff.begin(), g->m_coff.end(), coff) - g->m_coff.begin());
    if (k >= g->nm || g->m_coff[k] != coff || uoff > g->out_len[k]) return false;
    *out = g->out_off[k] + uoff;
    return true;
}

// A walk's per-segment tables: PAGE-LOCKED HOST memory of the context (c->h_walk, grow-only) that the walk kernels read
// and write over the link -- four uploads and five read-backs per decode were copy commands that each queued behind the
// 64 MB pieces of the read in progress; and a per-call device buffer ended in a hipFree, a device-wide wait.  (One table
// for the depth read and covstats: both decode ing_q[0], so never at once.)
static int ingest_walk_table(gd_ctx* c, size_t bytes, const char* whose)
{
    if (bytes <= c->h_walk.cap()) return GD_OK;
    if (c->h_walk) { HIPCHK(c, hipStreamSynchronize(c->stream)); c->h_walk.reset(); }   // (a kernel of the last call may still read it)
    const size_t want = std::max<size_t>(2 * bytes + 4096, 2u << 20);   // (rarely again: see IngestBufs::fit_host)
    if (c->h_walk.alloc(want) != hipSuccess)
        return fail(c, GD_E_NOMEM, "cannot page-lock the %s walk's tables", whose);
    return GD_OK;
}

// One reference of the fed range -> contig tid.  release: the range is dropped afterwards (always on error).
static int ingest_decode(gd_ctx* c, int32_t tid, int32_t ref_id, const uint64_t* anchors, size_t n_anchors,
                         uint64_t* n_records, bool release, uint64_t end_anchor = 0, bool append = false,
                         double expect_scale = 0.0)
{
    if (!c || !anchors || n_anchors == 0) return GD_E_INVALID;
    IngestGuard guard{c, false};
    IngestState* g = nullptr;
    if (int r = ingest_oldest(c, &guard, &g)) return r;
    if (tid < 0 || (size_t)tid >= c->contigs.size()) return fail(c, GD_E_RANGE, "tid %d out of range", tid);
    if (n_anchors > 0xfffffff0ull) return fail(c, GD_E_RANGE, "too many anchors");
    const uint64_t total = g->total;
    // ---- anchors (virtual offsets) -> byte offsets in the inflated range ----------------------
    std::vector<uint64_t> seg_beg(n_anchors), seg_end(n_anchors);
    for (size_t i = 0; i < n_anchors; ++i) {
        if (!ingest_voff(g, anchors[i], &seg_beg[i]))
            return fail(c, GD_E_INVALID, "anchor %zu (virtual offset %llu) is not inside a member of the range", i,
                        (unsigned long long)anchors[i]);
        if (i && seg_beg[i] <= seg_beg[i - 1]) return fail(c, GD_E_INVALID, "anchors must be strictly ascending");
        if (i) seg_end[i - 1] = seg_beg[i];
    }
    seg_end[n_anchors - 1] = total;                   // a record of another reference ends the last walk earlier
    if (end_anchor) {                                 // one part of a reference: up to the first record of the next part
        uint64_t e = 0;
        if (!ingest_voff(g, end_anchor, &e) || e <= seg_beg[n_anchors - 1])
            return fail(c, GD_E_INVALID, "the part's end (virtual offset %llu) is not inside a member of the range behind its last anchor",
                        (unsigned long long)end_anchor);
        seg_end[n_anchors - 1] = e;
    }
    if (int r = ingest_wait_inflated(c, g)) return r;
    const double td1 = ing_now();
    // ---- count the records of every anchor segment ----------------------------------------------
    if (int r = ingest_walk_table(c, n_anchors * 6 * sizeof(uint64_t) + n_anchors * 4 * sizeof(uint32_t), "record")) return r;
    uint64_t* s_beg = c->h_walk.as<uint64_t>();
    uint64_t* s_end = s_beg + n_anchors;
    uint64_t* s_rbase = s_end + n_anchors;
    uint64_t* s_obase = s_rbase + n_anchors;
    uint64_t* s_nops = s_obase + n_anchors;
    uint64_t* s_tbase = s_nops + n_anchors;
    uint32_t* s_nrec = reinterpret_cast<uint32_t*>(s_tbase + n_anchors);
    int32_t* s_first = reinterpret_cast<int32_t*>(s_nrec + n_anchors);
    int32_t* s_last = s_first + n_anchors;
    uint32_t* s_flags = reinterpret_cast<uint32_t*>(s_last + n_anchors);
    memcpy(s_beg, seg_beg.data(), n_anchors * sizeof(uint64_t));
    memcpy(s_end, seg_end.data(), n_anchors * sizeof(uint64_t));
    gd::BamSegJob bj{};
    bj.data = g->d_out; bj.n_bytes = total; bj.seg_beg = s_beg; bj.seg_end = s_end; bj.tid = ref_id;
    bj.n_ref = c->bam_n_ref > 0 ? c->bam_n_ref : 0x7fffffff;
    bj.n_seg = (uint32_t)n_anchors; bj.n_rec = s_nrec; bj.n_ops = s_nops; bj.first_pos = s_first; bj.last_pos = s_last;
    bj.flags = s_flags;
    // the record table: the counting walk notes where every record starts (and the ops of its segment in front of it), the
    // extraction is then a thread per record instead of the walk a second time.  Room per segment for the most records its
    // bytes can hold (36 each at least): 0.22 bytes of table per inflated byte, the context's, grow-only.  A segment of 4 GB
    // (never: anchors are 16 kb of reference apart) or an allocation that fails leave the second walk in place.
    {
        uint64_t n_tab = 0;
        bool fits = true;
        for (size_t i = 0; i < n_anchors; ++i) {
            const uint64_t len = seg_end[i] > seg_beg[i] ? seg_end[i] - seg_beg[i] : 0;
            if (len > 0xffffffffull) fits = false;
            s_tbase[i] = n_tab;
            n_tab += len / 36 + 1;
        }
        if (fits && n_tab * 8 > c->d_rectab.cap()) HIPCHK(c, hipStreamSynchronize(c->stream));   // (a walk of the last call may still read it)
        if (fits && IngestBufs::fit(c->d_rectab, (size_t)n_tab * 8)) {
            bj.tab = c->d_rectab.as<uint32_t>();
            bj.tab_base = s_tbase;
        }
    }
    const unsigned seg_grid = (unsigned)n_anchors;         // one wave per anchor segment
    hipLaunchKernelGGL(gd::gd_bam_walk_kernel<false>, dim3(seg_grid), dim3(64), 0, c->stream, bj);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const double td2 = ing_now();
    c->ing_secs[4] += td2 - td1;
    if (append && c->contigs[tid].adopted) return fail(c, GD_E_STATE, "contig %d holds adopted device records", tid);
    const uint64_t N0 = append ? c->contigs[tid].n_reads : 0, M0 = append ? c->contigs[tid].n_ops : 0;
    uint64_t N = 0, M = 0;
    int32_t prev_last = append ? c->contigs[tid].last_pos : -0x7fffffff;
    bool left = append && c->contigs[tid].ing_left;      // a record of another reference has been met
    for (size_t i = 0; i < n_anchors; ++i) {
        if (s_flags[i] & gd::BW_CORRUPT) return fail(c, GD_E_INVALID, "corrupt BAM record in anchor segment %zu", i);
        // a coordinate-sorted BAM holds a reference's records in ONE run: records of this one after a record of
        // another (a walk that a foreign record ended, then a later anchor with records again) are refused, as the
        // host decoder refuses them -- `samtools depth -r` would silently stop at the foreign record
        if ((left && s_nrec[i]) || (s_flags[i] & gd::BW_REF_RESUMES))
            return fail(c, GD_E_UNSORTED, "contig %d: records continue after a record of another reference (anchor segment %zu)", tid, i);
        if (s_flags[i] & gd::BW_LEFT_REF) left = true;
        if (s_flags[i] & gd::BW_OVERRAN) return fail(c, GD_E_INVALID, "anchor %zu is not a record start (stale or foreign index?)", i + 1);
        if ((s_flags[i] & gd::BW_UNSORTED) || (s_nrec[i] && s_first[i] < prev_last))
            return fail(c, GD_E_UNSORTED, "contig %d: records not coordinate sorted (anchor segment %zu)", tid, i);
        if (s_nrec[i]) prev_last = s_last[i];
        s_rbase[i] = N0 + N;                          // (in place: the extraction reads them from there)
        s_obase[i] = M0 + M;
        N += s_nrec[i];
        M += s_nops[i];
    }
    if (M0 + M > 0xffffffffull) return fail(c, GD_E_RANGE, "more than 2^32 CIGAR ops on contig %d", tid);
    if (N0 + N >= kMaxReadsPerContig) return fail(c, GD_E_RANGE, "more than 2^30 records on contig %d", tid);

    // ---- extract into the contig's SoA arrays ----------------------------------------------------
    HIPCHK(c, hipStreamSynchronize(c->copy_stream));
    ContigHost& h = c->contigs[tid];
    if (!append) {
        free_contig(h);
    } else if (h.ck_ok) {                     // derived structures no longer cover the stream
        HIPCHK(c, hipStreamSynchronize(c->stream));
        drop_ck(h);
    }
    if (N) {
        // one allocation for the whole reference when the caller knows what to expect (a reference read in parts),
        // else exactly what this call holds; a part that outgrows the arrays makes them grow (copied once)
        size_t want_r = (size_t)N, want_o = (size_t)std::max<uint64_t>(M, 1);
        if (!append && expect_scale > 1.0 && expect_scale < 65536.0) {
            const double er = (double)N * expect_scale * 1.06 + 65536, eo = (double)M * expect_scale * 1.06 + 65536;   // (short: the arrays grow, copied once)
            if (er < (double)kMaxReadsPerContig) want_r = (size_t)er;
            if (eo <= 4294967295.0) want_o = (size_t)eo;
        }
        if (append) {
            if (h.n_reads + want_r > h.cap_reads()) want_r = std::max(want_r, h.cap_reads() / 2);
            if (h.n_ops + want_o > h.cigar.cap()) want_o = std::max(want_o, h.cigar.cap() / 2);
        }
        if (int r = reserve_records(c, h, want_r, want_o, Growth::EXACT)) return r;
        c->ing_secs[5] += ing_now() - td2;
        bj.rec_base = s_rbase; bj.op_base = s_obase;
        bj.pos = h.pos; bj.flag = h.flag; bj.mapq = h.mapq; bj.cigar_off = h.off; bj.cigar = h.cigar;
        if (bj.tab) hipLaunchKernelGGL(gd::gd_bam_extract_tab_kernel, dim3(seg_grid), dim3(256), 0, c->stream, bj);
        else hipLaunchKernelGGL(gd::gd_bam_walk_kernel<true>, dim3(seg_grid), dim3(64), 0, c->stream, bj);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(h.off + N0 + N), (int)(uint32_t)(M0 + M), 1, c->stream));   // (a fill kernel, not a copy command)
        // position index + spans of what the walk just wrote (its order and offsets were checked by the walk itself)
        const int32_t before = h.last_pos;
        h.n_reads = (size_t)(N0 + N);
        h.n_ops = (size_t)(M0 + M);
        if (int r = index_records(c, h, (size_t)N0, (size_t)(N0 + N), before, false, c->stream)) return r;
        uint32_t w[3] = {0, 0, 0};
        if (int r = read_ingest_words(c, c->stream, w)) return r;
        if (c->ingest_span_dirty) take_ingest_span(c, (int32_t)w[1]);
        c->ing_secs[6] += ing_now() - td2;
    }
    h.n_reads = (size_t)(N0 + N);
    h.n_ops = (size_t)(M0 + M);
    if (N) h.last_pos = prev_last;
    h.ing_left = left;
    c->computed = false;
    if (n_records) *n_records = N;
    guard.on = false;
    if (release) ingest_pop(c);
    return GD_OK;
}

int gd_ingest_decode(gd_ctx* c, int32_t tid, int32_t ref_id, const uint64_t* anchors, size_t n_anchors, uint64_t* n_records)
{
    return ingest_decode(c, tid, ref_id, anchors, n_anchors, n_records, false);
}

int gd_ingest_finish(gd_ctx* c, int32_t tid, int32_t ref_id, const uint64_t* anchors, size_t n_anchors, uint64_t* n_records)
{
    return ingest_decode(c, tid, ref_id, anchors, n_anchors, n_records, true);
}

int gd_ingest_decode_part(gd_ctx* c, int32_t tid, int32_t ref_id, const uint64_t* anchors, size_t n_anchors, uint64_t end_anchor,
                          unsigned flags, double expect_scale, uint64_t* n_records)
{
    if (c && (flags & ~(unsigned)(GD_PART_APPEND | GD_PART_RELEASE))) return fail(c, GD_E_INVALID, "unknown part flags 0x%x", flags);
    return ingest_decode(c, tid, ref_id, anchors, n_anchors, n_records, (flags & GD_PART_RELEASE) != 0, end_anchor,
                         (flags & GD_PART_APPEND) != 0, expect_scale);
}

// The BGZF members of a byte range (SAMv1 4.1: gzip header with a BC extra subfield).
int gd_bgzf_members(const uint8_t* data, size_t n_bytes, size_t cap, uint64_t* member_off, uint32_t* member_size,
                    uint16_t* header_size, uint32_t* isize, uint32_t* crc, size_t* n_members)
{
    if (!data || !n_members) return GD_E_INVALID;
    size_t nm = 0;
    for (size_t p = 0; p + 18 <= n_bytes;) {
        const uint8_t* h = data + p;
        if (h[0] != 0x1f || h[1] != 0x8b || h[2] != 8 || !(h[3] & 4)) return GD_E_INVALID;
        const size_t xlen = (size_t)h[10] | ((size_t)h[11] << 8);
        if (p + 12 + xlen > n_bytes) break;
        size_t q = 12, bsize = 0;
        while (q + 4 <= 12 + xlen) {
            const size_t slen = (size_t)h[q + 2] | ((size_t)h[q + 3] << 8);
            if (h[q] == 66 && h[q + 1] == 67 && slen == 2 && q + 6 <= 12 + xlen)
                bsize = ((size_t)h[q + 4] | ((size_t)h[q + 5] << 8)) + 1;
            q += 4 + slen;
        }
        if (bsize < 12 + xlen + 8) return GD_E_INVALID;
        if (p + bsize > n_bytes) break;                     // a trailing partial member is ignored
        if (nm < cap) {
            if (member_off) member_off[nm] = p;
            if (member_size) member_size[nm] = (uint32_t)bsize;
            if (header_size) header_size[nm] = (uint16_t)(12 + xlen);
            if (isize) isize[nm] = (uint32_t)h[bsize - 4] | ((uint32_t)h[bsize - 3] << 8) | ((uint32_t)h[bsize - 2] << 16) |
                                   ((uint32_t)h[bsize - 1] << 24);
            if (crc) crc[nm] = (uint32_t)h[bsize - 8] | ((uint32_t)h[bsize - 7] << 8) | ((uint32_t)h[bsize - 6] << 16) |
                               ((uint32_t)h[bsize - 5] << 24);
        }
        ++nm;
        p += bsize;
    }
    *n_members = nm;
    return nm > cap ? GD_E_CAPACITY : GD_OK;
}

int gd_ingest_bgzf(gd_ctx* c, int32_t tid, int32_t ref_id, const uint8_t* data, size_t n_bytes, uint64_t base_coffset,
                   const uint64_t* anchors, size_t n_anchors, uint64_t* n_records)
{
    if (int r = in_flight(c)) return r;
    if (!c || !data || !anchors || n_anchors == 0) return GD_E_INVALID;
    (void)gd_ingest_abort(c);                              // one-shot form: nothing else may be pending
    size_t nm = 0;
    int rc = gd_bgzf_members(data, n_bytes, 0, nullptr, nullptr, nullptr, nullptr, nullptr, &nm);
    if (rc != GD_OK && rc != GD_E_CAPACITY) return fail(c, GD_E_INVALID, "the range does not start with a BGZF member");
    if (nm == 0) return fail(c, GD_E_INVALID, "no complete BGZF member in the range");
    std::vector<uint64_t> moff(nm);
    std::vector<uint32_t> msize(nm), misize(nm), mcrc(nm);
    std::vector<uint16_t> mhdr(nm);
    if (gd_bgzf_members(data, n_bytes, nm, moff.data(), msize.data(), mhdr.data(), misize.data(), mcrc.data(), &nm) != GD_OK)
        return fail(c, GD_E_INVALID, "corrupt BGZF member table");
    if (int r = gd_ingest_begin(c, n_bytes, base_coffset, nm, moff.data(), msize.data(), mhdr.data(), misize.data(), mcrc.data()))
        return r;
    if (int r = gd_ingest_feed(c, data, n_bytes)) { (void)gd_ingest_abort(c); return r; }
    return gd_ingest_finish(c, tid, ref_id, anchors, n_anchors, n_records);
}
