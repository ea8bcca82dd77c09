// gd_api_records.inc -- records into a context: the host worker pool, gd_acquire / gd_commit / gd_push / gd_reserve,
// gd_adopt_device, the index pass over what arrived and its verdicts, gd_reset (part of gd_api.hip, inside extern "C").

// Worker threads of a context (created by the first large gd_push / gd_commit, kept until gd_destroy): the staging blocks are filled by several threads (one core moves ~11 GB/s into pinned
// memory, a Gen5 x16 link takes five times that), block k + 1 while the copies of block k are on the link.
namespace {
struct FillPool {
    // COPY: plain copy.  POS: int32 positions, copied and checked (non-decreasing from `prev`, not negative).
    // OFFSETS: 32-bit CSR offsets, rebased by -sub and checked (non-decreasing from `prev`, as bits).  CHECK_POS /
    // CHECK_OFFSETS: the same checks alone (gd_commit: the caller filled the block itself).  PREAD: `bytes` from offset
    // `src` of the file descriptor `sub` (gd_ingest_feed_fd).
    enum Kind { COPY, POS, OFFSETS, CHECK_POS, CHECK_OFFSETS, PREAD };
    struct Item { void* dst; const void* src; size_t bytes; uint32_t sub; Kind kind; int32_t prev; };
    std::atomic<uint32_t> bad{0};
    std::vector<std::thread> th;
    std::vector<Item> items;
    std::atomic<size_t> next{0}, done{0};
    std::atomic<uint64_t> gen{0};
    std::atomic<bool> quit{false};
    std::mutex mu;
    std::condition_variable cv;
    // One branch-free pass the compiler vectorises, with and without the copy (`copy` is a literal where this is
    // inlined); != 0: out of order or negative.
    __attribute__((always_inline)) static uint32_t pass_pos(int32_t* __restrict__ d, const int32_t* __restrict__ s, size_t n, int32_t prev, bool copy)
    {
        uint32_t wrong = 0;
        if (n) { wrong = (uint32_t)(s[0] < prev) | (uint32_t)(s[0] < 0); if (copy) d[0] = s[0]; }
        for (size_t k = 1; k < n; ++k) { wrong |= (uint32_t)(s[k] < s[k - 1]); if (copy) d[k] = s[k]; }
        return wrong;
    }
    // (`prev` = the offset in front of this item: items that are copied are cut every 1 MB without overlap, and a dip
    // exactly at a cut -- possibly below `sub`, so that the rebased offset wraps -- must not pass; items that are only
    // checked overlap by one offset and give 0)
    __attribute__((always_inline)) static uint32_t pass_offsets(uint32_t* __restrict__ d, const uint32_t* __restrict__ s, size_t n, uint32_t prev, uint32_t sub, bool copy)
    {
        uint32_t wrong = 0;
        if (n) { wrong = (uint32_t)(s[0] < prev); if (copy) d[0] = s[0] - sub; }
        for (size_t k = 1; k < n; ++k) { wrong |= (uint32_t)(s[k] < s[k - 1]); if (copy) d[k] = s[k] - sub; }
        return wrong;
    }
    // != 0: the item failed its check (or its read)
    static uint32_t run_item(const Item& it)
    {
        const size_t n = it.bytes / 4;
        switch (it.kind) {
        case COPY: memcpy(it.dst, it.src, it.bytes); return 0;
        case POS: return pass_pos(static_cast<int32_t*>(it.dst), static_cast<const int32_t*>(it.src), n, it.prev, true);
        case CHECK_POS: return pass_pos(nullptr, static_cast<const int32_t*>(it.src), n, it.prev, false);
        case OFFSETS: return pass_offsets(static_cast<uint32_t*>(it.dst), static_cast<const uint32_t*>(it.src), n, (uint32_t)it.prev, it.sub, true);
        case CHECK_OFFSETS: return pass_offsets(nullptr, static_cast<const uint32_t*>(it.src), n, (uint32_t)it.prev, it.sub, false);
        case PREAD:
            for (size_t got = 0; got < it.bytes;) {
                const ssize_t r = pread((int)it.sub, static_cast<char*>(it.dst) + got, it.bytes - got,
                                        (off_t)(reinterpret_cast<uintptr_t>(it.src) + got));
                if (r <= 0) return 1;
                got += (size_t)r;
            }
            return 0;
        }
        return 1;
    }
    void drain()
    {
        for (;;) {
            const size_t i = next.fetch_add(1);
            if (i >= items.size()) break;
            if (run_item(items[i])) bad.store(1);
            done.fetch_add(1);
        }
    }
    std::atomic<int> active{0};
    // how long a worker spins for the next batch before it sleeps: gd_push's blocks follow each other within a fraction of a
    // millisecond (20 000); the pieces of a device BAM read are 2 ms apart, and fifteen workers spinning through that use up
    // CPU time a container's quota then takes from the threads that read the file (gd_ingest_feed_fd sets 500)
    std::atomic<int> spin_limit{20000};
    void start(int n)
    {
        for (int k = 0; k < n; ++k)
            th.emplace_back([this] {
                uint64_t seen = 0;
                for (;;) {
                    // the next block of a push follows within a fraction of a millisecond: spin that long before sleeping
                    // (a condition-variable wake-up costs tens of microseconds per worker and block)
                    for (int spin = 0; spin < spin_limit.load(std::memory_order_relaxed) && gen.load(std::memory_order_relaxed) == seen && !quit.load(std::memory_order_relaxed); ++spin)
                        __builtin_ia32_pause();
                    {
                        std::unique_lock<std::mutex> lk(mu);
                        cv.wait(lk, [&] { return quit.load() || gen.load() != seen; });
                        if (quit.load()) return;
                        seen = gen.load();
                        active.fetch_add(1);               // (under the lock: run() never swaps the items under a worker)
                    }
                    drain();
                    active.fetch_sub(1);
                }
            });
    }
    // runs the items on the workers and the calling thread; returns when all are done
    void run(std::vector<Item>&& work)
    {
        for (;;) {
            std::unique_lock<std::mutex> lk(mu);
            if (active.load() != 0) { lk.unlock(); std::this_thread::yield(); continue; }
            items = std::move(work);
            next.store(0); done.store(0);
            gen.fetch_add(1);
            break;
        }
        cv.notify_all();
        drain();
        while (done.load() < items.size()) std::this_thread::yield();
    }
    // The items on `pool`'s workers and the calling thread, or -- no pool: a small job -- on the calling thread alone;
    // != 0: an item failed.
    static uint32_t run_items(FillPool* pool, std::vector<Item>&& work)
    {
        if (!pool) {
            uint32_t wrong = 0;
            for (const Item& it : work) wrong |= run_item(it);
            return wrong;
        }
        pool->bad.store(0);
        pool->run(std::move(work));
        return pool->bad.load();
    }
    ~FillPool()
    {
        { std::lock_guard<std::mutex> lk(mu); quit.store(true); }
        cv.notify_all();
        for (auto& t : th) t.join();
    }
};

static void drop_pool(gd_ctx* c) { delete c->pool; c->pool = nullptr; c->pool_workers = 0; }

// the context's pool, with push_threads - 1 workers (the calling thread works too)
static FillPool* ctx_pool(gd_ctx* c)
{
    const int want = c->push_threads - 1;
    if (c->pool && c->pool_workers != want) { delete c->pool; c->pool = nullptr; }
    if (!c->pool && want > 0) {
        c->pool = new (std::nothrow) FillPool();
        if (c->pool) { c->pool->start(want); c->pool_workers = want; }
    }
    return c->pool;
}
}  // namespace


// gd_index_records_kernel over the reads [r0, r1) of a contig that are resident (or will be, in stream order) on `st`:
// position index (allocated on first use), spans, and -- check != 0 -- the record checks.
static int index_records(gd_ctx* c, ContigHost& h, size_t r0, size_t r1, int32_t prev_pos, bool check, hipStream_t st, bool committed = false)
{
    if (r1 <= r0) return GD_OK;
    const size_t n_idx = (size_t)(h.length >> 6) + 2;
    const bool idx = c->ingest_index && h.ridx_reads == r0;      // (an index with a hole is no index)
    if (idx && !h.ridx) HIPCHK(c, h.ridx.alloc(n_idx));
    if (!idx && !check) return GD_OK;
    gd::IndexJob j{};
    j.pos = h.pos; j.off = h.off; j.cigar = h.cigar;
    j.ridx = idx ? h.ridx.get() : nullptr;
    j.n_idx = (uint32_t)n_idx;
    j.out = c->d_ingest;
    j.bad_out = c->d_ingest + (committed ? 3 : 0);
    j.r0 = (uint32_t)r0; j.r1 = (uint32_t)r1;
    j.n_reads_total = (uint32_t)r1;
    j.n_ops_total = (uint32_t)std::min<size_t>(h.n_ops, 0xffffffffu);
    j.prev_pos = r0 ? prev_pos : -1;
    j.check = check ? 1u : 0u;
    // spans are measured for short-read shaped data only (a lane walks its read's ops one by one)
    j.walk_ops = (c->ingest_index && h.n_ops <= 6 * r1) ? 1u : 0u;          // (r1 = the contig's records once this block is in)
    hipLaunchKernelGGL(gd::gd_index_records_kernel, dim3((unsigned)((r1 - r0 + 255) / 256)), dim3(256), 0, st, j);
    HIPCHK(c, hipGetLastError());
    if (idx) h.ridx_reads = r1;
    if (j.walk_ops) c->ingest_span_dirty = true;
    return GD_OK;
}

// d_ingest's words on the host: a one-wave kernel stores them into page-locked memory and the stream is waited for -- no
// copy command (a device-to-host copy queues on the copy engine behind whatever a read in progress has put there).
static int read_ingest_words(gd_ctx* c, hipStream_t st, uint32_t (&w)[3])
{
    hipLaunchKernelGGL(gd::gd_copy_words_kernel, dim3(1), dim3(64), 0, st, c->d_ingest, c->h_ingest, 4u);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(st));
    w[0] = c->h_ingest[0]; w[1] = c->h_ingest[1]; w[2] = c->h_ingest[2];
    return GD_OK;
}

// GD_OPT_COMMIT_CHECK = 1: what the index pass found in the blocks committed since the last look (h_ingest[3], just read
// on a stream that is behind the copy stream).  A failure stays on the device word: the records are part of the contig,
// gd_compute keeps refusing until gd_reset.
static int commit_verdict(gd_ctx* c)
{
    c->commit_checks_pending = false;
    const uint32_t bad = c->h_ingest[3];
    if (!bad) return GD_OK;
    c->commit_checks_pending = true;
    const int lo = c->commit_tid_lo, hi = c->commit_tid_hi;
    if (bad & 4u) return fail(c, GD_E_RANGE, "contigs %d..%d: a committed record has a negative position (a placed BAM record has POS >= 0); gd_reset", lo, hi);
    if (bad & 1u) return fail(c, GD_E_UNSORTED, "contigs %d..%d: committed records are not coordinate sorted; gd_reset", lo, hi);
    return fail(c, GD_E_INVALID, "contigs %d..%d: cigar_off of committed records not monotone; gd_reset", lo, hi);
}

// The spans the index kernel has measured so far become the look-back of the next gd_compute (verified there as ever).
static void take_ingest_span(gd_ctx* c, int32_t span)
{
    c->ingest_span_dirty = false;
    if (span <= 0 || span == c->ingest_span) return;
    c->ingest_span = span;
    if (!c->lookback_pinned && span <= kAutoLongSpan) c->lookback = std::max(64, (span + 63) & ~63);
}

int gd_acquire(gd_ctx* c, size_t reads_cap, size_t ops_cap, gd_batch* out)
{
    if (!c || !out) return GD_E_INVALID;
    if (int r = set_device(c)) return r;
    // the cursor moves here, not at the commit: a producer may hold several blocks (its threads fill block k+1 while
    // block k is validated and committed); a slot that comes round while still held means every slot is out
    RingSlot& s = c->ring[c->ring_next];
    if (s.held)
        return fail(c, GD_E_STATE, "all %d staging blocks are held: gd_commit one (n_reads 0 gives it back unused)", kRingSlots);
    if (s.busy) {
        HIPCHK(c, hipEventSynchronize(s.done));
        s.busy = false;
    }
    if (reads_cap < 1) reads_cap = 1;
    if (ops_cap < 1) ops_cap = 1;
    if (s.b.reads_cap < reads_cap) {
        s.pos.reset(); s.flag.reset(); s.mapq.reset(); s.cigar_off.reset();
        s.b.pos = nullptr; s.b.flag = nullptr; s.b.mapq = nullptr; s.b.cigar_off = nullptr;
        s.b.reads_cap = 0;
        HIPCHK(c, s.pos.alloc(reads_cap));
        HIPCHK(c, s.flag.alloc(reads_cap));
        HIPCHK(c, s.mapq.alloc(reads_cap));
        HIPCHK(c, s.cigar_off.alloc(reads_cap + 1));
        s.b.pos = s.pos; s.b.flag = s.flag; s.b.mapq = s.mapq; s.b.cigar_off = s.cigar_off;
        s.b.reads_cap = reads_cap;
    }
    if (s.b.ops_cap < ops_cap) {
        s.cigar.reset();
        s.b.cigar = nullptr;
        s.b.ops_cap = 0;
        HIPCHK(c, s.cigar.alloc(ops_cap));
        s.b.cigar = s.cigar;
        s.b.ops_cap = ops_cap;
    }
    s.b.slot = c->ring_next;
    s.held = true;
    c->ring_next = (c->ring_next + 1) % kRingSlots;
    *out = s.b;
    return GD_OK;
}

static int commit_block(gd_ctx* c, const gd_batch* b, int32_t tid, size_t n_reads, size_t n_ops, bool validated);

int gd_commit(gd_ctx* c, const gd_batch* b, int32_t tid, size_t n_reads, size_t n_ops)
{
    return commit_block(c, b, tid, n_reads, n_ops, false);
}

// Makes room for n_reads / n_ops more records of a contig.  EXACT: in one step (a producer that knows its totals: gd_push,
// gd_reserve; growing geometrically block by block drains the copy pipeline at every step).  DOUBLING: at least twice
// what is there (gd_commit, block by block).  The arrays get exactly the capacity decided here (regrow_dev): what an array
// holds and what the contig believes it holds are one number.  A group that failed half way is finished by the next call.
enum class Growth { EXACT, DOUBLING };
static int reserve_records(gd_ctx* c, ContigHost& h, size_t n_reads, size_t n_ops, Growth g)
{
    const size_t need_r = h.n_reads + n_reads, need_o = h.n_ops + n_ops;
    const size_t cap_r = h.cap_reads();
    if (need_r > cap_r) {
        const size_t ncap = g == Growth::DOUBLING ? std::max(need_r, cap_r * 2) : need_r;
        if (h.pos.cap() < ncap) if (int r = regrow_dev(c, h.pos, ncap, true, h.n_reads)) return r;
        if (h.flag.cap() < ncap) if (int r = regrow_dev(c, h.flag, ncap, true, h.n_reads)) return r;
        if (h.mapq.cap() < ncap) if (int r = regrow_dev(c, h.mapq, ncap, true, h.n_reads)) return r;
        if (h.off.cap() < ncap + 1) if (int r = regrow_dev(c, h.off, ncap + 1, true, h.n_reads ? h.n_reads + 1 : 0)) return r;
    }
    if (need_o > h.cigar.cap()) {
        const size_t ncap = g == Growth::DOUBLING ? std::max(need_o, h.cigar.cap() * 2) : need_o;
        if (int r = regrow_dev(c, h.cigar, ncap, true, h.n_ops)) return r;
    }
    return GD_OK;
}

static int commit_block(gd_ctx* c, const gd_batch* b, int32_t tid, size_t n_reads, size_t n_ops, bool validated)
{
    if (int r = in_flight(c)) return r;
    if (!c || !b) return GD_E_INVALID;
    if (int r = set_device(c)) return r;
    if (b->slot < 0 || b->slot >= kRingSlots || c->ring[b->slot].b.pos != b->pos)
        return fail(c, GD_E_INVALID, "batch was not obtained from gd_acquire");
    RingSlot& s = c->ring[b->slot];
    if (!s.held) return fail(c, GD_E_STATE, "batch was committed already");
    s.held = false;                                      // (whatever happens below, the block goes back to the ring)
    if (tid < 0 || (size_t)tid >= c->contigs.size()) return fail(c, GD_E_RANGE, "tid %d out of range", tid);
    if (n_reads > b->reads_cap || n_ops > b->ops_cap) return fail(c, GD_E_INVALID, "batch overflow");
    if (n_reads == 0) return GD_OK;
    ContigHost& h = c->contigs[tid];
    if (h.adopted) return fail(c, GD_E_STATE, "contig %d holds adopted device records", tid);
    if (b->cigar_off[0] != 0 || b->cigar_off[n_reads] != n_ops)
        return fail(c, GD_E_INVALID, "cigar_off must start at 0 and end at n_ops");
    if ((uint64_t)h.n_ops + n_ops > 0xffffffffull)
        return fail(c, GD_E_RANGE, "more than 2^32 CIGAR ops on contig %d", tid);
    if ((uint64_t)h.n_reads + n_reads >= kMaxReadsPerContig)
        return fail(c, GD_E_RANGE, "more than 2^30 records on contig %d", tid);
    // coordinate order (BAM SO:coordinate) is what makes the tile search valid.  The common case -- nothing
    // wrong -- is three branch-free passes the compiler vectorises (a 12.6 M-record chromosome: ~2 ms instead of
    // ~13 ms for the record-by-record loop, which was a quarter of the whole host-to-results path); only a block
    // that fails them is walked again to say where.
    int32_t last = h.last_pos;
    const bool on_device = !validated && c->commit_check_device && c->h2d_kernel && n_reads >= 4096;
    if (validated) last = b->pos[n_reads - 1];           // (gd_push: its filler threads checked the block while copying)
    else if (on_device) {
        // the seam with what is there already is looked at here; the rest by the index pass once the block has landed
        if (b->pos[0] < 0) return fail(c, GD_E_RANGE, "contig %d record %zu: negative position %d (a placed BAM record has POS >= 0)", tid, (size_t)h.n_reads, b->pos[0]);
        if (b->pos[0] < last) return fail(c, GD_E_UNSORTED, "contig %d record %zu: pos %d < %d", tid, (size_t)h.n_reads, b->pos[0], last);
        last = b->pos[n_reads - 1];
    } else {
        const int32_t* const p = b->pos;
        const uint32_t* const o = b->cigar_off;
        // pieces of 64 k records: positions non-decreasing (from the record before), offsets non-decreasing -- a large
        // block's go to the context's worker threads, a small one's run right here (no list, no allocation)
        FillPool* const pool = n_reads >= (1u << 18) ? ctx_pool(c) : nullptr;
        std::vector<FillPool::Item> work;
        uint32_t bad = (uint32_t)(p[0] < 0);                 // sorted: p[0] is the smallest
        const size_t piece = 1u << 16;
        for (size_t a = 0; a < n_reads; a += piece) {
            const size_t e = std::min(n_reads, a + piece);
            const FillPool::Item ip{nullptr, p + a, (e - a) * 4, 0u, FillPool::CHECK_POS, a ? p[a - 1] : last};
            const FillPool::Item io{nullptr, o + a, (e - a + 1) * 4, 0u, FillPool::CHECK_OFFSETS, 0};
            if (pool) { work.push_back(ip); work.push_back(io); }
            else bad |= FillPool::run_item(ip) | FillPool::run_item(io);
        }
        if (pool) bad |= FillPool::run_items(pool, std::move(work));
        if (bad) {
            for (size_t i = 0; i < n_reads; ++i) {
                if (p[i] < 0) return fail(c, GD_E_RANGE, "contig %d record %zu: negative position %d (a placed BAM record has POS >= 0)", tid, h.n_reads + i, p[i]);
                if (p[i] < last) return fail(c, GD_E_UNSORTED, "contig %d record %zu: pos %d < %d", tid, h.n_reads + i, p[i], last);
                if (o[i + 1] < o[i]) return fail(c, GD_E_INVALID, "cigar_off not monotone");
                last = p[i];
            }
        }
        last = p[n_reads - 1];
    }
    // the CSR offsets are rebased to the contig stream: on the way by the copy kernel, else here
    const uint32_t base = (uint32_t)h.n_ops;
    const bool blit = c->h2d_kernel && n_reads >= 4096;
    if (base && !blit) {
        uint32_t* __restrict__ const o = b->cigar_off;
        for (size_t i = 0; i <= n_reads; ++i) o[i] += base;
    }
    if (int r = reserve_records(c, h, n_reads, n_ops, Growth::DOUBLING)) return r;
    hipStream_t cs = c->copy_stream;
    if (blit) {
        // one launch: workgroups read the page-locked block over the link (gd_stage.hpp)
        gd::H2DJob j{};
        j.off_add = base;
        j.seg[0] = {h.pos + h.n_reads, b->pos, n_reads * sizeof(int32_t)};
        j.seg[1] = {h.off + h.n_reads, b->cigar_off, (n_reads + 1) * sizeof(uint32_t)};
        j.seg[2] = {h.cigar + h.n_ops, b->cigar, n_ops * sizeof(uint32_t)};
        j.seg[3] = {h.flag + h.n_reads, b->flag, n_reads * sizeof(uint16_t)};
        j.seg[4] = {h.mapq + h.n_reads, b->mapq, n_reads * sizeof(uint8_t)};
        hipLaunchKernelGGL(gd::gd_h2d_kernel, dim3(c->h2d_grid), dim3(256), 0, cs, j);
        HIPCHK(c, hipGetLastError());
    } else {
        HIPCHK(c, hipMemcpyAsync(h.pos + h.n_reads, b->pos, n_reads * sizeof(int32_t), hipMemcpyHostToDevice, cs));
        HIPCHK(c, hipMemcpyAsync(h.flag + h.n_reads, b->flag, n_reads * sizeof(uint16_t), hipMemcpyHostToDevice, cs));
        HIPCHK(c, hipMemcpyAsync(h.mapq + h.n_reads, b->mapq, n_reads * sizeof(uint8_t), hipMemcpyHostToDevice, cs));
        HIPCHK(c, hipMemcpyAsync(h.off + h.n_reads, b->cigar_off, (n_reads + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, cs));
        if (n_ops)
            HIPCHK(c, hipMemcpyAsync(h.cigar + h.n_ops, b->cigar, n_ops * sizeof(uint32_t), hipMemcpyHostToDevice, cs));
    }
    {
        // the block is part of the contig's stream now (in copy-stream order): index it, measure its spans
        const size_t r0 = h.n_reads;
        const int32_t before = h.last_pos;
        h.n_ops += n_ops;                                  // (index_records reads the contig's totals)
        const int ri = index_records(c, h, r0, r0 + n_reads, before, on_device, cs, true);
        h.n_ops -= n_ops;
        if (ri) return ri;
    }
    HIPCHK(c, hipEventRecord(s.done, cs));
    s.busy = true;
    if (h.ck_ok) {                          // the long-read structures no longer cover the stream
        HIPCHK(c, hipStreamSynchronize(c->stream));
        drop_ck(h);
    }
    h.n_reads += n_reads;
    h.n_ops += n_ops;
    h.last_pos = last;
    c->computed = false;
    if (on_device) {
        if (!c->commit_checks_pending) { c->commit_tid_lo = c->commit_tid_hi = tid; c->commit_checks_pending = true; }
        c->commit_tid_lo = std::min(c->commit_tid_lo, tid);
        c->commit_tid_hi = std::max(c->commit_tid_hi, tid);
    }
    return GD_OK;
}

int gd_check_commits(gd_ctx* c)
{
    if (!c) return GD_E_INVALID;
    if (int r = in_flight(c)) return r;
    if (!c->commit_checks_pending) return GD_OK;
    if (int r = set_device(c)) return r;
    uint32_t w[3];
    if (int r = read_ingest_words(c, c->copy_stream, w)) return r;
    return commit_verdict(c);
}

int gd_push(gd_ctx* c, int32_t tid, const int32_t* pos, const uint16_t* flag, const uint8_t* mapq,
            const uint32_t* cigar_off, const uint32_t* cigar, size_t n_reads, size_t n_ops)
{
    if (!c) return GD_E_INVALID;
    if (n_reads == 0) return GD_OK;
    if (!pos || !flag || !mapq || !cigar_off || (n_ops && !cigar)) return GD_E_INVALID;
    if (tid < 0 || (size_t)tid >= c->contigs.size()) return fail(c, GD_E_RANGE, "tid %d out of range", tid);
    if (int r = in_flight(c)) return r;
    if (int r = set_device(c)) return r;
    {
        ContigHost& h = c->contigs[tid];
        if (h.adopted) return fail(c, GD_E_STATE, "contig %d holds adopted device records", tid);
        if (cigar_off[n_reads] > n_ops) return fail(c, GD_E_INVALID, "cigar_off out of range");
        if (int r = reserve_records(c, h, n_reads, cigar_off[n_reads] - cigar_off[0], Growth::EXACT)) return r;   // one allocation, not one per doubling
    }
    const size_t chunk = c->push_chunk;   // records per staging block (kRingSlots blocks: one being filled, the others on the link)
    FillPool* const pool = n_reads >= (1u << 18) ? ctx_pool(c) : nullptr;   // (small pushes run on the calling thread)
    const size_t piece = 1u << 20;   // bytes per work item
    size_t i = 0;
    while (i < n_reads) {
        size_t n = std::min(chunk, n_reads - i);
        size_t o0 = cigar_off[i], o1 = cigar_off[i + n];
        if (o1 < o0 || o1 > n_ops) return fail(c, GD_E_INVALID, "cigar_off out of range");
        gd_batch b;
        if (int r = gd_acquire(c, n, o1 - o0, &b)) return r;
        std::vector<FillPool::Item> work;
        const int32_t before = i ? pos[i - 1] : c->contigs[tid].last_pos;
        auto add = [&](void* dst, const void* src, size_t bytes, uint32_t sub, FillPool::Kind kind) {
            for (size_t at = 0; at < bytes; at += piece) {
                FillPool::Item it{static_cast<char*>(dst) + at, static_cast<const char*>(src) + at, std::min(piece, bytes - at), sub, kind, 0};
                if (kind == FillPool::POS) it.prev = at ? reinterpret_cast<const int32_t*>(static_cast<const char*>(src) + at)[-1] : before;
                if (kind == FillPool::OFFSETS) it.prev = at ? reinterpret_cast<const int32_t*>(static_cast<const char*>(src) + at)[-1] : (int32_t)sub;
                work.push_back(it);
            }
        };
        add(b.pos, pos + i, n * sizeof(int32_t), 0, FillPool::POS);                             // copied and checked: sorted, not negative
        add(b.flag, flag + i, n * sizeof(uint16_t), 0, FillPool::COPY);
        add(b.mapq, mapq + i, n * sizeof(uint8_t), 0, FillPool::COPY);
        add(b.cigar_off, cigar_off + i, (n + 1) * sizeof(uint32_t), (uint32_t)o0, FillPool::OFFSETS);   // block relative; checked: non-decreasing
        if (o1 > o0) add(b.cigar, cigar + o0, (o1 - o0) * sizeof(uint32_t), 0, FillPool::COPY);
        // a block that failed a check goes through gd_commit's own validation, which says where
        const bool checked = FillPool::run_items(pool, std::move(work)) == 0;
        if (int r = commit_block(c, &b, tid, n, o1 - o0, checked)) return r;
        i += n;
    }
    return GD_OK;
}

int gd_reserve(gd_ctx* c, int32_t tid, size_t n_reads, size_t n_ops)
{
    if (!c) return GD_E_INVALID;
    if (int r = in_flight(c)) return r;
    if (int r = set_device(c)) return r;
    if (tid < 0 || (size_t)tid >= c->contigs.size()) return fail(c, GD_E_RANGE, "tid %d out of range", tid);
    ContigHost& h = c->contigs[tid];
    if (h.adopted) return fail(c, GD_E_STATE, "contig %d holds adopted device records", tid);
    if ((uint64_t)h.n_ops + n_ops > 0xffffffffull) return fail(c, GD_E_RANGE, "more than 2^32 CIGAR ops on contig %d", tid);
    if ((uint64_t)h.n_reads + n_reads >= kMaxReadsPerContig) return fail(c, GD_E_RANGE, "more than 2^30 records on contig %d", tid);
    return reserve_records(c, h, n_reads, n_ops, Growth::EXACT);
}

int gd_adopt_device(gd_ctx* c, int32_t tid, const gd_batch* d, size_t n_reads, size_t n_ops)
{
    if (int r = in_flight(c)) return r;
    if (!c || !d) return GD_E_INVALID;
    if (int r = set_device(c)) return r;
    if (tid < 0 || (size_t)tid >= c->contigs.size()) return fail(c, GD_E_RANGE, "tid %d out of range", tid);
    if (n_reads && (!d->pos || !d->flag || !d->mapq || !d->cigar_off)) return GD_E_INVALID;
    if (n_ops > 0xffffffffull) return fail(c, GD_E_RANGE, "more than 2^32 CIGAR ops");
    // depth <= records of the contig; the window reduction adds four depths in 32 bits
    if (n_reads >= kMaxReadsPerContig) return fail(c, GD_E_RANGE, "more than 2^30 records on one contig");
    // The arrays are checked and indexed right away, on this context's stream: whatever
    // stream of the caller produced them must have finished.  A device-wide wait makes that true for
    // any producer (a few microseconds per contig, at ingest time).
    HIPCHK(c, hipDeviceSynchronize());
    ContigHost& h = c->contigs[tid];
    ContigHost t;                                          // the new stream, checked before the old one is let go
    t.length = h.length;
    t.pos.borrow(d->pos, n_reads); t.flag.borrow(d->flag, n_reads); t.mapq.borrow(d->mapq, n_reads);   // (the caller frees them)
    t.off.borrow(d->cigar_off, n_reads + 1); t.cigar.borrow(d->cigar, n_ops);
    t.n_reads = n_reads; t.n_ops = n_ops;
    t.adopted = true;
    if (n_reads) {
        // what gd_commit checks on a host block, here in one pass over pos / cigar_off on the device -- the same pass
        // leaves the position index and the largest span (gd_index_records_kernel)
        uint32_t w[3] = {0, 0, 0};
        int r = GD_OK;
        if (hipMemsetAsync(c->d_ingest, 0, sizeof(uint32_t), c->stream) != hipSuccess) r = fail(c, GD_E_HIP, "hipMemsetAsync failed");
        if (r == GD_OK) r = index_records(c, t, 0, n_reads, -1, true, c->stream);
        if (r == GD_OK) r = read_ingest_words(c, c->stream, w);
        if (r == GD_OK) {
            const uint32_t bad = w[0];
            if (bad & 4u) r = fail(c, GD_E_RANGE, "contig %d: a device record has a negative position (a placed BAM record has POS >= 0)", tid);
            else if (bad & 1u) r = fail(c, GD_E_UNSORTED, "contig %d: device records not coordinate sorted", tid);
            else if (bad & 2u) r = fail(c, GD_E_INVALID, "contig %d: CSR offsets of the device records are not a non-decreasing sequence from 0 to at most %zu", tid, n_ops);
        }
        if (r != GD_OK) { free_contig(t); return r; }      // (the contig keeps what it held)
        t.last_pos = (int32_t)w[2];
        take_ingest_span(c, (int32_t)w[1]);
    }
    free_contig(h);
    h = std::move(t);
    c->computed = false;
    return GD_OK;
}

int gd_reset(gd_ctx* c)
{
    if (int r = in_flight(c)) return r;
    if (!c) return GD_E_INVALID;
    if (int r = set_device(c)) return r;
    (void)gd_ingest_abort(c);                              // a device BAM read in progress (its reader thread) ends here
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipStreamSynchronize(c->copy_stream));
    for (auto& h : c->contigs) free_contig(h);             // (the lengths stay)
    c->bounds.clear();
    return forget_records_state(c);
}
