// index_host.cpp -- `goleft-depth index`: a BAM's .bai made on the device.
//
//   goleft-depth index [-c|--csi] [-m|--min-shift N] [-o OUT] in.bam
//
// The host reads the header (bam_head.hpp, shared with covstats), feeds the file range after range (gd_ingest_begin /
// _feed_fd; ranges are cut at BGZF member boundaries, up to three are pending, and each begins with the last member of the
// one before, where the record the cut goes through nearly always starts) and lets the
// device find the record starts, walk the records and reduce them to runs, a linear index and per-reference counts
// (gd_index_begin / _decode / _result).  What is left for the host is the index arithmetic on the runs -- far fewer than
// records --: htslib's bin compression, the chunk merge, the backward fill and the file's layout (gdh_bai_assemble, plain
// C++: a CPU test drives it without a device).  The same bytes serve `goleft depth` on a BAM without an index
// (GOLEFT_GPU_INDEX=1: gdh::build_index, nothing is written).  With -c the same runs, windows and counts become a .csi
// (DESIGN.md section 3.20): the binning scheme is a parameter of the walk and of the assembler, a .bai's is (14, 5).
#include <unistd.h>
#include <zlib.h>

#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../../../include/goleft_depth.h"
#include "../../../include/goleft_depth_host.h"
#include "bam_head.hpp"
#include "bam_reader.hpp"
#include "cli.hpp"
#include "csi_reader.hpp"
#include "gpu_ingest.hpp"
#include "index_build.hpp"

namespace {

constexpr uint64_t kUnset = ~0ull;

struct Chunk { uint64_t beg, end; };

// The binning scheme: bins whose smallest span 2^min_shift positions, `depth` levels below bin 0 (a .bai: 14 and 5).
uint32_t level_first(int level) { return (uint32_t)(((1ull << (3 * level)) - 1) / 7); }
uint32_t pseudo_bin(int depth) { return level_first(depth + 1) + 1; }             // 37450 at depth 5
int bin_level(uint32_t b, int depth)
{
    int level = depth;
    while (level > 0 && b < level_first(level)) --level;
    return level;
}

void put32(std::vector<uint8_t>* o, uint32_t v) { for (int k = 0; k < 4; ++k) o->push_back((uint8_t)(v >> (8 * k))); }
void put64(std::vector<uint8_t>* o, uint64_t v) { for (int k = 0; k < 8; ++k) o->push_back((uint8_t)(v >> (8 * k))); }

// One reference: its runs (file order) -> its bins after htslib's compression and chunk merge, ascending.
std::map<uint32_t, std::vector<Chunk>> reference_bins(const gd_index_run* runs, size_t n, int depth)
{
    std::map<uint32_t, std::vector<Chunk>> bins;
    for (size_t k = 0; k < n; ++k) bins[runs[k].bin].push_back(Chunk{runs[k].beg, runs[k].end});
    // the deepest level up to level 1: a bin that spans fewer than 65536 compressed bytes moves into its parent -- if that exists
    for (int level = depth; level >= 1; --level) {
        std::vector<uint32_t> at;
        for (const auto& b : bins)
            if (bin_level(b.first, depth) == level) at.push_back(b.first);
        for (uint32_t b : at) {
            std::vector<Chunk>& ch = bins[b];
            const uint32_t parent = (b - 1) >> 3;
            if ((ch.back().end >> 16) - (ch.front().beg >> 16) >= 65536) continue;
            auto p = bins.find(parent);
            if (p == bins.end()) continue;
            p->second.insert(p->second.end(), ch.begin(), ch.end());
            bins.erase(b);
        }
    }
    for (auto& b : bins) {
        std::vector<Chunk>& ch = b.second;
        std::stable_sort(ch.begin(), ch.end(), [](const Chunk& x, const Chunk& y) { return x.beg < y.beg; });
        size_t w = 0;
        for (size_t k = 1; k < ch.size(); ++k) {
            if ((ch[w].end >> 16) >= (ch[k].beg >> 16)) ch[w].end = std::max(ch[w].end, ch[k].end);
            else ch[++w] = ch[k];
        }
        ch.resize(w + 1);
    }
    return bins;
}

// Both layouts from one walk over the references: the bins (compressed and merged, ascending, the pseudo-bin last) and the
// linear array as far as its last touched window, an untouched window taking the value of the one behind it.  A .bai
// stores that array; a .csi stores, per real bin, the entry of the bin's first window (0 when that window lies behind the
// last touched one; the pseudo-bin: 0) and no array.
int64_t assemble(bool csi, int min_shift, int depth, int32_t n_ref, const gd_index_run* runs, size_t n_runs, const uint64_t* lin_off,
                 const uint64_t* linear, const gd_index_ref* refs, uint64_t n_no_coor, uint8_t* out, size_t cap)
{
    if (n_ref < 0 || (n_runs && !runs) || (n_ref && (!lin_off || !refs))) return -1;
    const uint32_t pseudo = pseudo_bin(depth);
    for (size_t k = 0; k < n_runs; ++k)
        if (runs[k].ref < 0 || runs[k].ref >= n_ref || runs[k].bin >= pseudo || (k && runs[k].ref < runs[k - 1].ref)) return -1;
    std::vector<uint8_t> o;
    if (csi) {
        o.insert(o.end(), {'C', 'S', 'I', 1});
        put32(&o, (uint32_t)min_shift);
        put32(&o, (uint32_t)depth);
        put32(&o, 0);                                                            // l_aux
    } else o.insert(o.end(), {'B', 'A', 'I', 1});
    put32(&o, (uint32_t)n_ref);
    std::vector<uint64_t> filled;
    size_t k = 0;
    for (int32_t r = 0; r < n_ref; ++r) {
        const size_t first = k;
        while (k < n_runs && runs[k].ref == r) ++k;
        const std::map<uint32_t, std::vector<Chunk>> bins = k > first ? reference_bins(runs + first, k - first, depth) : std::map<uint32_t, std::vector<Chunk>>();
        if (lin_off[r + 1] < lin_off[r] || (lin_off[r + 1] > lin_off[r] && !linear)) return -1;
        const uint64_t* const lin = linear + lin_off[r];
        uint64_t n_intv = lin_off[r + 1] - lin_off[r];
        while (n_intv && lin[n_intv - 1] == kUnset) --n_intv;
        filled.resize((size_t)n_intv);
        uint64_t behind = 0;
        for (uint64_t w = n_intv; w-- > 0;) {
            if (lin[w] != kUnset) behind = lin[w];
            filled[(size_t)w] = behind;
        }
        const bool has = refs[r].n_mapped + refs[r].n_unmapped > 0;
        put32(&o, (uint32_t)bins.size() + (has ? 1u : 0u));
        for (const auto& b : bins) {
            put32(&o, b.first);
            if (csi) {
                const int level = bin_level(b.first, depth);
                const uint64_t w = (uint64_t)(b.first - level_first(level)) << (3 * (depth - level));
                put64(&o, w < n_intv ? filled[(size_t)w] : 0);
            }
            put32(&o, (uint32_t)b.second.size());
            for (const Chunk& c : b.second) { put64(&o, c.beg); put64(&o, c.end); }
        }
        if (has) {
            put32(&o, pseudo);
            if (csi) put64(&o, 0);
            put32(&o, 2);
            put64(&o, refs[r].first_beg); put64(&o, refs[r].last_end); put64(&o, refs[r].n_mapped); put64(&o, refs[r].n_unmapped);
        }
        if (!csi) {
            put32(&o, (uint32_t)n_intv);
            for (uint64_t w = 0; w < n_intv; ++w) put64(&o, filled[(size_t)w]);
        }
    }
    put64(&o, n_no_coor);
    if (out && cap >= o.size()) memcpy(out, o.data(), o.size());
    return (int64_t)o.size();
}

// The payload as a BGZF file: members of at most 65280 payload bytes, then the empty member that ends such a file.
bool bgzf_write(const std::vector<uint8_t>& payload, std::vector<uint8_t>* out)
{
    static const uint8_t eof_member[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 27, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    out->clear();
    std::vector<uint8_t> buf(65536);
    for (size_t at = 0; at < payload.size();) {
        const size_t take = std::min<size_t>(payload.size() - at, 65280);
        z_stream z;
        memset(&z, 0, sizeof z);
        if (deflateInit2(&z, 6, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) != Z_OK) return false;
        z.next_in = const_cast<Bytef*>(payload.data() + at);
        z.avail_in = (uInt)take;
        z.next_out = buf.data();
        z.avail_out = (uInt)buf.size() - 26;                                     // (what the header and the trailer take)
        const int rc = deflate(&z, Z_FINISH);
        const size_t clen = buf.size() - 26 - z.avail_out;
        deflateEnd(&z);
        if (rc != Z_STREAM_END) return false;                                    // (65280 bytes never deflate to more than 65510)
        const uint8_t head[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};
        out->insert(out->end(), head, head + 16);
        const size_t bsize = clen + 25;                                          // the member's size - 1
        out->push_back((uint8_t)bsize);
        out->push_back((uint8_t)(bsize >> 8));
        out->insert(out->end(), buf.data(), buf.data() + clen);
        put32(out, (uint32_t)crc32(crc32(0L, Z_NULL, 0), payload.data() + at, (uInt)take));
        put32(out, (uint32_t)take);
        at += take;
    }
    out->insert(out->end(), eof_member, eof_member + 28);
    return true;
}

}  // namespace

extern "C" int64_t gdh_bai_assemble(int32_t n_ref, const gd_index_run* runs, size_t n_runs, const uint64_t* lin_off,
                                    const uint64_t* linear, const gd_index_ref* refs, uint64_t n_no_coor, uint8_t* out, size_t cap)
{
    return assemble(false, 14, 5, n_ref, runs, n_runs, lin_off, linear, refs, n_no_coor, out, cap);
}

extern "C" int64_t gdh_csi_assemble(int32_t n_ref, const gd_index_run* runs, size_t n_runs, const uint64_t* lin_off,
                                    const uint64_t* linear, const gd_index_ref* refs, uint64_t n_no_coor, int32_t min_shift, int32_t depth,
                                    uint8_t* out, size_t cap)
{
    if (min_shift < 8 || min_shift > 24 || depth < 0 || depth > 8) return -1;
    return assemble(true, min_shift, depth, n_ref, runs, n_runs, lin_off, linear, refs, n_no_coor, out, cap);
}

namespace {

using gdh::cli::now_s;

struct Timing { double list = 0, feed = 0, decode = 0, read_back = 0, assemble = 0; int ranges = 0, rounds = 0; int64_t slices = 0, guesses = 0; };

}  // namespace

namespace gdh {

int csi_depth(const std::vector<int64_t>& lengths, int min_shift)
{
    int64_t longest = 0;
    for (int64_t l : lengths) longest = std::max(longest, l);
    int depth = 0;
    while (longest + 256 > (1ll << (min_shift + 3 * depth))) ++depth;             // (htslib adds the 256)
    return depth;
}

int build_bai(gd_ctx* ctx, const std::string& bam, std::vector<uint8_t>* out, std::string* err, IndexStats* stats)
{
    return build_index(ctx, bam, IndexFormat::Bai, 14, out, err, stats);
}

int build_index(gd_ctx* ctx, const std::string& bam, IndexFormat format, int min_shift, std::vector<uint8_t>* out, std::string* err,
                IndexStats* stats)
{
    const bool csi = format == IndexFormat::Csi;
    if (csi && (min_shift < 8 || min_shift > 24)) { *err = "min_shift " + std::to_string(min_shift) + ": a .csi is made with 8 to 24"; return GD_E_INVALID; }
    Timing tm;
    const double t_enter = now_s();
    BamHead head;
    if (!read_bam_head(bam, &head, err)) return GD_E_INVALID;
    const std::vector<int64_t>& lengths = head.lengths;
    FileMap fm;
    if (!fm.open(bam)) { *err = "cannot open " + bam; return GD_E_INVALID; }
    auto lib_fail = [&](int rc) { *err = std::string(gd_strerror(rc)) + " (" + gd_last_error(ctx) + ")"; (void)gd_ingest_abort(ctx); return rc; };
    // compressed bytes per range (GOLEFT_INDEX_RANGE_BYTES: the tests cut files of a few kilobytes)
    uint64_t range_bytes = 128ull << 20;
    if (const char* e = getenv("GOLEFT_INDEX_RANGE_BYTES")) if (*e) range_bytes = (uint64_t)std::max<long long>(64, strtoll(e, nullptr, 10));
    // the member that holds the first record
    double t0 = now_s();
    uint64_t first_voff = 0;
    bool have_first = false;
    if (!first_record_voffset(fm.fd, fm.size, head.length, &first_voff, &have_first)) { *err = bam + ": not a BGZF file"; return GD_E_INVALID; }
    tm.list += now_s() - t0;
    const int depth = csi ? csi_depth(lengths, min_shift) : 5;
    int rc = csi ? gd_index_begin_csi(ctx, (int32_t)lengths.size(), lengths.data(), first_voff, fm.size, min_shift, depth)
                 : gd_index_begin(ctx, (int32_t)lengths.size(), lengths.data(), first_voff, fm.size);
    if (rc != GD_OK) return lib_fail(rc);
    gd_index_counts cnt{};
    if (have_first) {
        (void)gd_set_option(ctx, GD_OPT_INGEST_RANGE_HINT, (int64_t)std::min<uint64_t>(range_bytes, fm.size));
        // Up to three ranges are pending, as in the depth read: while the oldest is decoded the next two are read, uploaded
        // and inflated.  Where a range ends is known from its member headers alone, where its last whole record ends only
        // after its decode -- so the range behind it begins with its LAST MEMBER over again (64 KB read twice): the record
        // the cut goes through nearly always starts there.  When it starts further in front (a record longer than a member
        // cut by the range's end), what is pending is dropped and the feed starts over from that record.
        struct Range { uint64_t beg = 0, used = 0, last_member = 0; bool last = false; };
        auto announce = [&](uint64_t beg, uint64_t want, Range* r) -> int {
            for (;;) {
                const double ta = now_s();
                MemberTable mt;
                const bool listed = beg < fm.size && list_members_serial_fd(fm.fd, beg, (size_t)std::min<uint64_t>(want, fm.size - beg), &mt);
                if (listed && mt.n == 0 && want < fm.size - beg) { want *= 2; continue; }     // not one whole member in the range: a larger one
                if (!listed || mt.n == 0) {
                    *err = bam + ": truncated or damaged BGZF data at file offset " + std::to_string(beg);
                    (void)gd_ingest_abort(ctx);
                    return GD_E_INVALID;
                }
                r->beg = beg;
                r->used = mt.off[mt.n - 1] + mt.size[mt.n - 1];
                r->last_member = mt.off[mt.n - 1];
                r->last = beg + r->used >= fm.size;
                const double tb = now_s();
                int rc2 = gd_ingest_begin(ctx, r->used, beg, mt.n, mt.off.data(), mt.size.data(), mt.hdr.data(), mt.isize.data(), mt.crc.data());
                if (rc2 == GD_OK) rc2 = gd_ingest_feed_fd(ctx, fm.fd, beg, (size_t)r->used);
                if (rc2 != GD_OK) return lib_fail(rc2);
                tm.list += tb - ta; tm.feed += now_s() - tb;
                return GD_OK;
            }
        };
        std::deque<Range> pending;
        uint64_t voff = first_voff, want = range_bytes;
        for (;;) {
            if (pending.empty()) {
                Range r;
                if ((rc = announce(voff >> 16, want, &r)) != GD_OK) return rc;
                pending.push_back(r);
            }
            while (pending.size() < 3 && !pending.back().last && pending.back().last_member > 0) {
                Range r;
                if ((rc = announce(pending.back().beg + pending.back().last_member, range_bytes, &r)) != GD_OK) return rc;
                pending.push_back(r);
            }
            const Range cur = pending.front();
            pending.pop_front();
            const double tc = now_s();
            rc = gd_index_decode(ctx, cur.last ? 1 : 0, &cnt);
            if (rc != GD_OK) return lib_fail(rc);
            tm.decode += now_s() - tc;
            ++tm.ranges; tm.rounds += cnt.rounds; tm.slices += cnt.slices; tm.guesses += cnt.guesses;
            if (cur.last) break;
            if (!pending.empty() && (cnt.resume >> 16) >= pending.front().beg) { voff = cnt.resume; want = range_bytes; continue; }
            if (!pending.empty()) { (void)gd_ingest_abort(ctx); pending.clear(); }
            if (cnt.resume == voff) want *= 2;                    // not one whole record in the range: a larger one
            else { voff = cnt.resume; want = range_bytes; }
        }
    }
    // ---- what the device made of it, and the file's bytes --------------------------------------------------------
    t0 = now_s();
    size_t n_runs = 0, n_lin = 0;
    uint64_t n_no_coor = 0;
    rc = gd_index_result(ctx, nullptr, 0, &n_runs, nullptr, 0, &n_lin, nullptr, nullptr);
    if (rc != GD_OK) return lib_fail(rc);
    std::vector<gd_index_run> runs(n_runs);
    std::vector<uint64_t> linear(n_lin);
    std::vector<gd_index_ref> refs(lengths.size());
    rc = gd_index_result(ctx, runs.data(), n_runs, &n_runs, linear.data(), n_lin, &n_lin, refs.data(), &n_no_coor);
    if (rc != GD_OK) return lib_fail(rc);
    tm.read_back = now_s() - t0;
    t0 = now_s();
    std::vector<uint64_t> lin_off(lengths.size() + 1, 0);
    rc = gd_index_windows(ctx, lin_off.data(), lin_off.size());
    if (rc != GD_OK) return lib_fail(rc);
    if (lin_off.back() != n_lin) { *err = "the device's linear index has another size than expected (internal error)"; return GD_E_INVALID; }
    const int64_t need = assemble(csi, min_shift, depth, (int32_t)lengths.size(), runs.data(), n_runs, lin_off.data(), linear.data(), refs.data(), n_no_coor, nullptr, 0);
    if (need < 0) { *err = "cannot assemble the index (internal error)"; return GD_E_INVALID; }
    out->resize((size_t)need);
    (void)assemble(csi, min_shift, depth, (int32_t)lengths.size(), runs.data(), n_runs, lin_off.data(), linear.data(), refs.data(), n_no_coor, out->data(), out->size());
    if (csi) {                                                                   // a .csi is BGZF; a .bai is stored as it is
        std::vector<uint8_t> file;
        if (!bgzf_write(*out, &file)) { *err = "cannot compress the index (internal error)"; return GD_E_INVALID; }
        out->swap(file);
    }
    if (stats) { stats->min_shift = csi ? min_shift : 14; stats->depth = depth; }
    tm.assemble = now_s() - t0;
    if (stats) { stats->records = cnt.records; stats->rounds = tm.rounds; stats->ranges = tm.ranges; }
    if (getenv("GOLEFT_INDEX_TIMING")) {
        double lib[5] = {0, 0, 0, 0, 0}, ing[7] = {0, 0, 0, 0, 0, 0, 0};
        (void)gd_index_timing(ctx, lib, 5);
        (void)gd_ingest_timing(ctx, ing, 7);
        fprintf(stderr, "{\"index_s\": %.4f, \"records\": %" PRId64 ", \"ranges\": %d, \"slices\": %" PRId64 ", \"guesses\": %" PRId64 ", \"repair_rounds\": %d, "
                        "\"list_members_s\": %.4f, \"begin_feed_s\": %.4f, \"decode_s\": %.4f, \"read_s\": %.4f, \"wait_inflate_s\": %.4f, "
                        "\"guess_s\": %.4f, \"walks_s\": %.4f, \"runs_linear_s\": %.4f, \"device_read_back_s\": %.4f, \"result_s\": %.4f, \"assemble_s\": %.4f}\n",
                now_s() - t_enter, (int64_t)cnt.records, tm.ranges, tm.slices, tm.guesses, tm.rounds, tm.list, tm.feed, tm.decode, ing[0], lib[0],
                lib[1], lib[2], lib[3], lib[4], tm.read_back, tm.assemble);
    }
    return GD_OK;
}

}  // namespace gdh

namespace {

void usage(FILE* f)
{
    fputs("usage: index [-c|--csi] [-m|--min-shift N] [-o OUT] in.bam\n"
          "  -c  write a .csi (in.bam.csi) instead of a .bai: for references longer than 2^29 - 256\n"
          "  -m  the bits of the smallest bin's span, 8 to 24 (default 14); implies -c\n", f);
}

int env_int(const char* name, int dflt)
{
    const char* e = getenv(name);
    return e && *e ? atoi(e) : dflt;
}

}  // namespace

extern "C" int gdh_index_build(const char* bam, uint8_t** out, size_t* n_out, int64_t* stats, char* errbuf, size_t errcap)
{
    return gdh_index_build_csi(bam, 0, 14, out, n_out, stats, errbuf, errcap);
}

extern "C" int gdh_index_build_csi(const char* bam, int csi, int min_shift, uint8_t** out, size_t* n_out, int64_t* stats, char* errbuf, size_t errcap)
{
    if (!bam || !out || !n_out) return GD_E_INVALID;
    *out = nullptr;
    *n_out = 0;
    gdh::cli::Device ctx;
    std::string err;
    std::vector<uint8_t> bytes;
    gdh::IndexStats st;
    int rc = GD_E_NODEVICE;
    if (!ctx.open("index")) err = "no usable MI355X device";
    else {
        if (getenv("GOLEFT_INDEX_SLICE")) (void)gd_set_option(ctx, GD_OPT_INDEX_SLICE, env_int("GOLEFT_INDEX_SLICE", 65536));
        if (getenv("GOLEFT_INDEX_GUESS_CHECKS")) (void)gd_set_option(ctx, GD_OPT_INDEX_GUESS_CHECKS, env_int("GOLEFT_INDEX_GUESS_CHECKS", 3));
        if (getenv("GOLEFT_INDEX_REPAIR_ROUNDS")) (void)gd_set_option(ctx, GD_OPT_INDEX_REPAIR_ROUNDS, env_int("GOLEFT_INDEX_REPAIR_ROUNDS", 4));
        rc = gdh::build_index(ctx, bam, csi ? gdh::IndexFormat::Csi : gdh::IndexFormat::Bai, min_shift, &bytes, &err, &st);
    }
    if (errbuf && errcap) snprintf(errbuf, errcap, "%s", err.c_str());
    if (rc != GD_OK) return rc;
    if (stats) { stats[0] = st.records; stats[1] = st.rounds; stats[2] = st.ranges; }
    if (stats && csi) { stats[3] = st.min_shift; stats[4] = st.depth; }
    *out = static_cast<uint8_t*>(malloc(bytes.size() ? bytes.size() : 1));
    if (!*out) return GD_E_NOMEM;
    memcpy(*out, bytes.data(), bytes.size());
    *n_out = bytes.size();
    return GD_OK;
}

extern "C" void gdh_index_free(uint8_t* p) { free(p); }

extern "C" int gdh_csi_read(const uint8_t* bytes, size_t n, int32_t ref, int64_t* info, uint64_t* anchors, size_t cap, size_t* n_anchors,
                            char* errbuf, size_t errcap)
{
    gdh::CsiIndex x;
    std::string err;
    if (!bytes || !info) err = "no input";
    else if (gdh::read_csi_bytes(bytes, n, &x, &err) && ref >= (int32_t)x.anchors.size()) err = "no such reference";
    if (errbuf && errcap) snprintf(errbuf, errcap, "%s", err.c_str());
    if (!err.empty()) return GD_E_INVALID;
    info[0] = x.min_shift; info[1] = x.depth; info[2] = (int64_t)x.anchors.size(); info[3] = x.has_no_coor ? 1 : 0; info[4] = (int64_t)x.n_no_coor;
    if (n_anchors) *n_anchors = 0;
    if (ref < 0) return GD_OK;
    const std::vector<uint64_t>& v = x.anchors[(size_t)ref];
    info[5] = x.has_chunks[(size_t)ref]; info[6] = (int64_t)x.chunk_end[(size_t)ref];
    info[7] = x.n_mapped[(size_t)ref]; info[8] = x.n_unmapped[(size_t)ref];
    if (n_anchors) *n_anchors = v.size();
    if (anchors && cap < v.size()) return GD_E_CAPACITY;
    if (anchors && !v.empty()) memcpy(anchors, v.data(), v.size() * sizeof(uint64_t));
    return GD_OK;
}

extern "C" int gdh_index_run(int argc, const char* const* argv)
{
    using gdh::cli::Args;
    std::string out_path, bam;
    bool csi = false;
    int min_shift = 14;
    Args c(argc, argv, usage);
    for (;;) {
        const Args::Kind kind = c.next();
        if (kind == Args::End) break;
        if (kind == Args::Help) return 0;
        if (kind == Args::Positional) {
            if (!bam.empty()) { (void)c.fail("one BAM at a time"); return 255; }
            bam = c.arg;
            continue;
        }
        if (c.key == "-c" || c.key == "--csi") { csi = true; continue; }
        if (c.key == "-m" || c.key == "--min-shift") {
            if (!c.value()) return 255;
            char* end = nullptr;
            const long v = strtol(c.val.c_str(), &end, 10);
            if (c.val.empty() || *end || v < 8 || v > 24) { (void)c.fail("-m %s: min_shift is 8 to 24", c.val.c_str()); return 255; }
            min_shift = (int)v;
            csi = true;
            continue;
        }
        if (c.key != "-o" && c.key != "--output") { (void)c.fail("unknown argument %s", c.arg.c_str()); return 255; }
        if (!c.value()) return 255;
        out_path = c.val;
    }
    if (bam.empty()) { (void)c.fail("a BAM is required"); return 255; }
    if (out_path.empty()) out_path = bam + (csi ? ".csi" : ".bai");
    uint8_t* bytes = nullptr;
    size_t n = 0;
    int64_t stats[5] = {0, 0, 0, 0, 0};
    char err[1024] = "";
    const int rc = gdh_index_build_csi(bam.c_str(), csi ? 1 : 0, min_shift, &bytes, &n, stats, err, sizeof err);
    if (rc != GD_OK) {
        fprintf(stderr, "index: %s: %s\n", bam.c_str(), err[0] ? err : gd_strerror(rc));
        return rc == GD_E_UNSORTED ? 2 : 1;
    }
    // through a temporary file and a rename: a reader never sees half an index
    const std::string tmp = out_path + ".tmp." + std::to_string((long)getpid());
    FILE* f = fopen(tmp.c_str(), "wb");
    bool ok = f != nullptr;
    if (ok) ok = fwrite(bytes, 1, n, f) == n;
    if (f) ok = (fclose(f) == 0) && ok;
    if (ok) ok = rename(tmp.c_str(), out_path.c_str()) == 0;
    gdh_index_free(bytes);
    if (!ok) {
        (void)unlink(tmp.c_str());
        fprintf(stderr, "index: cannot write %s\n", out_path.c_str());
        return 1;
    }
    return 0;
}

extern "C" int gdh_index_main(int argc, const char* const* argv) { return gdh_index_run(argc, argv); }
