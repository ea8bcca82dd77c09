// index_host.cpp -- `goleft-depth index`: a BAM's .bai made on the device.
//
//   goleft-depth index [-o OUT.bai] in.bam
//
// The host reads the header (bam_head.hpp, shared with covstats), feeds the file range after range (gd_ingest_begin /
// _feed_fd; ranges are cut at BGZF member boundaries, up to three are pending, and each begins with the last member of the
// one before, where the record the cut goes through nearly always starts) and lets the
// device find the record starts, walk the records and reduce them to runs, a linear index and per-reference counts
// (gd_index_begin / _decode / _result).  What is left for the host is the index arithmetic on the runs -- far fewer than
// records --: htslib's bin compression, the chunk merge, the backward fill and the file's layout (gdh_bai_assemble, plain
// C++: a CPU test drives it without a device).  The same bytes serve `goleft depth` on a BAM without an index
// (GOLEFT_GPU_INDEX=1: gdh::build_bai, nothing is written).
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
#include "gpu_ingest.hpp"
#include "index_build.hpp"

namespace {

constexpr uint32_t kPseudoBin = 37450;
constexpr uint64_t kUnset = ~0ull;

struct Chunk { uint64_t beg, end; };

int bin_level(uint32_t b) { return b >= 4681 ? 5 : b >= 585 ? 4 : b >= 73 ? 3 : b >= 9 ? 2 : b >= 1 ? 1 : 0; }

void put32(std::vector<uint8_t>* o, uint32_t v) { for (int k = 0; k < 4; ++k) o->push_back((uint8_t)(v >> (8 * k))); }
void put64(std::vector<uint8_t>* o, uint64_t v) { for (int k = 0; k < 8; ++k) o->push_back((uint8_t)(v >> (8 * k))); }

// One reference: its runs (file order) -> its bins after htslib's compression and chunk merge, ascending.
std::map<uint32_t, std::vector<Chunk>> reference_bins(const gd_index_run* runs, size_t n)
{
    std::map<uint32_t, std::vector<Chunk>> bins;
    for (size_t k = 0; k < n; ++k) bins[runs[k].bin].push_back(Chunk{runs[k].beg, runs[k].end});
    // level 5 up to level 1: a bin that spans fewer than 65536 compressed bytes moves into its parent -- if that exists
    for (int level = 5; level >= 1; --level) {
        std::vector<uint32_t> at;
        for (const auto& b : bins)
            if (bin_level(b.first) == level) at.push_back(b.first);
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

}  // namespace

extern "C" int64_t gdh_bai_assemble(int32_t n_ref, const gd_index_run* runs, size_t n_runs, const uint64_t* lin_off,
                                    const uint64_t* linear, const gd_index_ref* refs, uint64_t n_no_coor, uint8_t* out, size_t cap)
{
    if (n_ref < 0 || (n_runs && !runs) || (n_ref && (!lin_off || !refs))) return -1;
    for (size_t k = 0; k < n_runs; ++k)
        if (runs[k].ref < 0 || runs[k].ref >= n_ref || runs[k].bin >= kPseudoBin || (k && runs[k].ref < runs[k - 1].ref)) return -1;
    std::vector<uint8_t> o;
    o.insert(o.end(), {'B', 'A', 'I', 1});
    put32(&o, (uint32_t)n_ref);
    size_t k = 0;
    for (int32_t r = 0; r < n_ref; ++r) {
        const size_t first = k;
        while (k < n_runs && runs[k].ref == r) ++k;
        const std::map<uint32_t, std::vector<Chunk>> bins = k > first ? reference_bins(runs + first, k - first) : std::map<uint32_t, std::vector<Chunk>>();
        const bool has = refs[r].n_mapped + refs[r].n_unmapped > 0;
        put32(&o, (uint32_t)bins.size() + (has ? 1u : 0u));
        for (const auto& b : bins) {
            put32(&o, b.first);
            put32(&o, (uint32_t)b.second.size());
            for (const Chunk& c : b.second) { put64(&o, c.beg); put64(&o, c.end); }
        }
        if (has) {
            put32(&o, kPseudoBin);
            put32(&o, 2);
            put64(&o, refs[r].first_beg); put64(&o, refs[r].last_end); put64(&o, refs[r].n_mapped); put64(&o, refs[r].n_unmapped);
        }
        // the linear index: as far as the last touched window; an untouched window takes the value of the one behind it
        if (lin_off[r + 1] < lin_off[r] || (lin_off[r + 1] > lin_off[r] && !linear)) return -1;
        const uint64_t* const lin = linear + lin_off[r];
        uint64_t n_intv = lin_off[r + 1] - lin_off[r];
        while (n_intv && lin[n_intv - 1] == kUnset) --n_intv;
        put32(&o, (uint32_t)n_intv);
        const size_t at = o.size();
        o.resize(at + 8 * (size_t)n_intv);
        uint64_t behind = 0;
        for (uint64_t w = n_intv; w-- > 0;) {
            if (lin[w] != kUnset) behind = lin[w];
            for (int b = 0; b < 8; ++b) o[at + 8 * (size_t)w + (size_t)b] = (uint8_t)(behind >> (8 * b));
        }
    }
    put64(&o, n_no_coor);
    if (out && cap >= o.size()) memcpy(out, o.data(), o.size());
    return (int64_t)o.size();
}

namespace {

using gdh::cli::now_s;

struct Timing { double list = 0, feed = 0, decode = 0, read_back = 0, assemble = 0; int ranges = 0, rounds = 0; int64_t slices = 0, guesses = 0; };

}  // namespace

namespace gdh {

int build_bai(gd_ctx* ctx, const std::string& bam, std::vector<uint8_t>* out, std::string* err, IndexStats* stats)
{
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
    int rc = gd_index_begin(ctx, (int32_t)lengths.size(), lengths.data(), first_voff, fm.size);
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
    const int64_t need = gdh_bai_assemble((int32_t)lengths.size(), runs.data(), n_runs, lin_off.data(), linear.data(), refs.data(), n_no_coor, nullptr, 0);
    if (need < 0) { *err = "cannot assemble the index (internal error)"; return GD_E_INVALID; }
    out->resize((size_t)need);
    (void)gdh_bai_assemble((int32_t)lengths.size(), runs.data(), n_runs, lin_off.data(), linear.data(), refs.data(), n_no_coor, out->data(), out->size());
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

void usage(FILE* f) { fputs("usage: index [-o OUT.bai] in.bam\n", f); }

int env_int(const char* name, int dflt)
{
    const char* e = getenv(name);
    return e && *e ? atoi(e) : dflt;
}

}  // namespace

extern "C" int gdh_index_build(const char* bam, uint8_t** out, size_t* n_out, int64_t* stats, char* errbuf, size_t errcap)
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
        rc = gdh::build_bai(ctx, bam, &bytes, &err, &st);
    }
    if (errbuf && errcap) snprintf(errbuf, errcap, "%s", err.c_str());
    if (rc != GD_OK) return rc;
    if (stats) { stats[0] = st.records; stats[1] = st.rounds; stats[2] = st.ranges; }
    *out = static_cast<uint8_t*>(malloc(bytes.size() ? bytes.size() : 1));
    if (!*out) return GD_E_NOMEM;
    memcpy(*out, bytes.data(), bytes.size());
    *n_out = bytes.size();
    return GD_OK;
}

extern "C" void gdh_index_free(uint8_t* p) { free(p); }

extern "C" int gdh_index_run(int argc, const char* const* argv)
{
    using gdh::cli::Args;
    std::string out_path, bam;
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
        if (c.key != "-o" && c.key != "--output") { (void)c.fail("unknown argument %s", c.arg.c_str()); return 255; }
        if (!c.value()) return 255;
        out_path = c.val;
    }
    if (bam.empty()) { (void)c.fail("a BAM is required"); return 255; }
    if (out_path.empty()) out_path = bam + ".bai";
    uint8_t* bytes = nullptr;
    size_t n = 0;
    int64_t stats[3] = {0, 0, 0};
    char err[1024] = "";
    const int rc = gdh_index_build(bam.c_str(), &bytes, &n, stats, err, sizeof err);
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
