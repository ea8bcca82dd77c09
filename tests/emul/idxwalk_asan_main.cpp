// idxwalk_asan_main.cpp -- TEST INFRASTRUCTURE (tests/test_index_emul.py): the indexer's two readers of untrusted bytes --
// the candidate test of gd_bamguess.hpp and bam_walk<IndexWalk> of gd_bamdecode.hpp -- compiled for the host with
// -fsanitize=address,undefined and run lane by lane, the inflated stream, the member tables, the slot array and every
// per-segment table each ending exactly at an inaccessible page.  On the GPU a read one byte too far is silent; here it
// ends the process.
//
//   idxwalk_asan_main [--fuzz N] a.bam b.bam ...
//
// Per file: the stream is inflated and parsed directly (the truth); the guess kernel runs with slices of 64, 1000 and
// 65536 bytes and with 3 and 0 chain checks, and every guess made with 3 checks must be a record start on an intact stream;
// the walk runs from every 5th true record start and its slots must be what the direct parse says (reference, POS, end,
// bin, flag 4, virtual offset); then from the guesses, wrong ones included.  --fuzz N: N damaged copies (bytes flipped in
// the fields a walk trusts; every third copy truncated) go through guesses and walks, both with more of the file to
// follow and without: nothing is compared, the run must end.  Prints one line per file and "ok".
#include <zlib.h>

#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <random>
#include <string>

#include "emul_machine.hpp"
#include "../../goleft_amd/csrc/gd_bamguess.hpp"

namespace {

struct Member { uint64_t coff, out; };
struct Truth { int32_t ref, beg, end; uint32_t bin; uint64_t off; };

bool inflate_bam(const char* path, std::vector<uint8_t>* data, std::vector<Member>* mem)
{
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    std::vector<uint8_t> raw;
    uint8_t tmp[65536];
    size_t g;
    while ((g = fread(tmp, 1, sizeof tmp, f)) > 0) raw.insert(raw.end(), tmp, tmp + g);
    fclose(f);
    for (size_t p = 0; p + 18 <= raw.size();) {
        const uint8_t* h = raw.data() + p;
        if (h[0] != 0x1f || h[1] != 0x8b) return false;
        const size_t xlen = h[10] | (h[11] << 8), bsize = (size_t)(h[16] | (h[17] << 8)) + 1;   // (BC is the only subfield of these files)
        if (xlen != 6 || p + bsize > raw.size()) return false;
        const uint32_t isize = h[bsize - 4] | (h[bsize - 3] << 8) | (h[bsize - 2] << 16) | ((uint32_t)h[bsize - 1] << 24);
        mem->push_back(Member{p, data->size()});
        const size_t at = data->size();
        data->resize(at + isize);
        z_stream z{};
        if (inflateInit2(&z, -15) != Z_OK) return false;
        z.next_in = const_cast<uint8_t*>(h + 18); z.avail_in = (uInt)(bsize - 26);
        z.next_out = data->data() + at; z.avail_out = isize;
        const int rc = isize ? inflate(&z, Z_FINISH) : Z_STREAM_END;
        inflateEnd(&z);
        if (rc != Z_STREAM_END) return false;
        p += bsize;
    }
    return true;
}

uint32_t rd32(const uint8_t* p) { uint32_t v; memcpy(&v, p, 4); return v; }

const gd::GuessJob* g_guess = nullptr;
const gd::IdxWalkJob* g_walk = nullptr;
void body_guess() { gd::gd_bam_guess_kernel(*g_guess); }
void body_walk() { gd::gd_idx_walk_kernel(*g_walk); }

// A copy of n items of T that ends at a guard page.
template <class T>
struct Fenced {
    emul::Guarded g;
    T* p;
    size_t n;
    explicit Fenced(size_t count) : g((count ? count : 1) * sizeof(T)), p(reinterpret_cast<T*>(g.p)), n(count) {}
    Fenced(const std::vector<T>& v) : Fenced(v.size()) { if (!v.empty()) memcpy(p, v.data(), v.size() * sizeof(T)); }
};

struct Stream {
    std::vector<uint8_t> data;
    std::vector<Member> mem;
    std::vector<int32_t> ref_len;
    uint64_t first = 0;
};

std::vector<uint64_t> guesses(const Stream& s, uint64_t n_bytes, uint64_t slice, uint32_t checks)
{
    if (s.first >= n_bytes) return {};
    // (at most 400 slices from the stream's start: a lane is a fiber here, and a slice costs 64 of them)
    const size_t n_slice = (size_t)std::min<uint64_t>((n_bytes - s.first + slice - 1) / slice, 400);
    Fenced<uint8_t> d((size_t)n_bytes);
    memcpy(d.p, s.data.data(), (size_t)n_bytes);
    Fenced<int32_t> rl(s.ref_len);
    Fenced<uint64_t> out(n_slice);
    gd::GuessJob j{};
    j.data = d.p; j.n_bytes = n_bytes; j.first = s.first; j.slice = slice; j.n_slice = (uint32_t)n_slice; j.checks = checks;
    j.n_ref = (int32_t)s.ref_len.size(); j.ref_len = rl.p; j.guess = out.p;
    g_guess = &j;
    for (unsigned b = 0; b < n_slice; ++b) emul::run(body_guess, 64, b);
    std::vector<uint64_t> v;
    for (size_t k = 0; k < n_slice; ++k)
        if (out.p[k] != ~0ull && (v.empty() || out.p[k] > v.back())) v.push_back(out.p[k]);
    return v;
}

struct Walked { std::vector<gd::IdxRec> recs; std::vector<uint32_t> n_rec, flags; std::vector<uint64_t> end_off; };

// One walk per segment [beg[k], beg[k + 1]) (the last to n_bytes), the slots laid out as gd_api_index.inc lays them out.
Walked walk(const Stream& s, uint64_t n_bytes, const std::vector<uint64_t>& beg, uint32_t open_end)
{
    const size_t n = beg.size();
    Walked w;
    if (!n) return w;
    Fenced<uint8_t> d((size_t)n_bytes);
    memcpy(d.p, s.data.data(), (size_t)n_bytes);
    std::vector<uint64_t> mo, mc;
    for (const Member& m : s.mem)
        if (m.out < n_bytes || mo.empty()) { mo.push_back(m.out); mc.push_back(m.coff); }
    Fenced<uint64_t> f_mo(mo), f_mc(mc), f_beg(beg), f_end(n), f_slot(n), f_endoff(n);
    Fenced<uint32_t> f_nrec(n), f_flags(n);
    const uint64_t n_slots = (n_bytes - beg[0]) / 36 + n + 2;
    Fenced<gd::IdxRec> slots((size_t)n_slots);
    for (size_t k = 0; k < n; ++k) {
        f_end.p[k] = k + 1 < n ? beg[k + 1] : n_bytes;
        f_slot.p[k] = (beg[k] - beg[0]) / 36 + k;
    }
    gd::IdxWalkJob j{};
    j.data = d.p; j.n_bytes = n_bytes; j.seg_beg = f_beg.p; j.seg_end = f_end.p; j.slot_base = f_slot.p; j.n_seg = (uint32_t)n;
    j.open_end = open_end; j.slots = slots.p; j.n_slots = n_slots; j.n_rec = f_nrec.p; j.end_off = f_endoff.p; j.flags = f_flags.p;
    j.m_out = f_mo.p; j.m_coff = f_mc.p; j.n_mem = (uint32_t)mo.size(); j.n_ref = (int32_t)s.ref_len.size();
    g_walk = &j;
    for (unsigned b = 0; b < n; ++b) emul::run(body_walk, 64, b);
    for (size_t k = 0; k < n; ++k) {
        w.n_rec.push_back(f_nrec.p[k]); w.flags.push_back(f_flags.p[k]); w.end_off.push_back(f_endoff.p[k]);
        if (!(f_flags.p[k] & gd::BW_CORRUPT))
            for (uint32_t q = 0; q < f_nrec.p[k]; ++q) w.recs.push_back(slots.p[f_slot.p[k] + q]);
    }
    return w;
}

int fail(const char* path, const char* what) { fprintf(stderr, "%s: %s\n", path, what); return 1; }

int one_file(const char* path, int n_fuzz)
{
    Stream s;
    if (!inflate_bam(path, &s.data, &s.mem)) return fail(path, "cannot inflate");
    const std::vector<uint8_t>& d = s.data;
    if (d.size() < 12 || memcmp(d.data(), "BAM\1", 4) != 0) return fail(path, "not a BAM");
    uint64_t p = 8ull + rd32(d.data() + 4);
    const uint32_t n_ref = rd32(d.data() + p);
    p += 4;
    for (uint32_t r = 0; r < n_ref; ++r) {
        const uint32_t l_name = rd32(d.data() + p);
        s.ref_len.push_back((int32_t)rd32(d.data() + p + 4 + l_name));
        p += 8ull + l_name;
    }
    s.first = p;
    // ---- the truth -----------------------------------------------------------------------------------------------------
    std::vector<Truth> truth;
    while (p + 36 <= d.size()) {
        const uint32_t bs = rd32(d.data() + p);
        const uint8_t* r = d.data() + p + 4;
        Truth t{(int32_t)rd32(r), (int32_t)rd32(r + 4), 0, 0, p};
        const uint32_t l_name = r[8], n_cig = r[12] | (r[13] << 8), flag = r[14] | (r[15] << 8);
        uint64_t rlen = 0;
        for (uint32_t q = 0; q < n_cig; ++q) {
            const uint32_t op = rd32(r + 32 + l_name + 4 * q), k = op & 15;
            if (k == 0 || k == 2 || k == 3 || k == 7 || k == 8) rlen += op >> 4;
        }
        if ((flag & 4) || !rlen) rlen = 1;
        t.end = t.beg + 1;
        if (flag & 4) t.bin |= gd::IX_UNMAPPED;
        if (t.ref >= 0) { t.end = (int32_t)(t.beg + rlen); t.bin |= gd::bai_reg2bin((uint32_t)t.beg, (uint32_t)t.end); }
        truth.push_back(t);
        p += 4ull + bs;
    }
    if (p != d.size()) return fail(path, "the direct parse does not end with the stream");
    auto voff = [&](uint64_t o) {
        size_t k = s.mem.size();
        while (k-- > 0)
            if (s.mem[k].out <= o) break;
        return (s.mem[k].coff << 16) | (o - s.mem[k].out);
    };
    std::vector<char> is_start(d.size() + 1, 0);
    for (const Truth& t : truth) is_start[t.off] = 1;
    // ---- guesses on the intact stream --------------------------------------------------------------------------------------
    size_t n_guess = 0, n_wrong0 = 0;
    for (uint64_t slice : {64ull, 1000ull, 65536ull})
        for (uint32_t checks : {3u, 0u}) {
            const std::vector<uint64_t> g = guesses(s, d.size(), slice, checks);
            for (uint64_t o : g) {
                if (o >= d.size()) return fail(path, "a guess outside the stream");
                if (checks == 3 && !is_start[o]) return fail(path, "a guess with three chain checks that is no record start");
                if (checks == 0 && !is_start[o]) ++n_wrong0;
            }
            if (checks == 3) n_guess += g.size();
            // the walk from the guesses, wrong ones included: it must end inside its buffers
            const Walked w = walk(s, d.size(), g, 0);
            if (checks == 3 && !truth.empty()) {
                if (w.recs.size() != truth.size()) return fail(path, "the walk from true guesses lost records");
            }
        }
    // ---- the walk from true starts against the direct parse -----------------------------------------------------------------
    if (!truth.empty()) {
        std::vector<uint64_t> beg;
        for (size_t k = 0; k < truth.size(); k += 5) beg.push_back(truth[k].off);
        const Walked w = walk(s, d.size(), beg, 0);
        if (w.recs.size() != truth.size()) return fail(path, "record count");
        for (size_t k = 0; k < truth.size(); ++k) {
            const gd::IdxRec& c = w.recs[k];
            const Truth& t = truth[k];
            if (c.ref != t.ref || c.beg != t.beg || c.end != t.end || c.bin != t.bin || c.vbeg != voff(t.off)) return fail(path, "a slot differs from the direct parse");
        }
        for (size_t k = 0; k < beg.size(); ++k)
            if (w.flags[k] || w.end_off[k] != (k + 1 < beg.size() ? beg[k + 1] : d.size())) return fail(path, "a walk from a true start did not stop on the next one");
        // a stream cut inside its last record: with more to follow the walk stops in front of it, without it is damaged
        const uint64_t cut = truth.back().off + 20;
        const Walked wo = walk(s, cut, beg, 1), wc = walk(s, cut, beg, 0);
        if (wo.flags.back() || wo.end_off.back() != truth.back().off || wo.recs.size() != truth.size() - 1) return fail(path, "open end");
        if (!(wc.flags.back() & gd::BW_CORRUPT)) return fail(path, "closed end");
    }
    // ---- damaged copies -------------------------------------------------------------------------------------------------------
    std::mt19937_64 rng(12345);
    for (int c = 0; c < n_fuzz && !truth.empty(); ++c) {
        Stream m = s;
        for (int k = 0, nk = 1 + (int)(rng() % 5); k < nk; ++k) {
            const Truth& t = truth[rng() % truth.size()];
            static const int at[] = {0, 1, 2, 3, 4, 7, 8, 11, 12, 16, 17, 18, 20, 23, 24, 27, 28, 31, 36, 40, 44};
            const uint64_t o = t.off + (rng() % 4 ? (uint64_t)at[rng() % (sizeof at / sizeof at[0])] : rng() % 300);
            if (o < m.data.size()) m.data[o] = rng() % 3 ? (uint8_t)(m.data[o] ^ (1u << (rng() % 8))) : (uint8_t)rng();
        }
        uint64_t n_bytes = m.data.size();
        if (c % 3 == 2) n_bytes = s.first + 1 + rng() % (n_bytes - s.first);
        const uint64_t slice = c % 2 ? 64 : 4096;
        const std::vector<uint64_t> g = guesses(m, n_bytes, slice, c % 4 == 0 ? 0u : 3u);
        for (uint64_t o : g)
            if (o >= n_bytes) return fail(path, "a guess outside a damaged stream");
        (void)walk(m, n_bytes, g, (uint32_t)(c & 1));
    }
    printf("%s records %zu guesses %zu wrong_without_checks %zu\n", path, truth.size(), n_guess, n_wrong0);
    return 0;
}

}  // namespace

int main(int argc, char** argv)
{
    int n_fuzz = 0, a = 1;
    if (argc > 2 && std::string(argv[1]) == "--fuzz") { n_fuzz = atoi(argv[2]); a = 3; }
    for (; a < argc; ++a)
        if (one_file(argv[a], n_fuzz)) return 1;
    printf("ok\n");
    return 0;
}
