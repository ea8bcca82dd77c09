// gd_bamdecode.hpp -- BAM records -> the engine's SoA arrays and covstats' record slots, on the device.
//
// Second stage of the device-side BAM read (after gd_inflate.hpp; replaces the decode every
// `samtools depth` child performs, depth/depth.go:45 of the reference).  BAM records are
// self-delimiting only forwards (block_size prefix), so a stream cannot be entered at an
// arbitrary byte -- but the .bai linear index stores the virtual offset of a record start
// for every 16 kb of reference (SAMv1 section 5.2: ioffset).  Those are the anchors: one
// wave walks the records from one anchor to the next, so a chromosome offers thousands of
// independent walks.
//   bam_walk<P>            THE walk: everything that trusts a length field of the file, once; a policy P says what a
//                          record is worth.  Compiles for the host (tests/emul/bamwalk_emul.cpp: behind guard pages)
//   gd_bam_walk_kernel<false>  DepthWalk: per segment records and CIGAR ops (CG:B,I tags resolved), first / last position,
//                          a sortedness flag; stops at the contig's end; leaves the table of record starts
//   gd_bam_extract_tab_kernel  a thread per record of that table -- no chain, no LDS, no barrier -- writing pos / flag /
//                          mapq / cigar_off / cigar at the segment's base (exclusive prefix sums of the counts, host side)
//   gd_bam_walk_kernel<true>   the same walk a second time, extracting (when no table fits)
//   gd_cs_walk_kernel      CsWalk: every record of a range, across references, to a CsRec slot (gd_covstats.hpp)
//   gd_idx_walk_kernel     IndexWalk: every record of a range to an IdxRec slot -- what a .bai is made of (gd_baiindex.hpp);
//                          its segments begin at GUESSED record starts (gd_bamguess.hpp), so a corrupt walk is no verdict
//                          before the host has confirmed the segment's start (gd_api_index.inc)
// Only the fields `samtools depth -Q q` consults are extracted.
#pragma once

namespace gd {

struct BamSegJob {
    const uint8_t* data;           // inflated bytes
    uint64_t n_bytes;
    const uint64_t* seg_beg;       // [n_seg] byte offset of the first record of the segment
    const uint64_t* seg_end;       // [n_seg] where the walk stops (next anchor, or n_bytes)
    int32_t  tid;                  // records of another reference end the contig
    int32_t  n_ref;                // references of the file: a sorted BAM goes on with tid < refID < n_ref, or -1
    uint32_t n_seg;
    // count pass
    uint32_t* n_rec;               // [n_seg]
    uint64_t* n_ops;               // [n_seg]
    int32_t*  first_pos;           // [n_seg] (0x7fffffff when empty)
    int32_t*  last_pos;            // [n_seg]
    uint32_t* flags;               // [n_seg] BW_* below
    // extract pass
    const uint64_t* rec_base;      // [n_seg] first record index of the segment
    const uint64_t* op_base;       // [n_seg] first op index
    int32_t*  pos;
    uint16_t* flag;
    uint8_t*  mapq;
    uint32_t* cigar_off;           // [n_records + 1]; [n_records] is written by the host
    uint32_t* cigar;
    // the record table (null: none).  Written by the count pass, read by gd_bam_extract_tab_kernel: two words per record,
    // {start - seg_beg[s], ops of the segment in front of it}, segment s at entry tab_base[s] (room for (seg_end - seg_beg)
    // / 36 + 1 records: a record is 36 bytes at least; the host keeps segments under 4 GB)
    uint32_t* tab;
    const uint64_t* tab_base;      // [n_seg]
};

// One record as covstats' sampling loop sees it.
struct CsRec {
    uint32_t flag;
    int32_t  pos, next_pos, tlen;
    uint32_t mlen;                  // the length of the only CIGAR op when that op is M, else CS_NOT_M
    uint32_t pad;
    uint64_t qlen;                  // query length of the stored CIGAR: M, I, S, =, X
};
constexpr uint32_t CS_NOT_M = 0xffffffffu;

struct CsWalkJob {
    const uint8_t* data;            // inflated bytes of the range
    uint64_t n_bytes;
    const uint64_t* seg_beg;        // [n_seg] first record of the segment
    const uint64_t* seg_end;        // [n_seg] next anchor (the last segment: n_bytes)
    const uint64_t* slot_base;      // [n_seg] first slot of the segment in `slots` (room for a record per 36 bytes)
    uint32_t n_seg;
    uint32_t open_end;              // more of the file follows: the last segment may end in a record cut by the range's end
    CsRec* slots;
    uint32_t* n_rec;                // [n_seg]
    uint64_t* end_off;              // [n_seg] where the walk stopped
    uint32_t* flags;                // [n_seg] BW_CORRUPT, BW_OVERRAN
};

// What a walk reports per segment (`flags` of both jobs): positions go backwards inside it; a record that cannot be one;
// the walk ran past seg_end (an anchor that is no record start); a record of another reference ended the walk before
// seg_end; ... and the reference resumes within the next 64 records.
enum : uint32_t { BW_UNSORTED = 1u, BW_CORRUPT = 2u, BW_OVERRAN = 4u, BW_LEFT_REF = 8u, BW_REF_RESUMES = 16u };

__device__ __forceinline__ uint32_t ld32(const uint8_t* p)
{
    uint32_t v;
    __builtin_memcpy(&v, p, 4);    // records are not aligned
    return v;
}

// The CIGAR of the record body r (block_size bytes): the stored one, or the CG:B,I tag's when the
// stored one is the <l_seq>S<ref_len>N placeholder (SAMv1 4.2.2).  false: corrupt.
__device__ __forceinline__ bool bam_record_cigar(const uint8_t* r, uint32_t block_size, const uint8_t** cg_out,
                                                 uint32_t* n_out)
{
    const uint32_t l_read_name = r[8];
    uint32_t n_cigar = (uint32_t)r[12] | ((uint32_t)r[13] << 8);
    const uint32_t l_seq = ld32(r + 16);
    if (32ull + l_read_name + 4ull * n_cigar > block_size) return false;
    const uint8_t* cg = r + 32 + l_read_name;
    if (n_cigar == 2 && (ld32(cg) & 0xf) == 4 && (ld32(cg) >> 4) == l_seq && (ld32(cg + 4) & 0xf) == 3) {
        const uint8_t* end = r + block_size;
        const uint8_t* t = cg + 8 + (l_seq + 1) / 2 + l_seq;
        while (t + 3 <= end) {
            const uint8_t t0 = t[0], t1 = t[1], ty = t[2];
            t += 3;
            uint32_t sz = 0;
            if (ty == 'A' || ty == 'c' || ty == 'C') sz = 1;
            else if (ty == 's' || ty == 'S') sz = 2;
            else if (ty == 'i' || ty == 'I' || ty == 'f') sz = 4;
            else if (ty == 'Z' || ty == 'H') { while (t < end && *t) ++t; ++t; continue; }
            else if (ty == 'B') {
                if (t + 5 > end) break;
                const uint8_t sub = t[0];
                const uint32_t cnt = ld32(t + 1);
                t += 5;
                const uint32_t es = (sub == 'c' || sub == 'C') ? 1 : (sub == 's' || sub == 'S') ? 2 : 4;
                if (t0 == 'C' && t1 == 'G' && sub == 'I' && t + 4ull * cnt <= end) { cg = t; n_cigar = cnt; break; }
                t += (uint64_t)es * cnt;
                continue;
            } else break;
            t += sz;
        }
    }
    *cg_out = cg;
    *n_out = n_cigar;
    return true;
}

// ONE WAVE PER SEGMENT.  Records are self-delimiting only forwards, so finding where they start is a chain of
// dependent reads.  Round 3 gave each segment ONE LANE, which followed that chain with a load from HBM per record and
// then extracted the record itself -- 3 300 records in a row per segment of a 30x chromosome, every lane of a wave in
// a different place.  Here the wave stages 3 KB of the stream in LDS with coalesced 16-byte loads, lane 0 follows the
// block_size chain THERE (an LDS round trip per record) and notes up to 32 record starts, and then every lane takes one
// record -- CIGAR resolved (CG:B,I), fields extracted -- with the round's records' memory latencies in flight at once.
// Output positions inside a round come from the op counts the lanes leave in LDS.  Measured with the page-locked walk
// tables of gd_api_ingest.inc (the two changes were made together): the counting walk of a chromosome-sized range
// 17 -> 10 ms, the extracting one 18 -> 6 ms (scope iii).
// LDS: 3 KB of stream + 0.5 KB of tables.  Not more: the walks run BESIDE the inflate kernel of the next range, whose six
// workgroups per CU leave 4 KB of LDS -- a walk workgroup that needs more waits for an inflate workgroup to retire.
constexpr int BW_WIN = 3072;           // bytes of the stream staged per round
constexpr int BW_REC = 32;             // records per round at most (one lane each)

// What lane 0 does with the record the chain stands on: a lane extracts it; stepped over; the walk ends in front of it.
enum BwStep { BW_TAKE, BW_SKIP, BW_END };

// bam_walk<P>: it owns the window, the block_size chain's frame and the barriers of a round; the policy P (DepthWalk for
// the depth read, CsWalk for covstats) says what a record is worth:
//   HEAD / HOLD   bytes of a record that must lie inside the window / that the stream must hold before the chain reads it
//   begin         every lane, before the first round            cut     lane 0: flags of a record the stream holds in part
//   step          lane 0: the record at `off`, header h[] (LDS) record  a lane's work on its record; false: corrupt
//   emit          every lane, after the round's record() calls  finish  lane 0: the segment's results
template <class P, class Job>
__device__ __forceinline__ void bam_walk(const Job& j, P p)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_win[BW_WIN];
    __shared__ uint64_t s_off[BW_REC];     // stream offsets of the round's records
    __shared__ uint64_t s_wbase;           // where the next window begins (16-byte aligned)
    __shared__ uint32_t s_n, s_done;       // records of this round; the segment is finished
    __shared__ __attribute__((aligned(16))) uint8_t s_bad[BW_REC];   // the lane's record is corrupt (a byte each: read back as four words)
    const uint32_t s = blockIdx.x;
    if (s >= j.n_seg) return;
    const uint32_t lane = threadIdx.x;
    const uint64_t stop = j.seg_end[s];
    uint64_t off = j.seg_beg[s];           // lane 0's walk state
    uint32_t fl = 0;
    p.begin(j, s);
    if (lane == 0) { s_wbase = off & ~15ull; s_done = off < stop ? 0u : 1u; s_n = 0; }
    if (lane < (uint32_t)BW_REC) s_bad[lane] = 0;
    __syncthreads();
    while (s_done == 0u) {
        // ---- (1) the window: [wbase, wbase + BW_WIN), bytes past the stream read as zero ----
        const uint64_t wbase = s_wbase;
        for (uint32_t i = lane; i < BW_WIN / 16; i += 64) {
            const uint64_t a = wbase + 16ull * i;
            // (two words in registers, the stream's last bytes gathered one by one: a local array copied with a runtime
            // length is an alloca, which the compiler moves to LDS -- a kilobyte per workgroup on top of the 3.4 KB below)
            uint64_t w[2] = {0, 0};
            if (a + 16 <= j.n_bytes) __builtin_memcpy(w, j.data + a, 16);
            else
                for (uint64_t k = a; k < j.n_bytes; ++k) {
                    const uint64_t b = (uint64_t)j.data[k] << (8u * (uint32_t)((k - a) & 7u));
                    if (k - a < 8) w[0] |= b; else w[1] |= b;
                }
            __builtin_memcpy(s_win + 16u * i, w, 16);
        }
        __syncthreads();
        // ---- (2) lane 0: the block_size chain, in LDS ----
        if (lane == 0) {
            uint32_t k = 0, done = 0;
            while (k < (uint32_t)BW_REC) {
                if (off >= stop) { done = 1; break; }
                const uint64_t rel = off - wbase;
                if (rel + P::HEAD > (uint64_t)BW_WIN) break;                // the record's header lies in the next window
                if (off + P::HOLD > j.n_bytes) { fl |= p.cut(j, s); done = 1; break; }
                const uint32_t block_size = ld32(s_win + rel);
                if (block_size < 32) { fl |= BW_CORRUPT; done = 1; break; }
                if (off + 4 + block_size > j.n_bytes) { fl |= p.cut(j, s); done = 1; break; }
                const BwStep st = p.step(j, s_win + rel, off, stop, fl);
                if (st == BW_END) { done = 1; break; }
                if (st == BW_TAKE) s_off[k++] = off;
                off += 4ull + block_size;
            }
            if (!done && off >= stop) done = 1;
            s_n = k;
            s_done = done;
            s_wbase = off & ~15ull;
        }
        __syncthreads();
        // ---- (3) one record per lane ----
        const uint32_t n = s_n;
        if (lane < n) s_bad[lane] = p.record(j, s, lane, s_off[lane], wbase, s_win) ? 0 : 1;
        __syncthreads();
        uint64_t b[BW_REC / 8];
        __builtin_memcpy(b, s_bad, BW_REC);
        const bool bad = (b[0] | b[1] | b[2] | b[3]) != 0;                  // a corrupt record: the host refuses the file
        if (bad && lane == 0) { fl |= BW_CORRUPT; s_done = 1; }
        p.emit(j, s, lane, n, s_off, bad);
        __syncthreads();                                                    // (s_done above; and nobody still reads what the next round overwrites)
    }
    if (lane == 0) {
        if (off > stop) fl |= BW_OVERRAN;                                   // an anchor that is not a record start
        p.finish(j, s, off, fl);
    }
}

// The depth read: the records of ONE reference (j.tid), placed ones only, sorted; the walk ends at the first record of
// another reference.  !EXTRACT counts (and leaves the record table), EXTRACT writes the contig's arrays.
template <bool EXTRACT>
struct DepthWalk {
    static constexpr uint32_t HEAD = 16;   // block_size, refID, POS
    static constexpr uint32_t HOLD = 36;   // the smallest record
    uint32_t* s_nc;                        // [BW_REC] LDS: op counts of the round's records
    uint32_t nrec = 0;                     // lane 0's
    uint64_t nops = 0;
    int32_t first = 0x7fffffff, last = -0x7fffffff;
    uint64_t ri = 0, oi = 0;               // every lane: where the round's output begins; its record, and the CIGAR of it
    const uint8_t *r = nullptr, *cg = nullptr;
    uint32_t nc = 0;

    __device__ __forceinline__ void begin(const BamSegJob& j, uint32_t s) { if (EXTRACT) { ri = j.rec_base[s]; oi = j.op_base[s]; } }
    __device__ __forceinline__ uint32_t cut(const BamSegJob&, uint32_t) const { return BW_CORRUPT; }
    __device__ __forceinline__ BwStep step(const BamSegJob& j, const uint8_t* h, uint64_t off, uint64_t stop, uint32_t& fl)
    {
        const int32_t ref_id = (int32_t)ld32(h + 4);
        if (ref_id != j.tid) {
            // the contig's records end here -- in a sorted BAM.  `samtools depth -r` stops at the first record of
            // another reference and so does this walk; that the reference does not RESUME is checked over the next
            // records up to the segment's end (at most 64: one damaged refID is caught, a contig's true end costs
            // nothing), and by the host across segments (BW_LEFT_REF)
            fl |= BW_LEFT_REF;
            if (!(ref_id == -1 || (ref_id > j.tid && ref_id < j.n_ref))) { fl |= BW_CORRUPT; return BW_END; }   // not a refID a sorted BAM holds here: a damaged record (or a walk out of step)
            if (!EXTRACT) {
                uint64_t o2 = off;
                for (int q = 0; q < 64 && o2 < stop; ++q) {
                    if (o2 + 36 > j.n_bytes) break;
                    const uint32_t bs = ld32(j.data + o2);
                    if (bs < 32 || o2 + 4 + bs > j.n_bytes) break;
                    if ((int32_t)ld32(j.data + o2 + 4) == j.tid) { fl |= BW_REF_RESUMES; break; }
                    o2 += 4ull + bs;
                }
            }
            return BW_END;
        }
        const int32_t pos = (int32_t)ld32(h + 8);
        // POS -1 is BAM's "no position": a record filed under the reference but not placed on it (what `samtools
        // depth` drops through the 0x4 flag such a record carries) is not part of the contig's stream
        if (pos < 0) return BW_SKIP;
        if (nrec && pos < last) fl |= BW_UNSORTED;
        if (nrec == 0) first = pos;
        last = pos;
        ++nrec;
        return BW_TAKE;
    }
    // the record's CIGAR (the stored one or the CG tag's): its op count to LDS
    __device__ __forceinline__ bool record(const BamSegJob& j, uint32_t, uint32_t lane, uint64_t o, uint64_t wbase, const uint8_t* s_win)
    {
        r = j.data + o + 4;
        // the counting walk needs the op count alone, and the record's fixed fields and stored CIGAR are nearly always
        // inside the window it was found in: read there, it costs no trip to memory (block_size, refID, POS and
        // l_read_name lie inside by the chain's own condition); the CG:B,I placeholder and records that leave the
        // window go the long way
        const uint32_t rel = (uint32_t)(o - wbase);
        const uint32_t l_read_name = s_win[rel + 12u];
        bool ok, near = false;
        if (!EXTRACT && rel + 44u + l_read_name <= (uint32_t)BW_WIN) {
            const uint32_t block_size = ld32(s_win + rel);
            const uint32_t n_cigar = (uint32_t)s_win[rel + 16u] | ((uint32_t)s_win[rel + 17u] << 8);
            const uint32_t c0 = ld32(s_win + rel + 36u + l_read_name), c1 = ld32(s_win + rel + 40u + l_read_name);
            const bool placeholder = n_cigar == 2u && (c0 & 0xfu) == 4u && (c0 >> 4) == ld32(s_win + rel + 20u) && (c1 & 0xfu) == 3u;
            if (!placeholder) { near = true; ok = 32ull + l_read_name + 4ull * n_cigar <= block_size; nc = n_cigar; }
        }
        if (!near) ok = bam_record_cigar(r, ld32(j.data + o), &cg, &nc);
        s_nc[lane] = ok ? nc : 0u;
        return ok;
    }
    __device__ __forceinline__ void emit(const BamSegJob& j, uint32_t s, uint32_t lane, uint32_t n, const uint64_t* s_off, bool bad)
    {
        uint64_t before = 0, total = 0;                                     // ops of the round's records in front of this lane's; of all
        for (uint32_t q = 0; q < n; ++q) {
            if (q < lane) before += s_nc[q];
            total += s_nc[q];
        }
        const bool mine = !bad && lane < n;                                 // (nothing is written for a round with a corrupt record)
        if (mine && !EXTRACT && j.tab) {
            uint32_t* const e = j.tab + 2ull * (j.tab_base[s] + ri + lane);
            e[0] = (uint32_t)(s_off[lane] - j.seg_beg[s]);
            e[1] = (uint32_t)(oi + before);
        } else if (mine && EXTRACT) {
            const uint64_t rr = ri + lane, oo = oi + before;
            j.pos[rr] = (int32_t)ld32(r + 4);
            j.mapq[rr] = r[9];
            j.flag[rr] = (uint16_t)((uint32_t)r[14] | ((uint32_t)r[15] << 8));
            j.cigar_off[rr] = (uint32_t)oo;
            for (uint32_t q = 0; q < nc; ++q) j.cigar[oo + q] = ld32(cg + 4 * (uint64_t)q);
        }
        ri += n;
        oi += total;
        if (lane == 0) nops += total;
    }
    __device__ __forceinline__ void finish(const BamSegJob& j, uint32_t s, uint64_t, uint32_t fl) const
    {
        if (EXTRACT) return;
        j.n_rec[s] = nrec;
        j.n_ops[s] = nops;
        j.first_pos[s] = first;
        j.last_pos[s] = last;
        j.flags[s] = fl;
    }
};

template <bool EXTRACT>
__global__ __launch_bounds__(64) void gd_bam_walk_kernel(BamSegJob j)
{
    __shared__ uint32_t s_nc[BW_REC];
    bam_walk(j, DepthWalk<EXTRACT>{s_nc});
}

// covstats: EVERY record of the range in file order -- across references and through the unplaced tail -- each to a CsRec
// slot of its segment.  The range's last segment may end in a record the range holds only in part.
struct CsWalk {
    static constexpr uint32_t HEAD = 4;    // block_size
    static constexpr uint32_t HOLD = 4;
    uint64_t ri = 0;                       // records of the segment so far (every lane's copy)

    __device__ __forceinline__ void begin(const CsWalkJob&, uint32_t) {}
    // a record the range holds only in part: the next range begins with it (the last segment of a range that is not the
    // file's last); anywhere else the bytes are damaged
    __device__ __forceinline__ uint32_t cut(const CsWalkJob& j, uint32_t s) const
    {
        return s + 1 == j.n_seg && j.open_end ? 0u : (uint32_t)BW_CORRUPT;
    }
    // no refID test: covstats reads every record
    __device__ __forceinline__ BwStep step(const CsWalkJob&, const uint8_t*, uint64_t, uint64_t, uint32_t&) { return BW_TAKE; }
    __device__ __forceinline__ bool record(const CsWalkJob& j, uint32_t s, uint32_t lane, uint64_t o, uint64_t, const uint8_t*)
    {
        const uint32_t block_size = ld32(j.data + o);
        const uint8_t* const r = j.data + o + 4;
        const uint32_t l_read_name = r[8];
        const uint32_t n_cigar = (uint32_t)r[12] | ((uint32_t)r[13] << 8);
        CsRec c{(uint32_t)r[14] | ((uint32_t)r[15] << 8), (int32_t)ld32(r + 4), (int32_t)ld32(r + 24), (int32_t)ld32(r + 28), CS_NOT_M, 0, 0};
        const bool ok = 32ull + l_read_name + 4ull * n_cigar <= block_size;
        if (ok) {
            // the STORED CIGAR: the reference reads with everything variable-length but the CIGAR omitted, so a
            // CG:B,I tag is not resolved and the <l_seq>S<ref_len>N placeholder counts as it stands
            const uint8_t* const cg = r + 32 + l_read_name;
            for (uint32_t q = 0; q < n_cigar; ++q) {
                const uint32_t op = ld32(cg + 4ull * q), t = op & 0xfu;
                if (t == 0u || t == 1u || t == 4u || t == 7u || t == 8u) c.qlen += op >> 4;
            }
            if (n_cigar == 1u) {
                const uint32_t op = ld32(cg);
                if ((op & 0xfu) == 0u) c.mlen = op >> 4;
            }
        }
        j.slots[j.slot_base[s] + ri + lane] = c;
        return ok;
    }
    __device__ __forceinline__ void emit(const CsWalkJob&, uint32_t, uint32_t, uint32_t n, const uint64_t*, bool) { ri += n; }
    __device__ __forceinline__ void finish(const CsWalkJob& j, uint32_t s, uint64_t off, uint32_t fl) const
    {
        j.n_rec[s] = (uint32_t)ri;
        j.end_off[s] = off;
        j.flags[s] = fl;
    }
};

__global__ __launch_bounds__(64) void gd_cs_walk_kernel(CsWalkJob j) { bam_walk(j, CsWalk{}); }

// One record as the indexer sees it (SAMv1 5.2; DESIGN.md section 3.19, rules 1 and 2).
struct IdxRec {
    int32_t  ref;                   // refID (-1: unplaced)
    int32_t  beg;                   // POS as stored
    int32_t  end;                   // POS + the reference length of the STORED CIGAR; POS + 1 when unmapped or that length is 0
    uint32_t bin;                   // reg2bin(beg, end) | IX_UNMAPPED | IX_BADSPAN
    uint64_t vbeg;                  // virtual offset of the record's first byte
};
constexpr uint32_t IX_UNMAPPED = 1u << 31;   // flag 0x4
constexpr uint32_t IX_BADSPAN = 1u << 30;    // placed, and POS < 0 or end beyond the geometry's limit (2^29 for a .bai): end is POS + 1 then
constexpr uint32_t IX_BIN = 0x3fffffffu;     // every bin of a geometry the API accepts (depth <= 8) lies below bit 30

// The bin of [beg, end) in a binning scheme whose smallest bins span 2^min_shift positions, `depth` levels below bin 0
// (a .bai: 14 and 5): from the deepest level up, the first level at which both ends share a bin.
__device__ __forceinline__ uint32_t idx_reg2bin(uint32_t beg, uint32_t end, uint32_t min_shift, uint32_t depth)
{
    --end;
    uint32_t s = min_shift;
    uint32_t first = (uint32_t)(((1ull << (3u * depth)) - 1ull) / 7ull);     // the first bin of level `depth`
    for (uint32_t l = depth; l > 0u; --l) {
        if ((uint32_t)((uint64_t)beg >> s) == (uint32_t)((uint64_t)end >> s)) return first + (uint32_t)((uint64_t)beg >> s);
        s += 3u;
        first = (first - 1u) >> 3;
    }
    return 0u;
}

__device__ __forceinline__ uint32_t bai_reg2bin(uint32_t beg, uint32_t end) { return idx_reg2bin(beg, end, 14u, 5u); }   // SAMv1 5.3

struct IdxWalkJob {
    const uint8_t* data;            // inflated bytes of the range
    uint64_t n_bytes;
    const uint64_t* seg_beg;        // [n_seg] where the segment's walk begins: a record start, or a guess at one
    const uint64_t* seg_end;        // [n_seg] the next guess (the range's last segment: n_bytes)
    const uint64_t* slot_base;      // [n_seg] first slot of the segment
    uint32_t n_seg;
    uint32_t open_end;              // more of the file follows: the segment that ends with the range may end in a cut record
    IdxRec* slots;
    uint64_t n_slots;               // nothing is written at or behind this slot
    uint32_t* n_rec;                // [n_seg]
    uint64_t* end_off;              // [n_seg] where the walk stopped: the first record start at or behind seg_end
    uint32_t* flags;                // [n_seg] BW_CORRUPT
    const uint64_t* m_out;          // [n_mem] the range's members: exclusive sums of their ISIZE (m_out[0] = 0)
    const uint64_t* m_coff;         // [n_mem] ... and their file offsets
    uint32_t n_mem;
    int32_t  n_ref;
    uint32_t min_shift = 14, depth = 5;   // the binning scheme (as initialised: a .bai's)
    int64_t  max_end = 1ll << 29;   // a placed record may end here and no further: min(2^(min_shift + 3 depth), 2^31 - 1)
};

struct IndexWalk {
    static constexpr uint32_t HEAD = 4;
    static constexpr uint32_t HOLD = 4;
    uint64_t ri = 0;

    __device__ __forceinline__ void begin(const IdxWalkJob&, uint32_t) {}
    // a record the range holds only in part ends the walk in front of it (end_off < seg_end tells the host).  In ANY segment:
    // the guesses behind a cut record lie inside it, so the segment that meets it need not be the last
    __device__ __forceinline__ uint32_t cut(const IdxWalkJob& j, uint32_t) const { return j.open_end ? 0u : (uint32_t)BW_CORRUPT; }
    __device__ __forceinline__ BwStep step(const IdxWalkJob&, const uint8_t*, uint64_t, uint64_t, uint32_t&) { return BW_TAKE; }
    __device__ __forceinline__ bool record(const IdxWalkJob& j, uint32_t s, uint32_t lane, uint64_t o, uint64_t, const uint8_t*)
    {
        const uint32_t block_size = ld32(j.data + o);
        const uint8_t* const r = j.data + o + 4;
        const uint32_t l_read_name = r[8];
        const uint32_t n_cigar = (uint32_t)r[12] | ((uint32_t)r[13] << 8);
        const uint32_t flag = (uint32_t)r[14] | ((uint32_t)r[15] << 8);
        IdxRec c{(int32_t)ld32(r), (int32_t)ld32(r + 4), 0, 0u, 0ull};
        const bool ok = 32ull + l_read_name + 4ull * n_cigar <= block_size && c.ref >= -1 && c.ref < j.n_ref;
        if (ok) {
            uint64_t rlen = 0;                               // the STORED CIGAR: M D N = X (a CG:B,I tag is not consulted)
            const uint8_t* const cg = r + 32 + l_read_name;
            for (uint32_t q = 0; q < n_cigar; ++q) {
                const uint32_t op = ld32(cg + 4ull * q), t = op & 0xfu;
                if (t == 0u || t == 2u || t == 3u || t == 7u || t == 8u) rlen += op >> 4;
            }
            if ((flag & 4u) || rlen == 0) rlen = 1;
            const int64_t end = (int64_t)c.beg + (int64_t)rlen;
            c.end = c.beg + 1;
            if (flag & 4u) c.bin |= IX_UNMAPPED;
            if (c.ref >= 0) {
                if (c.beg < 0 || end > j.max_end) c.bin |= IX_BADSPAN;
                else { c.end = (int32_t)end; c.bin |= idx_reg2bin((uint32_t)c.beg, (uint32_t)end, j.min_shift, j.depth); }
            }
            // the member that holds byte o: the last one that begins at or before it (of several: the one with bytes)
            uint32_t lo = 0, hi = j.n_mem;                   // m_out[lo] <= o < m_out[hi]
            while (hi - lo > 1u) {
                const uint32_t mid = lo + (hi - lo) / 2u;
                if (j.m_out[mid] <= o) lo = mid; else hi = mid;
            }
            c.vbeg = (j.m_coff[lo] << 16) | (o - j.m_out[lo]);
        }
        const uint64_t at = j.slot_base[s] + ri + lane;
        if (at < j.n_slots) j.slots[at] = c;
        return ok && at < j.n_slots;
    }
    __device__ __forceinline__ void emit(const IdxWalkJob&, uint32_t, uint32_t, uint32_t n, const uint64_t*, bool) { ri += n; }
    __device__ __forceinline__ void finish(const IdxWalkJob& j, uint32_t s, uint64_t off, uint32_t fl) const
    {
        j.n_rec[s] = (uint32_t)ri;
        j.end_off[s] = off;
        j.flags[s] = fl;
    }
};

__global__ __launch_bounds__(64) void gd_idx_walk_kernel(IdxWalkJob j) { bam_walk(j, IndexWalk{}); }

// A THREAD PER RECORD over the table the counting walk left: a workgroup per anchor segment (its record count, bases and
// table entry come from the walk's tables), the fields and the CIGAR (the stored one or the CG tag's, found again) copied
// to the contig's arrays.  The records of neighbouring threads are neighbours in the stream and in the output.
__global__ __launch_bounds__(256) void gd_bam_extract_tab_kernel(BamSegJob j)
{
    const uint32_t s = blockIdx.x;
    if (s >= j.n_seg) return;
    const uint32_t n = j.n_rec[s];
    const uint64_t beg = j.seg_beg[s], rb = j.rec_base[s], ob = j.op_base[s];
    const uint32_t* const tab = j.tab + 2ull * j.tab_base[s];
    for (uint32_t k = threadIdx.x; k < n; k += blockDim.x) {
        const uint64_t o = beg + tab[2u * k];
        const uint8_t* const r = j.data + o + 4;
        const uint8_t* cg = nullptr;
        uint32_t nc = 0;
        (void)bam_record_cigar(r, ld32(j.data + o), &cg, &nc);      // (the walk has seen it succeed)
        const uint64_t rr = rb + k, oo = ob + tab[2u * k + 1u];
        j.pos[rr] = (int32_t)ld32(r + 4);
        j.mapq[rr] = r[9];
        j.flag[rr] = (uint16_t)((uint32_t)r[14] | ((uint32_t)r[15] << 8));
        j.cigar_off[rr] = (uint32_t)oo;
        for (uint32_t q = 0; q < nc; ++q) j.cigar[oo + q] = ld32(cg + 4 * (uint64_t)q);
    }
}

}  // namespace gd
