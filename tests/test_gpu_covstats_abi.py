"""The covstats kernels (gd_covstats.hpp: walk, compact, tile, tscan, select, hist) through the device ABI, count by
count: gd_covstats_begin / gd_covstats_decode / gd_covstats_histogram against tests/covstats_ref.py and this file's own
parse of the inflated stream, every comparison an exact integer one.

The CLI row (tests/test_gpu_covstats.py) rounds to two decimals, drops the upper tail in madFilter and shows nothing of a
range's state; here every range's counts, its `resume`, and the whole multiset of every histogram (overflow lists
included) are compared.  The sampling loop is sequential, so the state after the device has walked the first K records
of the file is bam_stats(recs[:K], n, skip).

The BAMs are crafted at test time.  Every edge that depends on byte layout or on a record index is asserted from the
crafted bytes alone by the tests without the gpu mark (test_input_*), so that an input that no longer hits its edge
fails there instead of turning a GPU test into a no-op."""
import bisect
import itertools
import struct
import zlib
from collections import Counter

import numpy as np
import pytest

from oracle import bamio
from tests import covstats_ref as R

GD_E_INVALID, GD_E_STATE, GD_E_CAPACITY = -1, -4, -8
WIN, REC = 3072, 32                      # BW_WIN, BW_REC of gd_bamdecode.hpp (the one walk, gd_cs_walk_kernel included): bytes of stream in LDS, records per round
SLOT_BYTES = 36                          # gd_covstats_decode: a slot per 36 bytes of a segment, plus one
CS_TILE, CS_HBINS = 1024, 1 << 16        # gd_covstats.hpp
LO = (0, -(CS_HBINS // 2), -(CS_HBINS // 2))   # CS_LO_SIZE, CS_LO_INS, CS_LO_TL
KINDS = ("sizes", "ins", "tl")
M, I, D, N_, S, H_, P, EQ, X = range(9)
REFS = [("c1", 1 << 30), ("c2", 1 << 29), ("c3", 1 << 20)]
ONE, PER_MEMBER, IRREGULAR = [1 << 30], [1], [3, 1, 2, 5, 1, 1, 4]
BIG = (1 << 28) - 1
NEVER = 10 ** 6                          # an n no file here reaches


# ---- a crafted BAM as this file sees it ---------------------------------------------------------------------------------
class Bam:
    """The file's bytes, its BGZF member table, the inflated stream and the record offsets in it -- all parsed here."""

    def __init__(self, path, records=True):
        self.path = path
        self.data = d = open(path, "rb").read()
        self.coff, self.isize, parts = [], [], []
        p = 0
        while p < len(d):
            assert d[p:p + 4] == b"\x1f\x8b\x08\x04" and d[p + 12:p + 16] == b"BC\x02\x00"
            xlen, = struct.unpack_from("<H", d, p + 10)
            bsize, = struct.unpack_from("<H", d, p + 16)
            raw = zlib.decompress(d[p + 12 + xlen:p + bsize + 1 - 8], -15)
            assert len(raw) == struct.unpack_from("<I", d, p + bsize + 1 - 4)[0]
            self.coff.append(p)
            self.isize.append(len(raw))
            parts.append(raw)
            p += bsize + 1
        self.nm = len(self.coff)                            # (the EOF marker included)
        self.coff.append(len(d))
        self.out = [0] + list(itertools.accumulate(self.isize))
        self.stream = s = b"".join(parts)
        self.total = len(s)
        l_text, = struct.unpack_from("<i", s, 4)
        p = 8 + l_text
        n_ref, = struct.unpack_from("<i", s, p)
        p += 4
        for _ in range(n_ref):
            p += 8 + struct.unpack_from("<i", s, p)[0]
        self.hdr = p
        self.beg, self.end = [], []
        self.recs = []
        self.cache = {}
        if records:
            while p < self.total:
                self.beg.append(p)
                p += 4 + struct.unpack_from("<i", s, p)[0]
                self.end.append(p)
            assert p == self.total
            self.recs = R.read_records(path)[2]
            assert len(self.recs) == len(self.beg)

    def member(self, coff):
        k = bisect.bisect_left(self.coff, coff)
        assert k <= self.nm and self.coff[k] == coff, "%d is not a member start of the file" % coff
        return k

    def resolve(self, v):
        """The offset in the inflated stream of virtual offset v: its member must be one of the file's (or the file's
        end, for the range that ends it) and its uoffset at most that member's ISIZE."""
        k, u = self.member(v >> 16), v & 0xffff
        assert u <= (self.isize[k] if k < self.nm else 0), "uoffset %d beyond ISIZE of the member at %d" % (u, v >> 16)
        return self.out[k] + u

    def voff(self, o):
        """Offset o of the inflated stream, spelled in the last member that begins at or before it."""
        k = bisect.bisect_right(self.out, o, 0, self.nm) - 1
        return (self.coff[k] << 16) | (o - self.out[k])

    def respell(self, v):
        """(member, 0) as (the member before, its ISIZE) where there is one with bytes."""
        k = self.member(v >> 16)
        if (v & 0xffff) == 0 and 0 < k <= self.nm and self.isize[k - 1] > 0:
            return (self.coff[k - 1] << 16) | self.isize[k - 1]
        return v

    def prefix(self, n, skip, k):
        key = (n, skip, k)
        if key not in self.cache:
            self.cache[key] = R.bam_stats(self.recs[:k], n, skip)
        return self.cache[key]

    # anchor choices
    def anchors(self, which):
        if which == "none":
            return np.zeros(0, np.uint64)
        if which == "bai":
            lin = bamio.read_bai_linear(self.path + ".bai")
            return np.unique(np.concatenate([np.zeros(0, np.uint64)] + [np.asarray(v, np.uint64) for v in lin.values()]))
        if which == "every":
            return np.asarray([self.voff(o) for o in self.beg], np.uint64)
        if which == "extra":                                # some record starts, one before any record, one behind all
            return np.asarray([0] + [self.voff(o) for o in self.beg[::7]] + [self.coff[self.nm - 1] << 16], np.uint64)
        raise KeyError(which)


def eligible(r):
    return (not r.flag & 0x604 and r.flag & 0x2 and r.pos < r.next_pos and len(r.cigar) == 1 and r.cigar[0][0] == M)


def ranges(bam, plan, n, skip, alt=False, decode=None):
    """The host's loop (covstats_host.cpp): a range is a run of whole members from the one that holds first_voffset;
    plan: how many members the successive ranges take (cycled; doubled while a range holds no whole record).  Every
    range is restated from the member table and the record offsets; decode(range, prefix state, done) returns the
    device's `resume` (without it: the restated one, for the checks that need no device).  alt: a first_voffset at
    uoffset 0 is spelled as the previous member's end."""
    plan = itertools.cycle(plan)
    voff, want, k_seen, out = bam.voff(bam.hdr), next(plan), 0, []
    while True:
        if alt:
            voff = bam.respell(voff)
        mi = bam.member(voff >> 16)
        me = min(mi + want, bam.nm)
        if me == bam.nm - 1:                                # (the EOF marker goes with the last data)
            me = bam.nm
        while me < bam.nm and bam.out[me] == bam.out[mi]:   # (a range of empty members only: the host's ranges are 64 KB at least)
            me += 1
        f = bam.resolve(voff)
        k0 = bisect.bisect_left(bam.beg, f)
        assert k0 == k_seen and (bam.beg[k0] == f if k0 < len(bam.beg) else f == bam.total)
        k1 = max(k0, bisect.bisect_right(bam.end, bam.out[me]))      # records that end at or before the range's last byte
        r = dict(voff=voff, mi=mi, me=me, last=me == bam.nm, k0=k0, k1=k1, n=k1 - k0, first=min(max(0, skip - k0), k1 - k0),
                 stop_at=bam.beg[k1] if k1 < len(bam.beg) else bam.total)
        st = bam.prefix(n, skip, k1)
        done = st["stopped"] if n > 0 else skip - k1 <= 0
        assert st["stopped"] == done                        # (the restatement's key says the same for n <= 0)
        out.append(r)
        if decode is not None:
            resume = decode(r, st, done)
        elif r["stop_at"] >= bam.out[me]:
            resume = bam.coff[me] << 16
        else:
            resume = bam.voff(r["stop_at"])
        if done or r["last"]:
            return out
        if bam.resolve(resume) == f:                        # not one whole record: a larger range
            want *= 2
            continue
        voff, k_seen, want = resume, k1, next(plan)


def run(eng, bam, n, skip, plan=ONE, anchors="none", alt=False):
    """One sampling run on the device, asserted after every gd_covstats_decode and at its end; returns what must not
    depend on the cutting or the anchors: the final counts and the three histograms."""
    a = bam.anchors(anchors) if isinstance(anchors, str) else np.asarray(anchors, np.uint64)
    got = {}

    def decode(r, st, done):
        eng.ingest_feed_range(bam.data[bam.coff[r["mi"]]:bam.coff[r["me"]]], bam.coff[r["mi"]])
        c = eng.covstats_decode(r["voff"], a, r["last"])
        ctx = "n=%d skip=%d range %r" % (n, skip, r)
        assert (c.range_records, c.records) == (r["n"], r["k1"]), ctx
        assert bam.resolve(c.resume) == r["stop_at"], ctx
        assert c.skip_left == max(0, skip - r["k1"]), ctx
        assert (c.unmapped, c.counted, c.bad, c.dup, c.proper) == st["counts"], ctx
        assert (c.sizes, c.inserts) == (len(st["sizes"]), len(st["ins"])), ctx
        assert c.done in (0, 1) and c.done == int(done), ctx
        if n <= 0:
            assert c.done == int(c.skip_left == 0), ctx
        got["c"] = c
        return c.resume

    eng.covstats_begin(n, skip)
    rs = ranges(bam, plan, n, skip, alt, decode)
    c, st = got["c"], bam.prefix(n, skip, rs[-1]["k1"])
    full = bam.prefix(n, skip, len(bam.recs))               # the loop has stopped or the file has ended
    assert all(st[k] == full[k] for k in ("counts", "stopped") + KINDS)
    hists = []
    for w, kind in enumerate(KINDS):
        lo, bins, ovf = eng.covstats_histogram(w)
        assert lo == LO[w] and bins.size == CS_HBINS
        assert all(not lo <= int(v) < lo + CS_HBINS for v in ovf), "an overflow value inside the window of %s" % kind
        have = Counter({lo + int(i): int(bins[i]) for i in np.flatnonzero(bins)})
        have.update(int(v) for v in ovf)
        want = Counter(st[kind])
        if have != want:
            v = min(k for k in set(have) | set(want) if have[k] != want[k])
            pytest.fail("%s, n=%d skip=%d: value %d sampled %d times, the device has %d" % (kind, n, skip, v, want[v], have[v]))
        assert int(bins.sum()) + ovf.size == (c.sizes if w == 0 else c.inserts)
        hists.append((bins.tobytes(), tuple(sorted(int(v) for v in ovf))))
    return (c.skip_left, c.unmapped, c.counted, c.bad, c.dup, c.proper, c.sizes, c.inserts, c.done), hists


def same_everywhere(eng, bam, n, skip, configs):
    res = [run(eng, bam, n, skip, plan, anchors, alt) for plan, anchors, alt in configs]
    assert all(r == res[0] for r in res[1:]), "n=%d skip=%d: the answer depends on the cutting or the anchors" % (n, skip)
    return res[0]


# ---- records ------------------------------------------------------------------------------------------------------------------
def pe(pos, ins=200, mlen=100, flag=0x3, tlen=None, ref=0, cigar=None, next_pos=None, **kw):
    """A 40-byte record (no name): proper pair, one M op -- eligible for an insert unless an argument says otherwise."""
    return R.raw_rec(ref, pos, flag, pos + mlen + ins if next_pos is None else next_pos,
                     ins + 2 * mlen if tlen is None else tlen, ((M, mlen),) if cigar is None else cigar, **kw)


def mixed(i, pos):
    """Period 11 (coprime with the four records of a select thread): the good and the eligible ranks part ways inside
    a thread, and every branch of the role is taken."""
    k = i % 11
    ml = 90 + i % 23
    if k in (0, 5):
        return pe(pos, 150 + i % 97, ml, tlen=300 + i % 211)
    if k == 1:
        return pe(pos, flag=0x5)                            # unmapped
    if k == 2:
        return pe(pos, flag=0x403, mlen=ml)                 # duplicate
    if k == 3:
        return pe(pos, mlen=ml, next_pos=pos)               # pos == next_pos: good, no insert
    if k == 4:
        return pe(pos, flag=0x203, mlen=ml)                 # QC failure
    if k == 6:
        return pe(pos, flag=0x603, mlen=ml)                 # both
    if k == 7:
        return pe(pos, flag=0x1, mlen=ml)                   # 0x2 absent
    if k == 8:
        return pe(pos, mlen=ml, next_pos=pos - 50)          # pos > next_pos
    if k == 9:
        return pe(pos, cigar=((EQ, ml),))                   # one op, not M
    return pe(pos, flag=0x407)                              # unmapped wins over duplicate


def build(d, name, recs, **kw):
    p = str(d / name)
    R.write_bam(p, REFS, recs, **kw)
    return Bam(p)


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("covabi")


# ---- the walk BAM ---------------------------------------------------------------------------------------------------------------
N36 = 400


def walk_rounds(beg, end, seg_beg, seg_end, n_bytes):
    """The rounds of gd_cs_walk_kernel over one segment, from the record offsets alone (offsets relative to the range's
    first inflated byte): [(records of the round, why it ended, rel of the record it ended on)]."""
    nxt = dict(zip(beg, end))
    off, rounds = seg_beg, []
    while True:
        wbase, k, why, rel = off & ~15, 0, "full", None
        while k < REC:
            rel = off - wbase
            if off >= seg_end:
                why = "end"
                break
            if rel + 4 > WIN:
                why = "window"
                break
            if off + 4 > n_bytes or nxt[off] > n_bytes:
                why = "cut"
                break
            k, off = k + 1, nxt[off]
        rounds.append((k, why, rel))
        if why in ("end", "cut") or off >= seg_end:
            return rounds


def walk_records(filler):
    recs = [mixed(i, 1000 * i) for i in range(22)]
    recs += [R.raw_rec(0, 30000 + i, 0x4) for i in range(N36)]           # block_size 32: no name, no CIGAR
    recs += [pe(40000 + 300 * i, tags=b"\0" * 260) for i in range(6)]      # 300 bytes each
    recs += [pe(43000, tags=b"\0" * filler)]
    recs += [pe(44000 + 300 * i, tags=b"\0" * 260) for i in range(14)]
    recs += [pe(50000, mlen=4000, l_seq=4000, name=b"q" * 254 + b"\0", tags=b"XZZ" + b"a" * 200 + b"\0")]   # > WIN bytes
    ops9 = ((M, 10), (I, 2), (D, 3), (N_, 400), (S, 5), (H_, 6), (P, 7), (EQ, 8), (X, 9))
    recs += [pe(60000), pe(60100, cigar=((EQ, 77),)), pe(60200, cigar=((S, 55),)), pe(60300, cigar=ops9),
             pe(60400, cigar=ops9[::-1] * 3), pe(60500, cigar=()), pe(60600, cigar=((M, BIG),) * 9 + ((D, BIG), (S, BIG)) * 4),
             pe(60700, cigar=tuple((i % 9, BIG) for i in range(65535))), pe(70000, mlen=BIG)]
    recs += [mixed(i, 100000 + 5000 * i) for i in range(40)]
    recs += [pe(2000 * i, 100 + i, ref=1) for i in range(30)] + [pe(3000 * i, flag=0x1, ref=2) for i in range(30)]
    recs += [R.raw_rec(-1, -1, 0x4 if i % 3 else 0x1, name=b"u\0") for i in range(25)]
    return recs


def walk_layout(hdr, recs):
    beg = [hdr + o for o in itertools.accumulate([0] + [len(r.raw) for r in recs[:-1]])]
    return beg, [b + len(r.raw) for b, r in zip(beg, recs)]


W_STRADDLE_END, W_BODY, W_EXACT, W_EMPTY = 30, 60, 90, 120    # records at which a member boundary is placed


def walk_cuts(hdr, beg, total):
    cuts = set(range(4096, total, 4096))
    cuts |= {beg[W_STRADDLE_END] + 2, beg[W_BODY] + 20, beg[W_EXACT], beg[W_EMPTY]}
    return sorted(list(cuts) + [beg[W_EMPTY]])            # (given twice: an empty member)


@pytest.fixture(scope="module")
def bam_walk(tmp):
    hdr = build(tmp, "empty.bam", [], index=False).hdr
    for filler in range(400):                               # the filler that puts a block_size word across a window's end
        recs = walk_records(filler)
        beg, end = walk_layout(hdr, recs)
        if any(why == "window" and rel in (WIN - 3, WIN - 2, WIN - 1) for _, why, rel in walk_rounds(beg, end, hdr, end[-1], end[-1])):
            return build(tmp, "walk.bam", recs, cuts=walk_cuts)
    pytest.fail("no filler gives a window straddle")


def run36(bam):
    """Anchors at both ends of the run of 36-byte records."""
    return np.asarray([bam.voff(bam.beg[22]), bam.voff(bam.beg[22 + N36])], np.uint64)


def test_input_walk_edges(bam_walk):
    b = bam_walk
    # one range without anchors: one segment from the header's end (member 0 holds it, so offsets are the stream's)
    rounds = walk_rounds(b.beg, b.end, b.hdr, b.total, b.total)
    assert sum(k for k, _, _ in rounds) == len(b.recs)
    assert any(why == "window" and rel in (3069, 3070, 3071) for _, why, rel in rounds)    # the word straddles WIN
    assert any(k == REC and why == "full" for k, why, _ in rounds)                         # > 32 records in one window
    assert all(e - s == SLOT_BYTES for s, e in zip(b.beg[22:22 + N36], b.end[22:22 + N36]))
    assert max(e - s for s, e in zip(b.beg, b.end)) > 260000 and any(WIN < e - s < 9000 for s, e in zip(b.beg, b.end))
    assert b.voff(b.hdr) & 0xffff                                                          # the first record: mid-member
    assert 0 in b.isize[1:-1]                                                              # an empty member in mid-file
    rs = ranges(b, PER_MEMBER, NEVER, 0)
    ends = [b.out[r["me"]] for r in rs]
    assert b.beg[W_STRADDLE_END] + 2 in ends and b.beg[W_BODY] + 20 in ends and b.beg[W_EXACT] in ends
    assert any(r["n"] == 0 for r in rs)                                                    # no whole record: doubled
    assert any(r["voff"] & 0xffff for r in rs[1:])                                         # a range that starts mid-member
    # every record start an anchor: a range whose last anchor is on the record it holds only in part
    assert any(r["stop_at"] < b.out[r["me"]] for r in rs)
    assert any(r["voff"] & 0xffff == b.isize[r["mi"]] for r in ranges(b, PER_MEMBER, NEVER, 0, alt=True))   # uoffset == ISIZE
    assert len({r.ref for r in b.recs}) == 4


WALK_CONFIGS = [(ONE, "none", False), (ONE, "bai", False), (ONE, "every", False), (PER_MEMBER, "none", False),
                (PER_MEMBER, "every", False), (PER_MEMBER, "extra", True), (IRREGULAR, "bai", False),
                (IRREGULAR, "every", True), (IRREGULAR, "extra", False), (PER_MEMBER, "bai", True)]


@pytest.fixture(scope="module")
def eng():
    from goleft_amd.engine import DepthEngine
    with DepthEngine(0) as e:
        yield e


@pytest.mark.gpu
@pytest.mark.parametrize("n,skip", [(NEVER, 0), (7, 3), (40, 430), (1, 0)])
def test_walk_edges_every_cutting_and_anchor_choice(eng, bam_walk, n, skip):
    configs = WALK_CONFIGS + [(ONE, run36(bam_walk), False), (IRREGULAR, run36(bam_walk), False)]
    res = same_everywhere(eng, bam_walk, n, skip, configs)
    if n == NEVER:                                          # the 64-bit query lengths reached the overflow list
        assert max(res[1][0][1]) == sum(BIG for i in range(65535) if i % 9 in (M, I, S, EQ, X))


# ---- the scan BAM -----------------------------------------------------------------------------------------------------------------
SCAN_COUNTS = [1500, 1024, 1025, 1, 4097, 1023, 300]       # records per range under SCAN_PLAN
SCAN_PLAN = [1, 1, 1, 1, 3, 1, 1]                           # members per range (4097 records: three members)
SCAN_N = sum(SCAN_COUNTS)
R4 = 1500 + 1024 + 1025 + 1                                 # the first record of the 4097-record range
SCAN_STOPS = [700, 1023, 1024, 1499, 1500, R4 + 4096, SCAN_N - 1]


def scan_cuts(hdr, beg, total):
    starts = list(itertools.accumulate([0] + SCAN_COUNTS[:-1]))
    return sorted([beg[s] for s in starts] + [beg[R4 + 1400], beg[R4 + 2800]])


@pytest.fixture(scope="module")
def bam_scan(tmp):
    recs = [pe(10 * i, 100 + i % 300) if i in SCAN_STOPS else mixed(i, 10 * i) for i in range(SCAN_N)]
    return build(tmp, "scan.bam", recs, cuts=scan_cuts)


def n_for_stop(bam, skip, idx):
    """The n whose n-th insert is record idx, asserted on the restatement."""
    n = sum(1 for r in bam.recs[skip:idx + 1] if eligible(r))
    assert eligible(bam.recs[idx]) and idx >= skip
    a, b = bam.prefix(n, skip, idx), bam.prefix(n, skip, idx + 1)
    assert not a["stopped"] and b["stopped"] and len(b["ins"]) == n
    return n


def test_input_scan_edges(bam_scan):
    b = bam_scan
    rs = ranges(b, SCAN_PLAN, NEVER, 0)
    assert [r["n"] for r in rs] == SCAN_COUNTS              # N of 1, 1023, 1024, 1025 and 4097 in a range
    assert all(r["stop_at"] == b.out[r["me"]] for r in rs)   # every range ends at a record's end
    # where the stop lands in its range, modulo CS_TILE
    where = {}
    for idx in SCAN_STOPS:
        skip = 700 if idx == 700 else 0
        rs = ranges(b, SCAN_PLAN, n_for_stop(b, skip, idx), skip)
        assert rs[-1]["k0"] <= idx < rs[-1]["k1"]
        where[idx] = (idx - rs[-1]["k0"], rs[-1]["n"], rs[-1]["first"])
    assert where[700] == (700, 1500, 700)                   # the stop at `first`
    assert where[1023][0] % CS_TILE == 1023 and where[1024][0] % CS_TILE == 0 and where[1024][0] > 0
    assert where[1499][0] == where[1499][1] - 1             # the last record of a range
    assert where[1500][0] == 0                              # index 0 of a range: cut immediately before the n-th insert
    assert where[R4 + 4096][0] == 4096                      # the partial fifth tile of the 4097-record range
    assert where[SCAN_N - 1][0] == SCAN_COUNTS[-1] - 1 and SCAN_N - 1 == len(b.recs) - 1
    # where the skip ends
    first = lambda skip: [(r["first"], r["n"]) for r in ranges(b, SCAN_PLAN, NEVER, skip)]
    assert first(700)[0] == (700, 1500) and first(1024)[0] == (1024, 1500)
    assert first(1500)[:2] == [(1500, 1500), (0, 1024)]     # first == N: no scan is launched
    assert first(1501)[:2] == [(1500, 1500), (1, 1024)]
    assert all(f == n for f, n in first(10 ** 7))


SCAN_CONFIGS = [(SCAN_PLAN, "none", False), (ONE, "none", False), (SCAN_PLAN, "extra", False)]


@pytest.mark.gpu
@pytest.mark.parametrize("idx", SCAN_STOPS)
def test_scan_stop_record_positions(eng, bam_scan, idx):
    skip = 700 if idx == 700 else 0
    res = same_everywhere(eng, bam_scan, n_for_stop(bam_scan, skip, idx), skip, SCAN_CONFIGS)
    assert res[0][-1] == 1


@pytest.mark.gpu
@pytest.mark.parametrize("skip", [700, 1024, 1500, 1501, 10 ** 7])
def test_scan_where_the_skip_ends(eng, bam_scan, skip):
    for n in (NEVER, 50):
        res = same_everywhere(eng, bam_scan, n, skip, SCAN_CONFIGS)
        assert (res[0][0] > 0) == (skip > SCAN_N)


@pytest.mark.gpu
def test_scan_n_of_zero_one_and_one_too_many(eng, bam_scan):
    n_elig = sum(1 for r in bam_scan.recs if eligible(r))
    for n, skip in ((0, 0), (0, 2000), (0, 10 ** 7), (1, 0), (n_elig, 0), (n_elig + 1, 0), (n_elig - 50, 37)):
        res = same_everywhere(eng, bam_scan, n, skip, SCAN_CONFIGS)
        assert res[0][-1] == int(n == 0 and skip < SCAN_N or 0 < n <= n_elig)


# ---- single-end data: the break -------------------------------------------------------------------------------------------------
SE_COUNTS = [1500, 2600]
SE_INS = (3000, 3100)                                       # the only two eligible records


def se_cuts(hdr, beg, total):
    return sorted({hdr, beg[1500]} | {beg[k] for k in range(1000, len(beg), 1000)})


@pytest.fixture(scope="module")
def bam_se(tmp):
    recs = [pe(10 * i) if i in SE_INS else pe(10 * i, flag=0x5 if i % 5 == 2 else 0x1) for i in range(sum(SE_COUNTS))]
    return build(tmp, "se.bam", recs, cuts=se_cuts)


SE_PLAN = [2, 1 << 30]                                      # 1500 records, then the rest


def test_input_single_end_edges(bam_se):
    b = bam_se
    assert [r["n"] for r in ranges(b, SE_PLAN, NEVER, 0)] == SE_COUNTS
    # sizes0 == 2n when the second range begins, and its first record breaks the loop
    a, c = b.prefix(600, 0, 1500), b.prefix(600, 0, 1501)
    assert len(a["sizes"]) == 1200 and not a["stopped"] and c["stopped"] and not c["ins"] and c["counts"][1] == a["counts"][1] + 1
    # n = 2 in one range of five tiles: every good record from rank 4 to the first eligible one is a candidate for the
    # break (tiles 0, 1 and 2) and the second eligible record for the n-th insert (tile 3): the minimum decides
    good = [i for i, r in enumerate(b.recs) if not r.flag & 0x604]
    assert b.prefix(2, 0, good[4])["stopped"] is False and b.prefix(2, 0, good[4] + 1)["stopped"]
    assert good[4] < CS_TILE < 2 * CS_TILE < SE_INS[0] < 3 * CS_TILE < SE_INS[1]
    # the same with the skip past tile 0: the minimum is in tile 1, other candidates in tiles 1 and 2
    g = [i for i in good if i >= 1030]
    assert b.prefix(2, 1030, g[4] + 1)["stopped"] and CS_TILE < g[4] < 2 * CS_TILE


@pytest.mark.gpu
def test_single_end_break_with_carried_sizes_and_many_candidates(eng, bam_se):
    configs = [(SE_PLAN, "none", False), (ONE, "none", False), (PER_MEMBER, "every", True)]
    for n, skip in ((600, 0), (2, 0), (2, 1030), (599, 0), (601, 0), (1, 0), (NEVER, 0)):
        same_everywhere(eng, bam_se, n, skip, configs)


# ---- 257 tiles ---------------------------------------------------------------------------------------------------------------------
BIG_N = 256 * CS_TILE + 1            # the smallest record count with 257 tiles, the last one partial


@pytest.fixture(scope="module")
def bam_big(tmp):
    recs = [mixed(i, 10 * i) for i in range(BIG_N - 1)] + [pe(10 * BIG_N)]
    return build(tmp, "big.bam", recs, index=False)


def test_input_257_tiles(bam_big):
    rs = ranges(bam_big, ONE, NEVER, 0)
    n_tiles = (rs[0]["n"] + CS_TILE - 1) // CS_TILE
    assert len(rs) == 1 and rs[0]["n"] == BIG_N and n_tiles == 257 > 256 and BIG_N % CS_TILE == 1
    assert (n_tiles + 255) // 256 == 2                      # `per` of gd_cs_tscan_kernel
    assert eligible(bam_big.recs[-1])


@pytest.mark.gpu
def test_more_than_256_tiles_in_one_range(eng, bam_big):
    n_elig = sum(1 for r in bam_big.recs if eligible(r))
    for n, skip in ((n_elig, 0), (NEVER, 0), (n_elig - 1, 0), (1000, 100000)):
        res = run(eng, bam_big, n, skip)
        assert res[0][-1] == int(n <= n_elig)


# ---- the histograms -----------------------------------------------------------------------------------------------------------------
OVF_BLOCKS, OVF_N = 3, 150
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1


def hist_records():
    recs = [pe(i) for i in range(4096)]                                             # 64 waves, every lane in one bin
    recs += [pe(i, 200 + i % 2, 100 + i % 2, tlen=400 if i % 2 else -400) for i in range(4096)]    # two bins, lane by lane
    recs += [pe(i, -32 + i % 64, 100 + i % 64, tlen=1000 + i % 64) for i in range(4096)]           # 64 distinct bins
    edge = [pe(0, mlen=0), pe(0, mlen=65535), pe(0, mlen=65536)]                    # sizes at 0, CS_HBINS - 1, CS_HBINS
    for v in (-32769, -32768, 32767, 32768):                                        # the windows of the other two kinds
        edge += [pe(0, ins=v, mlen=40000, tlen=v), pe(5, ins=v, mlen=40000, tlen=-v)]
    edge += [pe(0, tlen=I32_MIN), pe(0, tlen=I32_MAX)]
    edge += [pe(I32_MAX - 2, mlen=BIG, next_pos=I32_MAX), pe(I32_MIN, mlen=1, next_pos=I32_MAX)]   # 64-bit inserts
    recs += edge * 3
    n_body = len(recs)
    for k in range(OVF_BLOCKS * OVF_N):                     # outside all three windows
        recs.append(pe(k, ins=40000 + k % 3, mlen=70000 + k % 5, tlen=10 ** 6 + k))
    recs += [pe(i) for i in range(100)]
    return recs, n_body


def hist_cuts(hdr, beg, total):
    n_body = hist_records()[1]
    return sorted([hdr] + [beg[k] for k in range(1500, n_body, 1500)] + [beg[n_body + OVF_N * k] for k in range(OVF_BLOCKS + 1)])


@pytest.fixture(scope="module")
def bam_hist(tmp):
    return build(tmp, "hist.bam", hist_records()[0], cuts=hist_cuts)


def test_input_histogram_edges(bam_hist):
    b = bam_hist
    assert all(eligible(r) for r in b.recs)                 # every record is sampled three times
    n_body = hist_records()[1]
    outside = lambda w, v: not LO[w] <= v < LO[w] + CS_HBINS
    full = 0
    for r in ranges(b, PER_MEMBER, NEVER, 0):
        recs = b.recs[r["k0"]:r["k1"]]
        over = [sum(1 for x in recs if outside(0, R.qlen(x.cigar))),
                sum(1 for x in recs if outside(1, x.next_pos - x.pos - x.cigar[0][1])),
                sum(1 for x in recs if outside(2, x.tlen))]
        full += over == [r["n"]] * 3 and r["n"] == OVF_N and r["k0"] >= n_body       # the overflow count reaches ovf_cap = N
    assert full == OVF_BLOCKS
    st = b.prefix(NEVER, 0, len(b.recs))
    for w, want in enumerate(((0, 65535, 65536), (-32769, -32768, 32767, 32768), (-32769, -32768, 32767, 32768, I32_MIN, I32_MAX))):
        assert set(want) <= set(st[KINDS[w]])
    assert I32_MAX - (I32_MAX - 2 + BIG) in st["ins"] and I32_MAX - (I32_MIN + 1) in st["ins"]   # the latter exceeds 32 bits
    assert all(len({(R.qlen(x.cigar), x.next_pos - x.pos, x.tlen) for x in b.recs[k:k + 64]}) == 1 for k in range(0, 4096, 64))
    assert all(len({R.qlen(x.cigar) for x in b.recs[k:k + 64]}) == 2 for k in range(4096, 8192, 64))
    assert all(len({x.tlen for x in b.recs[k:k + 64]}) == 64 for k in range(8192, 12288, 64))


@pytest.mark.gpu
@pytest.mark.parametrize("n,skip", [(NEVER, 0), (6000, 0), (NEVER, 64), (5000, 4101)])
def test_histograms_bin_by_bin(eng, bam_hist, n, skip):
    res = same_everywhere(eng, bam_hist, n, skip, [(ONE, "none", False), (PER_MEMBER, "none", False), (IRREGULAR, "bai", False),
                                                    (PER_MEMBER, "extra", True)])
    if n == NEVER and skip == 0:
        assert all(len(h[1]) >= OVF_BLOCKS * OVF_N for h in res[1])     # overflow values of several ranges, kept


# ---- one context, two runs -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_context_used_again_answers_as_a_fresh_one(bam_big, bam_scan, bam_hist):
    from goleft_amd.engine import DepthEngine
    with DepthEngine(0) as fresh:
        want = run(fresh, bam_scan, 300, 10, SCAN_PLAN)
    with DepthEngine(0) as used:
        run(used, bam_big, NEVER, 0)
        run(used, bam_hist, NEVER, 0, PER_MEMBER)
        used.covstats_begin(5, 5)
        used.covstats_begin(300, 10)                        # begin twice: the first run's state is gone
        assert run(used, bam_scan, 300, 10, SCAN_PLAN) == want


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def damaged(tmp, name, bam, at, patch):
    s = bytearray(bam.stream)
    s[at:at + len(patch)] = patch
    raw, _ = R.bgzf_cut(bytes(s), list(range(4096, len(s), 4096)))
    p = tmp / name
    p.write_bytes(raw)
    return Bam(str(p), records=False)


def decode_whole(eng, bam, anchors=(), last=True, n=NEVER, members=None):
    me = bam.nm if members is None else members
    eng.covstats_begin(n, 0)
    eng.ingest_feed_range(bam.data[:bam.coff[me]], 0)
    return eng.covstats_decode(bam.voff(bam.hdr), np.asarray(anchors, np.uint64), last)


@pytest.mark.gpu
def test_refusals_leave_the_context_usable(tmp):
    from goleft_amd.engine import DepthEngine, GdError
    good = build(tmp, "good.bam", [mixed(i, 100 * i) for i in range(600)], block=4096)
    want = good.prefix(NEVER, 0, 600)

    def still_good(eng):
        c = decode_whole(eng, good)
        assert (c.records, c.unmapped, c.counted, c.bad, c.dup, c.proper) == (600,) + want["counts"]
        assert (c.sizes, c.inserts, c.done) == (len(want["sizes"]), len(want["ins"]), 0)

    def refused(eng, status, word, *a, **kw):
        with pytest.raises(GdError) as e:
            decode_whole(eng, *a, **kw)
        assert e.value.status == status and word in str(e.value), e.value
        still_good(eng)

    with DepthEngine(0) as eng:
        # before gd_covstats_begin, with a range fed; then with nothing fed
        eng.ingest_feed_range(good.data, 0)
        with pytest.raises(GdError) as e:
            eng.covstats_decode(good.voff(good.hdr), [], True)
        assert e.value.status == GD_E_STATE
        eng.covstats_begin(NEVER, 0)
        c = eng.covstats_decode(good.voff(good.hdr), [], True)          # the range is still pending: decoded now
        assert c.records == 600
        with pytest.raises(GdError) as e:
            eng.covstats_decode(good.voff(good.hdr), [], True)
        assert e.value.status == GD_E_STATE
        still_good(eng)
        # each damaged input once
        refused(eng, GD_E_INVALID, "anchor", good, anchors=[good.voff(good.beg[300]) + 3])
        at = good.beg[250]
        refused(eng, GD_E_INVALID, "segment", damaged(tmp, "bs.bam", good, at, struct.pack("<i", 31)))
        refused(eng, GD_E_INVALID, "segment", damaged(tmp, "cig.bam", good, at + 16, struct.pack("<H", 100)))   # n_cigar_op
        cut = next(k for k in range(2, good.nm) if good.out[k] not in good.beg)
        refused(eng, GD_E_INVALID, "segment", good, members=cut)          # last_range on a range that ends inside a record
        # an overflow list larger than the room offered
        over = build(tmp, "over.bam", [pe(i, mlen=70000) for i in range(10)], block=4096)
        c = decode_whole(eng, over)
        assert c.sizes == 10
        with pytest.raises(GdError) as e:
            eng.covstats_histogram(0, cap=9)
        assert e.value.status == GD_E_CAPACITY
        assert sorted(eng.covstats_histogram(0)[2]) == [70000] * 10
        still_good(eng)


# ---- random files ------------------------------------------------------------------------------------------------------------------
def random_bam(tmp, seed):
    rng = np.random.default_rng(seed)
    edge = [-32770, -32769, -32768, -1, 0, 1, 32767, 32768, 65535, 65536, 70000, 1 << 29, I32_MIN, I32_MAX]
    flags = [0x3, 0x3, 0x3, 0x1, 0x5, 0x403, 0x203, 0x603, 0x103, 0x803, 0x13, 0x0, 0x7]
    recs = []
    for i in range(int(rng.integers(2500, 4000))):
        flag = int(rng.choice(flags))
        pos = int(rng.integers(0, 1 << 28))
        kind = rng.integers(0, 10)
        if kind < 6:
            cigar = ((M, int(rng.choice([0, 1, 76, 100, 150, 151, 65535, 65536, BIG]))),)
        elif kind < 8:
            cigar = tuple((int(rng.integers(0, 9)), int(rng.integers(0, 300))) for _ in range(int(rng.integers(0, 12))))
        else:
            cigar = ((int(rng.choice([S, EQ, X, I, D])), int(rng.integers(1, 200))),)
        ins = int(rng.choice(edge)) if rng.integers(0, 4) == 0 else int(rng.integers(-300, 900))
        ml = cigar[0][1] if len(cigar) == 1 else 100
        nxt = min(max(pos + ml + ins, I32_MIN), I32_MAX) if rng.integers(0, 8) else pos - int(rng.integers(0, 3))
        tlen = int(rng.choice(edge)) if rng.integers(0, 4) == 0 else int(rng.integers(-1000, 1000))
        recs.append(R.raw_rec(int(rng.integers(-1, 3)), pos, flag, nxt, tlen, cigar, name=b"r" * int(rng.integers(0, 40)),
                              tags=b"\0" * int(rng.integers(0, 200)), l_seq=int(rng.integers(0, 60))))
    n_elig = sum(1 for r in recs if eligible(r))
    cases = [(int(rng.choice([1, 2, 17, n_elig // 2, n_elig, n_elig + 1, NEVER])), int(rng.choice([0, 1, 500, 1024, 2047])))
             for _ in range(3)]
    return build(tmp, "rand%d.bam" % seed, recs, block=int(rng.integers(300, 9000))), cases, rng


def test_input_random_files_hold_the_edges(tmp):
    for seed in range(4):
        b, cases, _ = random_bam(tmp, seed)
        st = b.prefix(NEVER, 0, len(b.recs))
        assert len(st["ins"]) > 300 and min(st["ins"]) < LO[1] and max(st["ins"]) >= LO[1] + CS_HBINS
        assert max(st["sizes"]) >= CS_HBINS and min(st["tl"]) < LO[2] and b.nm > 20


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(4))
def test_random_files_cuttings_and_anchors(eng, tmp, seed):
    b, cases, rng = random_bam(tmp, seed)
    every = b.anchors("every")
    for n, skip in cases:
        subset = every[rng.random(every.size) < 0.2]
        plan = [int(x) for x in rng.integers(1, 12, 9)]
        same_everywhere(eng, b, n, skip, [(ONE, "none", False), (plan, subset, bool(rng.integers(0, 2))),
                                          (PER_MEMBER if b.nm < 400 else [5], "every", False)])


# ---- the restatement's prefixes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,skip", [(1, 0), (5, 0), (40, 13), (3, 1000), (NEVER, 7), (0, 5)])
def test_prefix_restatement_is_consistent_with_the_whole(tmp, n, skip):
    recs = [mixed(i, 10 * i) for i in range(300)]
    if n == 3:
        recs = [pe(i, flag=0x1) for i in range(300)]        # single-end: the break, and a skip that outlasts the file
    full = R.bam_stats(recs, n, skip)
    prev, flips = R.bam_stats([], n, skip), 0
    assert prev["stopped"] == (n <= 0 and skip == 0)
    for k in range(1, len(recs) + 1):
        cur = R.bam_stats(recs[:k], n, skip)
        assert all(a <= b for a, b in zip(prev["counts"], cur["counts"]))
        for kind in KINDS:
            assert cur[kind] == full[kind][:len(cur[kind])] and len(prev[kind]) <= len(cur[kind])
        assert cur["stopped"] or not prev["stopped"]
        flips += cur["stopped"] != prev["stopped"]
        if prev["stopped"]:
            assert all(cur[key] == prev[key] for key in ("counts",) + KINDS)
        prev = cur
    assert all(prev[key] == full[key] for key in ("counts", "stopped") + KINDS)
    assert flips == (1 if full["stopped"] and not (n <= 0 and skip == 0) else 0)
    assert full["stopped"] == (skip < 300 if n in (0, 3) else n < NEVER)
