"""Shapes for the long-read path (goleft_amd/csrc/gd_chunk.hpp: gd_dels_raw_kernel and its four walks, gd_ltile2_kernel)
at the kernels' own thresholds, with the two things a test needs to trust them: a second reference that is independent
of the C oracle, and a plain model of the routing that says whether a shape reaches the edge it is named for.

Test infrastructure only, no pytest marks: tests/test_long_shapes.py (CPU) shows that every case hits its edge and that
both references agree; tests/test_gpu_long_shapes.py runs every case on the device.

The model is written from the text of gd_chunk.hpp, gd_kernels.hpp (gd_prep_kernel) and gd_api_compute.inc:
  * the deletion-list pass gives read r (CSR offset o0, n ops) the list slots (o0 >> 1) + r with room for
    cap = ((o0 + n) >> 1) - (o0 >> 1) + 1 entries and the index slots (o0 >> 6) + 3 r with room for
    pcap = ((o0 + n) >> 6) - (o0 >> 6) + 3.  A read of at most WAVE_DELS_MIN = 24 ops is walked by its own lane
    (serial_dels_plain; serial_dels, merged, when its D/N ops outnumber cap).  A longer one is walked by the wave in
    batches of 256 ops, four consecutive ops per lane (wave_dels_plain); the walk gives up at the first batch that
    holds an op above 2^22 bases, starts at or past POS_CAP - 2^30, or would pass cap.  The read is then walked again
    by wave_dels (merged, 64 ops per group), which itself leaves a read with an op above 2^22 bases or a group that
    starts at or past POS_CAP - 2^28 to the lane: serial_dels_plain again, then serial_dels when that passes cap;
  * the plain walks list every D/N op of at least one base and end the read after its last reference-consuming op;
    the merging walks list the D/N runs that an M = X op follows and end the read after its last such op;
  * a read with deletions and K = (end >> 12) - (pos >> 12) + 2 index entries keeps its index when the list is plain
    and K <= pcap; otherwise the tile kernel bisects the list (PT_SEARCH);
  * gd_stats: n_deletions = the list entries of all reads, max_span_seen = the largest end - pos of ALL reads with ops
    (the pass ignores the read filter), lookback = max(64, max_span_seen rounded up to 64);
  * the tile kernel takes the reads [lo, hi) of a tile in batches of NT = 256, candidate i of a batch in wave i % NW,
    lane i / NW.  A hit (end >= t0, pos < tend, kept by the filter) with deletions looks up a = deletions that start
    before t0 and b = those that start before the tile's end, and queues the deletions j0 = max(a - 1, 0) .. b - 1 in
    pieces of DL_CHUNK = 64, one piece per lane and round; a round that would take the wave's queue past LQ_CAP = 128
    drains it first.
The model's constants are restated here, not imported; kernel_constants() reads the headers' text and
tests/test_long_shapes.py holds the two against each other."""
import os
import re
from dataclasses import dataclass, field
from functools import lru_cache

import numpy as np

from oracle import pyoracle as po
from tests import helpers as H

T, NT, WAVE, NW = 4096, 256, 64, 4
DL_CHUNK, PT_SHIFT, WAVE_DELS_MIN, LQ_CAP = 64, 12, 24, 128
OP_MAX = 1 << 22                       # an op above this many bases ends both wave walks
POS_CAP = 0x7fffffff
PLAIN_POS_CAP = POS_CAP - (1 << 30)    # wave_dels_plain gives up on a batch that starts here or later
MERGED_POS_CAP = POS_CAP - (1 << 28)   # wave_dels leaves a group that starts here or later to the lane
BATCH, BATCH_AHEAD = 256, 768          # ops per batch of wave_dels_plain; distance of the load a batch issues
WIDE = 1 << 22                         # candidate reads from which a tile takes phase_b_rows

M, I, D, N, S, HC, P, EQ, X = range(9)
_CONSUMES = np.array([1, 0, 1, 1, 0, 0, 0, 1, 1] + [0] * 7, bool)
_SKIPS = np.array([0, 0, 1, 1] + [0] * 12, bool)


def kernel_constants():
    """The constants of the long-read kernels that the model restates, read from the sources' text."""
    def text(name):
        with open(os.path.join(H.ROOT, "goleft_amd", "csrc", name)) as f:
            return f.read()
    ch, k, sc = text("gd_chunk.hpp"), text("gd_kernels.hpp"), text("gd_scatter.hpp")
    num = lambda pattern, s: int(re.search(pattern, s).group(1), 0)
    big = {int(x) for x in re.findall(r"len(?:v)?\[\w\] > \(1u << (\d+)\)", ch)}
    assert len(big) == 1
    return {"DL_CHUNK": num(r"constexpr uint32_t DL_CHUNK = (\d+);", ch), "PT_SHIFT": num(r"constexpr int PT_SHIFT = (\d+);", ch),
            "WAVE_DELS_MIN": num(r"constexpr uint32_t WAVE_DELS_MIN = (\d+);", ch), "LQ_CAP": num(r"constexpr int LQ_CAP = (\d+);", ch),
            "OP_MAX": 1 << big.pop(), "POS_CAP": num(r"constexpr uint32_t POS_CAP = (0x[0-9a-f]+)u;", sc),
            "plain_pos_cap_shift": num(r"cur >= POS_CAP - \(1u << (\d+)\)\) \{ again = true", ch),
            "merged_pos_cap_shift": num(r"cur >= POS_CAP - \(1u << (\d+)\)\) \{ overflow = true", ch),
            "BATCH": num(r"if \(n > (\d+)u\) B = load\(\1u\);", ch), "BATCH_AHEAD": num(r"for \(uint32_t b0 = 0; b0 < n && !stop; b0 \+= (\d+)u\)", ch),
            "BATCH_LOAD": num(r"if \(b0 \+ (\d+)u < n\) slot = load", ch), "WIDE": 1 << num(r"const bool wide = nrd >= \(1u << (\d+)\);", ch),
            "T": num(r"constexpr int T = (\d+);", k), "NT": num(r"constexpr int NT = (\d+);", k),
            "WAVE": num(r"constexpr int WAVE = (\d+);", k), "NW_is_NT_over_WAVE": bool(re.search(r"constexpr int NW = NT / WAVE;", k))}


# ---- records --------------------------------------------------------------------------------------------------------

def cg(*ops):
    """[(op, length), ...] -> BAM-encoded ops"""
    return [(ln << 4) | op for op, ln in ops]


def reads_of(items):
    """po.Reads from (pos, encoded ops[, flag[, mapq]]) tuples, stably sorted by position."""
    items = sorted(items, key=lambda x: x[0])
    assert not items or items[0][0] >= 0
    off = np.zeros(len(items) + 1, np.int64)
    off[1:] = np.cumsum([len(x[1]) for x in items])
    flat = np.fromiter((v for x in items for v in x[1]), np.int64, int(off[-1]))
    return po.Reads(np.array([x[0] for x in items], np.int64).astype(np.int32),
                    np.array([x[2] if len(x) > 2 else 0 for x in items], np.uint16),
                    np.array([x[3] if len(x) > 3 else 60 for x in items], np.uint8), off.astype(np.uint32), flat.astype(np.uint32))


@dataclass
class Case:
    name: str
    edge: str                       # the edge the case claims; tests/test_long_shapes.py asserts it on the model
    lengths: list
    reads: dict                     # tid -> po.Reads
    W: int = 100
    Q: int = 1
    flag_mask: int = 0x704
    min_cov: int = 2
    max_mean_depth: int = 5
    index: bool = True              # the arrival-time position index (OPT_INGEST_INDEX)
    blocks: int = 1                 # the records of a contig are pushed in this many blocks of uneven size
    sparse: bool = False            # contigs too long for a per-base vector: sparse references, per-base dropped only
    simple: bool = False            # millions of reads of one `M` op each: modelled with numpy, not read by read
    family: str = ""
    mark: dict = field(default_factory=dict)

    def get(self, tid):
        return self.reads.get(tid, H.empty_reads())

    @property
    def step_used(self):
        return po.step_for(self.W)

    @property
    def n_tiles(self):
        return sum((L + T - 1) // T for L in self.lengths)


def block_cuts(n, blocks):
    """[0, ..., n]: the records of a contig as `blocks` blocks of uneven size, no cut on a multiple of 64."""
    if blocks == 1 or n < 4 * blocks:
        return [0, n]
    return [0] + [(n * (2 ** k - 1) // (2 ** blocks - 1)) | 1 for k in range(1, blocks)] + [n]


# ---- the per-read routing model -------------------------------------------------------------------------------------

@dataclass
class ReadModel:
    pos: int
    o0: int
    n: int
    cap: int
    pcap: int
    walk: str                       # "none", "serial_dels_plain", "wave_dels_plain", "wave_dels", "serial_dels"
    nd: int
    end: int
    index: str                      # "none", "slot", "search"
    K: int
    batches: int                    # batches wave_dels_plain completed (-1: the read never went there)
    why_again: str                  # what ended wave_dels_plain: "", "big", "pos", "slots"
    why_serial: str                 # what sent the read to its lane: "short", "big", "pos", "" (never)
    starts: np.ndarray              # the final list
    lens: np.ndarray

    @property
    def merged(self):
        return self.walk in ("wave_dels", "serial_dels")


def _split(ops):
    ops = ops.astype(np.int64)
    op, ln = ops & 15, ops >> 4
    cons = _CONSUMES[op] & (ln != 0)
    return ln, cons, cons & _SKIPS[op]


def _plain_lists(pos, ln, cons, dn, saturate):
    clen = np.where(cons, ln, 0)
    start = pos + np.cumsum(clen) - clen
    end = pos + int(clen.sum())
    if saturate:
        start, end = np.minimum(start, POS_CAP), min(end, POS_CAP)
    return start[dn], ln[dn], end


def _merged_lists(pos, ln, cons, dn):
    """serial_dels: neighbouring D/N ops merge, a run that no M follows is dropped, the read ends after its last M."""
    k = np.flatnonzero(cons)
    if not len(k):
        return np.zeros(0, np.int64), np.zeros(0, np.int64), pos
    kind, l = dn[k].astype(np.int64), ln[k]
    x = np.minimum(pos + np.cumsum(l) - l, POS_CAP)
    head = np.ones(len(k), bool)
    head[1:] = kind[1:] != kind[:-1]
    h = np.flatnonzero(head)
    run_start, run_kind = x[h], kind[h]
    run_end = np.append(run_start[1:], min(pos + int(l.sum()), POS_CAP))
    closed = (run_kind == 1) & (np.arange(len(h)) < len(h) - 1)
    counted = np.flatnonzero(run_kind == 0)
    end = int(run_end[counted[-1]]) if len(counted) else pos
    return run_start[closed], np.minimum(run_end[closed] - run_start[closed], POS_CAP), end


def walk_read(ops, pos, o0):
    """What gd_dels_raw_kernel does with one read."""
    n = len(ops)
    cap = ((o0 + n) >> 1) - (o0 >> 1) + 1
    pcap = ((o0 + n) >> 6) - (o0 >> 6) + 3
    e0 = np.zeros(0, np.int64)
    if n == 0:
        return ReadModel(pos, o0, 0, cap, pcap, "none", 0, pos, "none", 0, -1, "", "", e0, e0)
    ln, cons, dn = _split(ops)
    batches, why_again, why_serial = -1, "", "short"
    serial = n <= WAVE_DELS_MIN
    walk = None
    if not serial:
        why_serial = ""
        cur, w, batches = pos, 0, 0
        for b0 in range(0, n, BATCH):
            sl = slice(b0, b0 + BATCH)
            if (cons[sl] & (ln[sl] > OP_MAX)).any():
                why_again = "big"
            elif cur >= PLAIN_POS_CAP:
                why_again = "pos"
            elif w + int(dn[sl].sum()) > cap:
                why_again = "slots"
            if why_again:
                break
            w += int(dn[sl].sum())
            cur += int(ln[sl][cons[sl]].sum())
            batches += 1
        if not why_again:
            walk = "wave_dels_plain"
            starts, lens, end = _plain_lists(pos, ln, cons, dn, False)
        else:                                              # wave_dels: batches of 256 for the op test, groups of 64 for the position
            cur = pos
            for b0 in range(0, n, BATCH):
                sl = slice(b0, b0 + BATCH)
                if (cons[sl] & (ln[sl] > OP_MAX)).any():
                    why_serial = "big"
                    break
                for g0 in range(b0, min(b0 + BATCH, n), WAVE):
                    g = slice(g0, g0 + WAVE)
                    if cons[g].any():
                        if cur >= MERGED_POS_CAP:
                            why_serial = "pos"
                            break
                        cur += int(ln[g][cons[g]].sum())
                if why_serial:
                    break
            if why_serial:
                serial = True
            else:
                walk = "wave_dels"
                starts, lens, end = _merged_lists(pos, ln, cons, dn)
    if serial:
        starts, lens, end = _plain_lists(pos, ln, cons, dn, True)
        walk = "serial_dels_plain"
        if len(starts) > cap:
            walk = "serial_dels"
            starts, lens, end = _merged_lists(pos, ln, cons, dn)
    nd = len(starts)
    K = (end >> PT_SHIFT) - (pos >> PT_SHIFT) + 2 if nd and end >= pos else 0
    index = "none" if K == 0 else "slot" if walk.endswith("plain") and K <= pcap else "search"
    return ReadModel(pos, o0, n, cap, pcap, walk, nd, int(end), index, K, batches, why_again, why_serial,
                     np.asarray(starts, np.int64), np.asarray(lens, np.int64))


@lru_cache(maxsize=None)
def _reads_model(name):
    c = case(name)
    out = {}
    for t in range(len(c.lengths)):
        r = c.get(t)
        off = r.cigar_off.astype(np.int64)
        out[t] = tuple(walk_read(r.cigar[off[i]:off[i + 1]], int(r.pos[i]), int(off[i])) for i in range(r.n))
    return out


def reads_model(c, tid=0):
    """The ReadModel of every read of a contig."""
    return _reads_model(c.name)[tid]


def job_model(c):
    """dict(n_deletions, max_span_seen, lookback) of the job: what gd_stats reports."""
    nd, span = 0, 0
    for t, L in enumerate(c.lengths):
        if L > 0 and c.simple and c.get(t).n:              # one M op of at least one base per read: no deletions, span = its length
            span = max(span, int((c.get(t).cigar >> 4).max()))
        elif L > 0:
            for m in reads_model(c, t):
                nd += m.nd
                span = max(span, m.end - m.pos)
    return dict(n_deletions=nd, max_span_seen=span, lookback=max(64, (span + 63) & ~63))


def model_of_reads(r):
    """[ReadModel] of a po.Reads that belongs to no case (tests/test_gpu_longread.py)."""
    off = r.cigar_off.astype(np.int64)
    return [walk_read(r.cigar[off[i]:off[i + 1]], int(r.pos[i]), int(off[i])) for i in range(r.n)]


def stats_of_reads(r):
    ms = model_of_reads(r)
    span = max([m.end - m.pos for m in ms] + [0])
    return dict(n_deletions=sum(m.nd for m in ms), max_span_seen=span, lookback=max(64, (span + 63) & ~63))


# ---- the tile kernel's model ----------------------------------------------------------------------------------------

@dataclass
class WaveWork:
    candidates: int
    hits: int
    pieces: int
    drains: list                    # queue length at every drain, the last one included
    rounds: list                    # lanes that queued a piece, per round


@dataclass
class TileModel:
    ctg: int
    t0: int
    tend: int
    lo: int
    hi: int
    waves: list                     # NW WaveWork
    hit_reads: list                 # (read, wave, a, b, j0, rem, k0, k1, K, index)

    @property
    def nrd(self):
        return self.hi - self.lo

    @property
    def rows(self):
        """The tile leaves the single-pass phase B: it is clipped or has 2^22 candidate reads and more."""
        return self.tend - self.t0 != T or self.nrd >= WIDE


def kept_mask(r, Q, flag_mask):
    return ((r.flag.astype(np.int64) & flag_mask) == 0) & (r.mapq.astype(np.int64) >= Q)


def tile_model(c, ctg, t0):
    """gd_ltile2_kernel, phase A of one tile."""
    r, ms, L = c.get(ctg), reads_model(c, ctg), c.lengths[ctg]
    lookback = job_model(c)["lookback"]
    tend = min(t0 + T, L)
    pos = r.pos.astype(np.int64)
    frm = t0 - lookback if t0 > lookback else 0
    if c.index:
        frm &= ~63
    lo, hi = int(np.searchsorted(pos, frm, "left")), int(np.searchsorted(pos, tend, "left"))
    kept = kept_mask(r, c.Q, c.flag_mask)
    waves = [WaveWork(0, 0, 0, [], []) for _ in range(NW)]
    qn = [0] * NW
    hit_reads = []
    for base in range(lo, hi, NT):
        rem = np.zeros((NW, WAVE), np.int64)
        for i in range(base, min(base + NT, hi)):
            wv, lane = (i - base) % NW, (i - base) // NW
            m = ms[i]
            waves[wv].candidates += 1
            if not (m.end >= t0 and m.pos < tend and kept[i]):
                continue
            waves[wv].hits += 1
            if m.index == "none":
                continue
            pk = m.pos >> PT_SHIFT
            k0 = (t0 >> PT_SHIFT) - pk if t0 > m.pos else 0
            k1 = min(k0 + (T >> PT_SHIFT), m.K - 1)
            a = int(np.searchsorted(m.starts, (pk + k0) << PT_SHIFT, "left")) if k0 else 0
            b = m.nd if k1 == m.K - 1 else int(np.searchsorted(m.starts, (pk + k1) << PT_SHIFT, "left"))
            j0 = a - 1 if a else 0
            rem[wv, lane] = b - j0
            hit_reads.append((i, wv, a, b, j0, b - j0, k0, k1, m.K, m.index))
        for wv in range(NW):
            left = rem[wv].copy()
            while (left > 0).any():
                n_p = int((left > 0).sum())
                if qn[wv] + n_p > LQ_CAP:
                    waves[wv].drains.append(qn[wv])
                    qn[wv] = 0
                left = np.where(left > 0, left - np.minimum(left, DL_CHUNK), 0)
                qn[wv] += n_p
                waves[wv].pieces += n_p
                waves[wv].rounds.append(n_p)
    for wv in range(NW):
        if qn[wv]:
            waves[wv].drains.append(qn[wv])
    return TileModel(ctg, t0, tend, lo, hi, waves, hit_reads)


@lru_cache(maxsize=None)
def _tile_models(name):
    c = case(name)
    assert not c.sparse
    return tuple(tile_model(c, ctg, t0) for ctg, L in enumerate(c.lengths) for t0 in range(0, L, T))


def tile_models(c):
    return _tile_models(c.name)


def tile_range(c, ctg, t0):
    """(lo, hi, takes phase_b_rows) of one tile: its candidate reads, without the per-read model."""
    pos, L = c.get(ctg).pos.astype(np.int64), c.lengths[ctg]
    lookback = job_model(c)["lookback"]
    tend = min(t0 + T, L)
    lo = int(np.searchsorted(pos, (t0 - lookback if t0 > lookback else 0) & (~63 if c.index else -1), "left"))
    hi = int(np.searchsorted(pos, tend, "left"))
    return lo, hi, tend - t0 != T or hi - lo >= WIDE


def tile_at(c, ctg, t0):
    return next(t for t in tile_models(c) if t.ctg == ctg and t.t0 == t0)


# ---- the references -------------------------------------------------------------------------------------------------

def interval_events(c, tid):
    """(positions, deltas) int64 of depth = sum over kept reads of [pos <= x < end] - sum over list entries of [x in
    entry], from the MODEL's lists and ends, clipped to the contig."""
    r, L = c.get(tid), c.lengths[tid]
    kept = kept_mask(r, c.Q, c.flag_mask)
    if c.simple:
        p = r.pos.astype(np.int64)[kept]
        e = p + (r.cigar.astype(np.int64) >> 4)[kept]
        return np.minimum(np.concatenate([p, e]), L), np.concatenate([np.ones(len(p), np.int64), -np.ones(len(p), np.int64)])
    ms = reads_model(c, tid)
    at, dv = [], []
    for i, m in enumerate(ms):
        if not kept[i]:
            continue
        at += [np.array([m.pos, m.end], np.int64), m.starts, np.minimum(m.starts + m.lens, POS_CAP)]
        dv += [np.array([1, -1], np.int64), np.full(m.nd, -1, np.int64), np.full(m.nd, 1, np.int64)]
    if not at:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    return np.minimum(np.concatenate(at), L), np.concatenate(dv)


def interval_depth(c, tid):
    """int64[length]: the interval reference as a per-base vector."""
    L = c.lengths[tid]
    at, dv = interval_events(c, tid)
    diff = np.bincount(at[dv > 0], minlength=L + 1) - np.bincount(at[dv < 0], minlength=L + 1)     # (every delta is +1 or -1)
    return np.cumsum(diff[:L].astype(np.int64))


def segments(at, dv, L):
    """(starts, values) of the piecewise-constant depth of a difference array given as events: the sparse form."""
    order = np.argsort(at, kind="stable")
    at, dv = at[order], dv[order]
    u, first = np.unique(at, return_index=True)
    val = np.add.reduceat(dv, first) if len(u) else np.zeros(0, np.int64)
    keep = u < L
    starts, values = u[keep], np.cumsum(val)[keep]
    if not len(starts) or starts[0] != 0:
        starts, values = np.append(0, starts), np.append(0, values)
    change = np.ones(len(starts), bool)
    change[1:] = values[1:] != values[:-1]
    return starts[change].astype(np.int64), values[change].astype(np.int64)


def segments_of_depth(depth, a, L):
    """The sparse form of a per-base vector that covers [a, a + len(depth)) of a contig that is zero elsewhere."""
    d = np.concatenate([[0], depth.astype(np.int64), [0]])
    k = np.flatnonzero(d[1:] != d[:-1])
    return segments(a + k, d[k + 1] - d[k], L)


def sparse_results(starts, values, L, W, min_cov, max_mean_depth, step):
    """(window sums int64, minima int32, runs [n, 3] int32) of a piecewise-constant depth."""
    ends = np.append(starts[1:], L)
    integ = np.concatenate([[0], np.cumsum(values * (ends - starts))])
    def F(x):
        k = np.searchsorted(starts, x, "right") - 1
        return integ[k] + values[k] * (x - starts[k])
    edges = np.append(np.arange(0, L, W), L).astype(np.int64)
    sums = F(edges[1:]) - F(edges[:-1])
    mins = values[np.searchsorted(starts, edges[:-1], "right") - 1].copy()     # the segment a window starts in
    for s, v in zip(starts[1:], values[1:]):                                   # ... and every one that starts inside it
        w = int(s // W)
        mins[w] = min(mins[w], v)
    cls = np.where(values == 0, 0, np.where(values < min_cov, 1, np.where((max_mean_depth > 0) & (values >= max_mean_depth), 3, 2)))
    ch = np.ones(len(starts), bool)
    ch[1:] = cls[1:] != cls[:-1]
    at = np.union1d(starts[ch], np.arange(0, L, step, dtype=np.int64))
    rc = cls[np.searchsorted(starts, at, "right") - 1]
    runs = np.stack([at, np.append(at[1:], L), rc], 1).astype(np.int32) if len(at) else np.zeros((0, 3), np.int32)
    return sums.astype(np.int64), mins.astype(np.int32), runs


def busy_range(c, tid):
    """[a, b): every position of a contig that a read can cover, padded."""
    ms = reads_model(c, tid)
    if not ms:
        return 0, 0
    r = c.get(tid)
    reach = int((r.pos.astype(np.int64) + H.ref_span(r)).max())
    return max(0, ms[0].pos - 1000), min(c.lengths[tid], reach + 1000)


@lru_cache(maxsize=None)
def reference(name):
    """Per contig (sums, minima, runs, depth int64 or None) of a case from the interval reference.  Read only."""
    c = case(name)
    out = []
    for t, L in enumerate(c.lengths):
        if c.sparse:
            st, va = segments(*interval_events(c, t), L)
            out.append(sparse_results(st, va, L, c.W, c.min_cov, c.max_mean_depth, c.step_used) + (None,))
        else:
            d = interval_depth(c, t)
            out.append(_dense_results(c, d, L) + (d,))
        for a in out[-1]:
            if a is not None:
                a.setflags(write=False)
    return tuple(out)


def _dense_results(c, d, L, W=0):
    W = W or c.W
    edges = np.arange(0, L, W)
    if not len(edges):
        return np.zeros(0, np.int64), np.zeros(0, np.int32), np.zeros((0, 3), np.int32)
    return (np.add.reduceat(d.astype(np.int64), edges), np.minimum.reduceat(d, edges).astype(np.int32),
            H.oracle_runs(d, c.min_cov, c.max_mean_depth, po.step_for(W)))


@lru_cache(maxsize=None)
def oracle(name, W=0):
    """Per contig (sums, minima, runs, depth int32 or None) of a case from the C oracle (on a sparse case: from its
    per-base vector of the covered stretch, zeros elsewhere), for the case's window size or another.  Read only."""
    c = case(name)
    out = []
    for t, L in enumerate(c.lengths):
        if c.sparse:
            a, b = busy_range(c, t)
            d = po.perbase_c(c.get(t), c.Q, a, b, c.flag_mask)
            st, va = segments_of_depth(d, a, L)
            out.append(sparse_results(st, va, L, W or c.W, c.min_cov, c.max_mean_depth, po.step_for(W or c.W)) + (None,))
        else:
            # (millions of reads over one stretch: the oracle's difference-array walk, not its base-by-base one)
            d = oracle(name)[t][3] if W else po.perbase_c(c.get(t), c.Q, 0, L, c.flag_mask, diff=c.simple)
            out.append(_dense_results(c, d, L, W) + (d,))
        for a in out[-1]:
            if a is not None:
                a.setflags(write=False)
    return tuple(out)


# ---- building blocks ------------------------------------------------------------------------------------------------

def ordinary(k=100):
    """An ordinary long read: 4 k + 1 ops, k single-base deletions, 41 reference bases per period."""
    return cg((M, 20), (D, 1), (M, 20), (I, 1)) * k + cg((M, 5))


def n_op_read(n, dn_every=4, length=13):
    """A read of exactly n ops: M / I / M / D periods, a D/N op in the first and the last op of every batch of 256 and
    in the read's last op; every op code 0 - 8 appears."""
    out = []
    for k in range(n):
        if k % BATCH in (0, BATCH - 1) or k == n - 1:
            out.append(((D, N)[k % 2], 2))
        elif k % dn_every == dn_every - 1:
            out.append((D, 1 + k % 3))
        elif k % 2:
            out.append(((I, S, P, HC)[(k // 2) % 4], 1 + k % 5))
        else:
            out.append(((M, EQ, X)[(k // 2) % 3], length + k % 7))
    return cg(*out)


def dn_read(n, n_dn, neighbours=False, first=M):
    """n ops of which exactly n_dn are D/N ops of one base (spread evenly; `neighbours`: in adjacent pairs D N, so the
    merged count differs from the plain one), the others 9M; the first op is `first`, the last an M."""
    assert n_dn <= n - 2
    ops = [(M, 9)] * n
    ops[0] = (first, 9)
    if neighbours:
        slots = [1 + 3 * (j // 2) + j % 2 for j in range(n_dn)]
        if slots and slots[-1] >= n - 1:
            slots = list(range(1, 1 + n_dn))
    else:
        slots = [1 + (j * (n - 2)) // max(n_dn, 1) for j in range(n_dn)]
    assert len(set(slots)) == n_dn and max(slots, default=0) < n - 1, (n, n_dn)
    for j, s in enumerate(slots):
        ops[s] = ((D, N)[j % 2], 1)
    return cg(*ops)


def pad_ops(k):
    """A read of k ops that consumes nothing (moves the next read's CSR offset)."""
    return cg(*[((I, S, HC, P)[j % 4], 3) for j in range(k)])


class Layout:
    """Reads of one contig in coordinate order, with the CSR offset of the next one."""
    def __init__(self, pos=100, gap=37):
        self.items, self.o, self.pos, self.gap = [], 0, pos, gap

    def add(self, ops, pos=None, flag=0, mapq=60, gap=None):
        if pos is not None:
            assert pos >= self.pos or not self.items
            self.pos = pos
        self.items.append((self.pos, ops, flag, mapq))
        self.o += len(ops)
        self.pos += self.gap if gap is None else gap
        return len(self.items) - 1

    def align(self, mod, want):
        """Pads until the next read's CSR offset is `want` modulo `mod`."""
        k = (want - self.o) % mod
        if k:
            self.add(pad_ops(k))

    def reads(self):
        assert all(a[0] <= b[0] for a, b in zip(self.items, self.items[1:]))
        return reads_of(self.items)


# ---- the cases: the deletion-list pass ------------------------------------------------------------------------------

OP_COUNTS = (0, 1, 24, 25, 255, 256, 257, 258, 511, 512, 513, 514, 767, 768, 769, 770, 1024, 1535, 1536, 1537, 1538)


def dl_count_cases():
    lay, idx = Layout(), {}
    for n in OP_COUNTS:
        for a in range(4):
            lay.align(4, a)
            idx[(n, a)] = lay.add(n_op_read(n), gap=211)
    L = -(-(lay.pos + 40000) // T) * T + 77
    return [Case("dl-op-counts", "reads of 0, 1, 24 | 25, 255 .. 258, 511 .. 514, 767 .. 770, 1024, 1535 .. 1538 ops, each at a CSR "
                 "offset of 0, 1, 2 and 3 modulo 4; a D/N op in the first and last op of every batch and in the last op",
                 [L], {0: lay.reads()}, W=100, family="dl-counts", mark=dict(idx=idx))]


def dl_boundary_cases():
    """300 ops of 16 reference bases each: a batch covers exactly one tile's worth of positions, and read j starts 16 j
    before a tile boundary, so the boundary falls on op j of its batch -- every lane, every element of a lane."""
    ops = cg(*[((M, 16), (EQ, 16), (D, 16))[k % 3] if k % 7 else (N, 16) for k in range(300)])
    items = [(3 * T - 16 * j, ops) for j in range(BATCH)]
    # ... and one base off: the boundary falls inside op j
    items += [(5 * T - 16 * j - 7, ops) for j in range(0, BATCH, 5)]
    return [Case("dl-boundary-in-batch", "a tile boundary on the first base of every op 0 .. 255 of a batch, and inside every "
                 "fifth", [8 * T + 5], {0: reads_of(items)}, W=96, min_cov=100, max_mean_depth=200, family="dl-boundary")]


def dl_nothing_cases():
    lay = Layout()
    nothing = [[], pad_ops(1), pad_ops(7), cg((M, 0), (D, 0), (N, 0)), cg(*[(op, 5) for op in range(9, 16)]),
               pad_ops(30), cg(*[(op % 7 + 9, 5) for op in range(300)]), cg((M, 0)) * 70 + pad_ops(200)]
    for k, ops in enumerate(nothing * 3):
        lay.add(ordinary(3 + k), gap=5)
        lay.add(ops, gap=5)
    lay.add(ordinary(150))
    return [Case("dl-nothing", "reads that consume nothing (I S H P only, zero-length ops, codes 9 - 15; serial and wave walked) "
                 "and reads without ops between ordinary reads", [3 * T], {0: lay.reads()}, family="dl-nothing",
                 mark=dict(n_nothing=len(nothing) * 3))]


def _slot_case(name, edge, n, late_batch=None):
    """Per parity of o0 three reads of n ops with cap - 1, cap and cap + 1 D/N ops (neighbouring D N pairs from cap on), each
    between two neighbours that fill THEIR slots exactly."""
    lay, idx = Layout(gap=3000 if n > 24 else 400), {}
    nb = 9 if n <= 24 else 41
    def neighbour():
        cap = ((lay.o + nb) >> 1) - (lay.o >> 1) + 1
        lay.add(dn_read(nb, cap))
    for parity in (0, 1):
        for d in (-1, 0, 1):
            lay.align(2, (parity - nb) % 2)
            neighbour()
            o0 = lay.o
            cap = ((o0 + n) >> 1) - (o0 >> 1) + 1
            if late_batch is None:
                ops = dn_read(n, cap + d, neighbours=d >= 0)
            else:                                          # the slots run out in batch `late_batch`: M D pairs, then D N D N ...
                k = cap + d - (BATCH // 2) * late_batch
                ops = cg((M, 9), (D, 1)) * ((BATCH // 2) * late_batch) + cg((D, 1), (N, 1)) * (k // 2) + cg((D, 1)) * (k % 2)
                assert BATCH * late_batch < len(ops) <= BATCH * (late_batch + 1)
                ops += cg((M, 9)) * (n - len(ops))
            assert len(ops) == n and o0 % 2 == parity
            idx[(parity, d)] = lay.add(ops)
            neighbour()
    L = -(-(lay.pos + 12 * n) // T) * T + 9
    return Case(name, edge, [L], {0: lay.reads()}, W=100, family="dl-slots", mark=dict(idx=idx, n=n, late=late_batch))


def dl_slot_cases():
    return [_slot_case("dl-slots-serial", "cap - 1, cap, cap + 1 D/N ops on the lane's walk (24 ops), even and odd CSR offset", 24),
            _slot_case("dl-slots-wave", "cap - 1, cap, cap + 1 D/N ops on the wave's walk (25 ops)", 25),
            _slot_case("dl-slots-batch-1", "the slots run out in the first batch of the wave walk", 296, 0),
            _slot_case("dl-slots-batch-2", "the slots run out in the second batch of the wave walk", 552, 1),
            _slot_case("dl-slots-batch-4", "the slots run out in the fourth batch of the wave walk", 1064, 3)]


def dl_index_cases():
    out = []
    # K = pcap - 1, pcap, pcap + 1: a read of 40 ops owns pcap = 3 (4 when it crosses a multiple of 64) entries
    lay, idx = Layout(pos=T + 10, gap=0), {}
    for a in (0, 1, 62, 63):
        for d in (-1, 0, 1):
            lay.align(64, a)
            o0, n = lay.o, 40
            pcap = ((o0 + n) >> 6) - (o0 >> 6) + 3
            K = pcap + d                                   # the read spans K - 2 boundaries
            p = (lay.pos // T + 1) * T + 10
            span = (K - 2) * T if K > 2 else 1000          # K = 2: inside one tile
            ops = cg((M, 50), (D, 3)) + cg((M, 30), (I, 1)) * 18 + cg((M, span - 53 - 540 + 5), (D, 2))
            assert len(ops) == n
            idx[(a, d)] = lay.add(ops, pos=p)
            # the next read's first index entry lies directly behind this one's slots; a tile reads it
            lay.add(cg((M, 10), (D, 4), (M, 90)), pos=p + 5)
            lay.pos = p + span
    L = (lay.pos // T + 2) * T
    out.append(Case("dl-index-slots", "K = pcap - 1, pcap, pcap + 1 index entries at CSR offsets 0, 1, 62, 63 modulo 64, directly "
                    "before a read whose first index entry a tile reads", [L], {0: lay.reads()}, W=1000, family="dl-index",
                    mark=dict(idx=idx)))
    # the walk's clamp, many entries early
    lay, idx = Layout(gap=900), {}
    lay.add(ordinary(60))
    idx["3op"] = lay.add(cg((M, 50), (N, 100000), (M, 50)))
    lay.add(ordinary(60))
    for where, at in (("first", 30), ("middle", 150), ("last", 290)):
        ops = cg((M, 10), (D, 2)) * 150
        ops[at] = cg((N, 300000))[0]
        assert len(ops) == 300
        idx[where] = lay.add(ops)
        lay.add(ordinary(60))
    L = -(-(lay.pos + 310000) // T) * T + 123
    out.append(Case("dl-index-clamp", "the index walk's clamp many entries early: a 3-op read over 100 kb (serial), 300-op reads "
                    "with one 300 kb skip in the first, a middle and the last batch", [L], {0: lay.reads()}, W=250,
                    family="dl-index", mark=dict(idx=idx)))
    return out


def dl_merged_cases():
    """Reads that pass their slots (more D/N ops than cap) and have more than 24 ops: wave_dels."""
    dd = lambda k: cg((D, 1), (N, 2)) * (k // 2) + cg((D, 1)) * (k % 2)
    lay, idx = Layout(gap=700), {}
    def add(key, ops):
        lay.add(ordinary(20))
        idx[key] = lay.add(ops)
    flood = dd(400)                                       # what takes every one of these reads past its slots
    for g in (1, 2, 5):                                    # a run over g whole groups of 64 ops without a head
        add("run-%d" % g, cg((M, 9)) * 63 + dd(1) + dd(64 * g) + cg((M, 9)) * 40 + flood + cg((M, 5)))
    add("head-0", cg((M, 9)) * 64 + dd(1) + cg((M, 9)) * 63 + flood + cg((M, 5)))             # a head in lane 0 of group 1
    add("head-63", cg((M, 9)) * 63 + dd(1) + cg((M, 9)) * 64 + flood + cg((M, 5)))            # a head in lane 63 of group 0
    add("close-next-batch", cg((M, 9)) * 200 + dd(56) + cg((M, 9)) * 30 + flood + cg((M, 5)))   # the run closes in lane 0 of batch 1
    add("trailing", cg((M, 9)) * 30 + flood + cg((M, 7)) + dd(33))
    add("leading", dd(37) + cg((M, 9)) * 30 + flood + cg((M, 7)))
    add("only-dn", dd(300))
    add("only-dn-short", dd(24))
    lay.add(ordinary(100))
    L = -(-(lay.pos + 9000) // T) * T + 31
    out = [Case("dl-merged", "wave_dels: runs over 1, 2, 5 whole groups without a head, heads in lane 0 and lane 63, a run that closes "
                "in the first lane of the next batch, a trailing and a leading D/N run, only D/N ops", [L], {0: lay.reads()},
                W=100, family="dl-merged", mark=dict(idx=idx))]
    # an op of exactly 2^22 bases and of 2^22 + 1, on the plain and on the merged walk
    lay, idx = Layout(gap=50), {}
    for big in (OP_MAX, OP_MAX + 1):
        for merged in (False, True):
            body = cg((M, 30), (D, 2)) * 20 + cg((N, big)) + cg((M, 30), (D, 2)) * 20 + cg((M, 10))
            if merged:
                body = cg((M, 30)) + dd(200) + cg((M, 5), (N, big)) + cg((M, 30), (D, 2)) * 20 + cg((M, 10))
            lay.add(ordinary(30))
            idx[(big - OP_MAX, merged)] = lay.add(body)
    lay.add(ordinary(30))
    L = -(-(lay.pos + OP_MAX + 9000) // T) * T
    out.append(Case("dl-op-2^22", "an op of exactly 2^22 bases (stays on the wave walks) and of 2^22 + 1 (the lane's), on the plain "
                    "and on the merged walk", [L], {0: lay.reads()}, W=4000, family="dl-merged", mark=dict(idx=idx)))
    return out


def _unit_contig(n, wave_lanes):
    """n reads; those whose index modulo 64 is in wave_lanes have 60 ops (the wave walks them), the others 5."""
    items = []
    for i in range(n):
        ops = cg((M, 7), (D, 1), (M, 7), (I, 2)) * 15 if i % 64 in wave_lanes else cg((M, 20), (D, 2), (M, 9), (N, 3), (M, 4))
        items.append((10 + 13 * i, ops, 0x400 if i % 11 == 5 else 0))
    return reads_of(items)


def dl_unit_cases():
    counts = (63, 64, 65, 255, 256, 257)
    lanes = ((0,), (63,), (0, 63), tuple(range(64)), (5,), (0, 31, 63))
    lens = [10 + 13 * n + 500 for n in counts]
    reads = {t: _unit_contig(n, lanes[t]) for t, n in enumerate(counts)}
    out = [Case("dl-units", "63, 64, 65, 255, 256, 257 reads on a contig (units of 64, four units per workgroup); the wave-walked "
                "read in lane 0, in lane 63, in every lane", lens, reads, W=100, family="dl-units", mark=dict(counts=counts, lanes=lanes))]
    counts5 = (0, 1, 64, 65, 0)
    out.append(Case("dl-contigs-5", "five contigs in one job with 0, 1, 64, 65 and 0 reads: batch_find and ubeg", [T + 1, 900, 2 * T, T - 1, 700],
                    {t: _unit_contig(n, (0, 63)) for t, n in enumerate(counts5) if n}, W=64, family="dl-units", mark=dict(counts=counts5)))
    for nb in (2, 3):
        out.append(Case("dl-blocks-%d" % nb, "the same records pushed in %d blocks of uneven size" % nb, lens[3:], {t: reads[t + 3] for t in range(3)},
                        W=100, blocks=nb, family="dl-units"))
    return out


def dl_poscap_cases():
    """Four contigs, each just long enough for one read of 300 ops and deletions at a position cap."""
    long, short = cg((M, 30), (D, 2), (M, 9), (N, 5)) * 75, cg((M, 30), (D, 2), (M, 9), (N, 5)) * 15
    starts = (PLAIN_POS_CAP - 1, PLAIN_POS_CAP, MERGED_POS_CAP - 1, MERGED_POS_CAP)
    lens = [min(p + 75 * 46 + 70000, 0x7fff0000) for p in starts]
    reads = {t: reads_of([(p - 500000, ordinary(50)), (p, short if t >= 2 else long), (p + 100, ordinary(50))]) for t, p in enumerate(starts)}
    # ... and 300 ops one base before the merging wave walk's cap: its first group of 64 passes, its second does not
    reads[3] = reads_of([(MERGED_POS_CAP - 1, long), (MERGED_POS_CAP, short), (MERGED_POS_CAP + 100, ordinary(50))])
    return [Case("dl-pos-caps", "a read of 300 ops at POS_CAP - 2^30 - 1 (plain wave walk: one batch, then it gives up), at POS_CAP - "
                 "2^30 (gives up at once, the merging wave walk takes it); a read of 60 ops at POS_CAP - 2^28 - 1 (the merging wave "
                 "walk's one group) and at POS_CAP - 2^28 (the lane); 300 ops at POS_CAP - 2^28 - 1 (the lane, from the second group)",
                 lens, reads, W=65536, sparse=True, family="dl-poscap", mark=dict(starts=starts))]


# ---- the cases: the tile kernel -------------------------------------------------------------------------------------

def lt_candidate_cases():
    out = []
    t0 = 2 * T
    for n in (255, 256, 257, 511, 513):
        for which in ("wave0", "wave3", "all"):
            items = []
            for i in range(n):
                # candidate i of the tile (lo = 0 here: the look-back reaches the contig's start) belongs to wave i % 4
                reaches = which == "all" or i % NW == (0 if which == "wave0" else 3)
                p = 100 + 5 * i
                ops = cg((M, t0 - p + 50 + i % 40), (D, 3), (M, 40)) if reaches else cg((M, 30), (D, 2), (M, 10 + i % 9))
                flag, mapq = (0x400, 60) if i % 6 == 2 else (0, 0) if i % 6 == 5 else (0, 60)
                items.append((p, ops, flag, mapq))
            out.append(Case("lt-cand-%d-%s" % (n, which), "%d candidate reads in a tile's range, every third filtered, hits in %s" %
                            (n, {"wave0": "wave 0 only", "wave3": "wave 3 only", "all": "all waves"}[which]), [3 * T],
                            {0: reads_of(items)}, family="lt-candidates", mark=dict(t0=t0, n=n, which=which)))
    return out


def lt_geometry_cases():
    out = []
    t0, tend = 2 * T, 3 * T
    items = [(100, cg((M, 50)))]
    for e in (t0 - 1, t0, t0 + 1, tend - 1, tend, tend + 1):
        items.append((t0 - 700, cg((M, 300), (D, 5), (M, e - (t0 - 700) - 305))))
    for p in (t0 - 1, t0, tend - 1, tend):
        items.append((p, cg((M, 3), (D, 2), (M, 30))))
    out.append(Case("lt-read-edges", "reads that end on t0 - 1, t0, t0 + 1, tend - 1, tend, tend + 1 and start on t0 - 1, t0, tend - 1, tend",
                    [5 * T], {0: reads_of(items)}, family="lt-geometry", mark=dict(t0=t0)))
    for index in (True, False):
        for k, span in enumerate((64 * 70 - 1, 64 * 70, 64 * 70 + 1)):
            for de in (-1, 0, 1):
                items = [(50, cg((M, 40), (D, 2), (M, 40)))]
                items.append((t0 + de - span, cg((M, 100), (D, 7), (M, span - 107))))           # the job's longest read
                items += [(t0 - 3000 + 50 * i, cg((M, 60), (D, 1), (M, 60))) for i in range(100)]
                out.append(Case("lt-lookback-%d-%+d-%s" % (span, de, "index" if index else "noindex"),
                                "the longest read of the job spans %d and ends on t0 %+d: the look-back rounding" % (span, de),
                                [4 * T], {0: reads_of(items)}, index=index, family="lt-geometry", mark=dict(t0=t0, span=span, de=de)))
    return out


def lt_deletion_cases():
    out = []
    t0, tend = 2 * T, 3 * T
    for search in (False, True):
        items = []
        def read(p, ops):
            # the index: 256 more ops behind it, enough index slots for every tile the read spans.  PT_SEARCH: a D N flood
            # behind it takes the read past its list slots (merged list, no index)
            items.append((p, ops + (cg((D, 1), (N, 1)) * 30 + cg((M, 5)) if search else cg((M, 1), (I, 1)) * 128)))
        p0 = T + 100
        for e in (t0 - 1, t0, t0 + 1):                     # starts before t0, ends on e
            read(p0, cg((M, 3000), (D, e - (p0 + 3000)), (M, 200)))
        for s in (t0 - 1, t0, tend - 1, tend):             # starts on s
            read(p0 + 10, cg((M, s - (p0 + 10)), (D, 3), (M, 50)))
        read(p0 + 20, cg((M, 500), (D, 2 * T + 3000), (M, 500)))                     # over the whole tile and more
        read(p0 + 30, cg((M, t0 - p0 - 30 - 100), (D, 150), (M, 10)))            # the reach-in deletion is the read's first (a = 1)
        read(t0 + 50, cg((M, 10), (D, 3), (M, 10)))                              # none reaches in (a = 0), first and last tile at once
        # deletions elsewhere, none in tile t0: rem = 0 behind j0 (the last one before the tile ends before it)
        read(100, cg((M, 100), (D, 5), (M, 4 * T), (D, 5), (M, 50)))
        # k0 = 0 in its first tile, k1 clamped to K - 1 in its last
        read(t0 + 10, cg((M, 100), (D, 2), (M, T), (D, 2), (M, 80)))
        out.append(Case("lt-deletions-%s" % ("search" if search else "index"), "deletions that start before t0 and end on t0 - 1, t0, t0 + 1; "
                        "start on t0 - 1, t0, tend - 1, tend; span the tile; reach in as the read's first; a tile without any of a "
                        "read's deletions; a read's first and last tile -- through %s" % ("PT_SEARCH" if search else "the index"),
                        [6 * T], {0: reads_of(items)}, W=128, family="lt-deletions", mark=dict(t0=t0, search=search)))
    # PT_SEARCH lists of 1, 2 and 200 entries, bounds before the first and after the last entry
    items = []
    for nd in (1, 2, 200):
        ops = cg((M, 3 * T + 100)) + cg((D, 2), (M, 3)) * nd + cg((M, 40), (EQ, 12 * T), (M, 3 * T))
        items.append((100, ops))
    out.append(Case("lt-search-lists", "PT_SEARCH over lists of 1, 2 and 200 entries: tiles before the first entry, between, after the last",
                    [20 * T], {0: reads_of(items)}, W=1000, family="lt-deletions", mark=dict(search=True)))
    return out


def lt_queue_cases():
    out = []
    t0 = T
    for nd in (63, 64, 65, 128, 129, 2048):
        ops = cg((M, 10)) + cg((D, 1), (M, 1)) * nd + cg((M, 10))
        items = [(t0 - 10, ops), (t0 + 30, cg((M, 50), (D, 2), (M, 50))), (50, cg((M, 80)))]
        out.append(Case("lt-pieces-%d" % nd, "one read with %d single-base deletions two bases apart inside one tile" % nd, [3 * T],
                        {0: reads_of(items)}, W=64, family="lt-queue", mark=dict(t0=t0, nd=nd)))
    # one wave: 64 hits of 2 pieces each (128 items exactly), and one more item
    two = cg((M, 4)) + cg((D, 1), (M, 1)) * 65 + cg((M, 4))          # 65 deletions: pieces of 64 and 1
    one = cg((M, 4), (D, 1), (M, 4))
    for extra, waves in ((0, (0,)), (1, (0,)), (1, (0, 1, 2, 3))):
        items = []
        for i in range(NT + (NW if extra else 0)):
            mine = i % NW in waves
            items.append((t0 + 10 + i, (two if i < NT else one) if mine else cg((M, 30))))
        name = "lt-queue-%d%s" % (128 + extra, "-all" if len(waves) > 1 else "")
        out.append(Case(name, "%s 64 hits x 2 pieces = 128 items%s" % ("every wave queues" if len(waves) > 1 else "wave 0 queues",
                        " and one more: a drain before the round that would pass 128" if extra else " exactly: one drain, at the end"),
                        [3 * T], {0: reads_of(items)}, W=64, family="lt-queue", mark=dict(t0=t0, extra=extra, waves=waves)))
    # rounds of 1 .. 5 queued items (fetch4's tail), a lane that still queues while all others are done
    for k in (1, 2, 3, 4, 5):
        items = []
        for i in range(k):
            nd = 64 * 3 + 5 if i == 0 else 3                  # read 0 queues four pieces, the others one
            items.append((t0 + 10 + i, cg((M, 4)) + cg((D, 1), (M, 1)) * nd + cg((M, 4))))
        # all in wave 0: candidates 0, 4, 8 ... (the reads between belong to the other waves and have no deletions)
        spaced = []
        for i, it in enumerate(items):
            spaced.append(it)
            spaced += [(it[0], cg((M, 20)))] * (NW - 1)
        out.append(Case("lt-rounds-%d" % k, "a first round of %d queued items in one wave, then one lane that queues alone" % k, [3 * T],
                        {0: reads_of(spaced)}, W=64, family="lt-queue", mark=dict(t0=t0, k=k)))
    return out


def lt_clipped_cases():
    lens = [T - 1, T + 1, 1, 2 * T + 700]
    reads = {}
    for t, L in enumerate(lens):
        items = [(max(0, L - 900), cg((M, 300), (D, 5), (M, 700))), (0, cg((M, 1), (D, 1), (M, 1)))]
        items += [(p, cg((M, 40), (D, 3), (M, 40), (N, 9), (M, 20))) for p in range(0, max(L - 50, 1), 97)]
        reads[t] = reads_of(items)
    return [Case("lt-clipped", "contigs of T - 1, T + 1 and 1 positions: the last tile takes phase_b_rows", lens, reads, W=100,
                 family="lt-clipped")]


def lt_wide_cases():
    """2^22 - 1 and 2^22 candidate reads of one M op over 64 positions of one tile, built with numpy.  Every read is kept
    and covers the tile's whole second quarter: with 2^22 of them the quarter's share of the window sum is 2^22 * 1024 =
    2^32, one more than the single-pass phase B's 32-bit accumulators hold; with 2^22 - 1 it still fits."""
    out = []
    for n in (WIDE - 1, WIDE):
        i = np.arange(n, dtype=np.int64)
        pos = T + i * 64 // n
        ln = 3000 + i % 7
        r = po.Reads(pos.astype(np.int32), np.zeros(n, np.uint16), np.full(n, 60, np.uint8), np.arange(n + 1, dtype=np.uint32),
                     (ln << 4).astype(np.uint32))
        out.append(Case("lt-wide-%d" % n, "%d candidate reads in one full tile: %s" % (n, "the single-pass phase B still" if n < WIDE else
                        "phase_b_rows"), [3 * T], {0: r}, W=T, min_cov=100000, max_mean_depth=500000, simple=True, family="lt-wide",
                        mark=dict(t0=T, n=n)))
    return out


def _all_cases():
    out = (dl_count_cases() + dl_boundary_cases() + dl_nothing_cases() + dl_slot_cases() + dl_index_cases() + dl_merged_cases() +
           dl_unit_cases() + dl_poscap_cases() + lt_candidate_cases() + lt_geometry_cases() + lt_deletion_cases() +
           lt_queue_cases() + lt_clipped_cases() + lt_wide_cases())
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return out


DL_FAMILIES = ("dl-counts", "dl-boundary", "dl-nothing", "dl-slots", "dl-index", "dl-merged", "dl-units", "dl-poscap")
LT_FAMILIES = ("lt-candidates", "lt-geometry", "lt-deletions", "lt-queue", "lt-clipped", "lt-wide")
FAMILIES = DL_FAMILIES + LT_FAMILIES
_BUILT = {}


def case(name):
    if not _BUILT:
        _BUILT.update((c.name, c) for c in _all_cases())
    return _BUILT[name]


def names(family=None):
    case("dl-op-counts")
    return [n for n, c in _BUILT.items() if family is None or c.family == family]
