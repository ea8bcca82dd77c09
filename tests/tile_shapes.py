"""Shapes for the short-read tile kernels (gd_prep_kernel, gd_tile_fast_kernel, gd_tile_kernel / gd_tile_slow_kernel,
phase C and the read-back) at the kernels' own thresholds, with the two things a test needs to trust them: a second
reference that is independent of the C oracle, and a plain model of the routing that says whether a shape reaches the
edge it is named for.

Test infrastructure only, no pytest marks: tests/test_tile_shapes.py (CPU) shows that every case hits its edge and that
both references agree; tests/test_gpu_tile_shapes.py runs every case on the device on every tile route.

The routing model is written from the code and comments of goleft_amd/csrc/gd_kernels.hpp (gd_prep_kernel),
gd_tile_fast.hpp, gd_tile_generic.hpp, gd_tile_common.hpp and gd_api_compute.inc:
  * a tile is T = 4096 positions; its candidate reads are [lo, hi): hi the first read at or past the (clipped) tile
    end, lo the first read at or past `from` = t0 - lookback (0 when t0 <= lookback).  With the arrival-time position
    index `from` is rounded DOWN to a multiple of 64; on the straight-line route lo is then rounded down to a multiple
    of 4.  nrd = hi - lo, nst = the ops of those reads;
  * a tile is ORDINARY when it is full (tend - t0 == T), nrd <= 1024 and nst <= 1280; every other tile of a fast run
    is on the slow list (gd_stats.n_slow_tiles) and runs gd_tile_slow_kernel, the generic kernel's body;
  * straight-line kernel, phase A: a lane takes FOUR CONSECUTIVE reads.  A kept read (no masked flag bit, MAPQ >= Q,
    at least one op) of one or two ops is ONE interval computed inline; a kept read of three or more ops takes a rank
    in the workgroup queue: ranks below 120 are queued and walked after the barrier, the others are walked in place
    by their own lane.  Which read gets which rank depends on the order in which the four waves reach the queue's
    counter; inside one wave the order is slot-major (all first reads of the lanes, then all second reads, ...);
  * generic kernel, phase A: batches of NT * U = 1024 candidate reads; in EVERY batch, the first included, thread
    `tid`, slot `u` handles read base + tid + u * NT.  Only a kept read of one `M` op with 1 .. 2^28 - 1 bases is
    simple; every other kept read (one `=`, `X`, `D`, `S`, `0M`; two ops and more) goes to the wave's 64-entry queue.
    A batch that would take the queue past 64 drains it first; a batch with more than 64 such reads of one wave goes
    slot by slot.  The ops are staged in LDS when nst <= 1536 and read from global memory otherwise;
  * phase B: a wave owns a quarter of 1024 positions, four rows of 256, four positions per lane.  Per quarter the
    prep kernel resolves win0 (window of the first position), wleft (positions to the next window boundary, 1 .. W)
    and sleft (positions to the next forced run break, 0 = on the first position).  A row takes one of three window
    paths: no boundary; exactly one (split at lane `rel >> 2`, the straddling lane fixed by `rel & 3`); several.
    The class work of a whole quarter is skipped unless any_noisy: a depth below max(min_cov, 1) in the quarter, a
    depth at or above max_mean_depth, the carry (the depth just before the quarter) outside CALLABLE, or a forced
    break inside;
  * phase C adds a tile's boundary count to the counter of its group of SUPER = 1024 tiles; the host reads the first
    kSpecBounds = 4096 ordered boundaries back with the counters and copies the list again when there are more.
The look-back: gd_set_params with max_span_hint > 0 PINS it (gd_api.hip: lookback = hint, lookback_pinned; neither the
span measured as records arrive nor the tightening after a compute touch a pinned look-back), so every case here gives
a hint and the model knows the look-back of every attempt: the hint, and after a kept read that spans more,
(span + 63) & ~63 with one re-run (gd_api_compute.inc compute_complete: `max_span > lookback`).
The model's constants are restated here, not imported; kernel_constants() reads the headers' text and
tests/test_tile_shapes.py holds the two against each other."""
import os
import re
from dataclasses import dataclass, field
from functools import lru_cache

import numpy as np

from oracle import pyoracle as po
from tests import helpers as H
from tests import sums_shapes as S

T, NT, WAVE, NW, CHUNK, ROWS, U = 4096, 256, 64, 4, 1024, 4, 4
ORD_READS, FAST_CQ, QCAP, GEN_CQ, SUPER, SPEC = 1024, 1280, 120, 1536, 1024, 4096
FAST_BIG = 0x3fffffff
FAST_FAR = FAST_BIG - 65536
SPAN_SAT = 1 << 28
DEFAULT_LOOKBACK = 512
CAP_RUNS0 = 1 << 16                  # initial capacity of the boundary list (for jobs of fewer than 2^15 tiles)
COUNTED, CONSUMING = S.COUNTED, S.CONSUMING


def kernel_constants():
    """The constants of the tile kernels that the model restates, read from the sources' text."""
    def text(name):
        with open(os.path.join(H.ROOT, "goleft_amd", "csrc", name)) as f:
            return f.read()
    k, fast, gen, st = text("gd_kernels.hpp"), text("gd_tile_fast.hpp"), text("gd_tile_generic.hpp"), text("gd_api_state.hpp")
    num = lambda pattern, s: int(re.search(pattern, s).group(1))
    t = num(r"constexpr int T = (\d+);", k)
    mul, div = re.search(r"constexpr int CQ = \(T \* (\d+)\) / (\d+);", gen).groups()
    return {"T": t, "NT": num(r"constexpr int NT = (\d+);", k), "FAST_CQ": num(r"constexpr int FAST_CQ = (\d+);", k),
            "QCAP": num(r"constexpr int QCAP = (\d+);", fast), "U": num(r"constexpr int U = (\d+);", fast),
            "U_generic": num(r"constexpr int U = (\d+);", gen), "CQ": t * int(mul) // int(div),
            "SUPER": num(r"constexpr int SUPER = (\d+);", k), "ordinary_reads": num(r"nrd <= (\d+)u &&", k),
            "spec": num(r"constexpr size_t kSpecBounds = (\d+);", st),
            "lookback": num(r"constexpr int kDefaultLookback = (\d+);", st),
            "far": FAST_BIG - num(r"constexpr int FAST_FAR = FAST_BIG - (\d+);", k),
            "big": int(re.search(r"constexpr int FAST_BIG = (0x[0-9a-f]+);", k).group(1), 16)}


# ---- the case -------------------------------------------------------------------------------------------------------

@dataclass
class Case:
    name: str
    edge: str                       # the edge the case claims; tests/test_tile_shapes.py asserts it on the model
    lengths: list
    reads: dict                     # tid -> po.Reads
    W: int = 100
    Q: int = 1
    flag_mask: int = 0x704
    min_cov: int = 4
    max_mean_depth: int = 0
    step: int = 0
    hint: int = 512                 # max_span_hint: the pinned look-back of the first attempt
    index: bool = True              # the arrival-time position index (OPT_INGEST_INDEX)
    fresh: bool = False             # needs an engine context of its own (the boundary list's capacity is part of it)
    family: str = ""
    mark: dict = field(default_factory=dict)     # positions / tiles the case is about, for its model assertion

    def get(self, tid):
        return self.reads.get(tid, H.empty_reads())

    @property
    def step_used(self):
        return self.step or po.step_for(self.W)

    @property
    def n_tiles(self):
        return sum((L + T - 1) // T for L in self.lengths)


def reads_of(items):
    """po.Reads from (pos, cigar[, flag[, mapq]]) tuples, stably sorted by position."""
    items = sorted(items, key=lambda x: x[0])
    flag = np.array([x[2] if len(x) > 2 else 0 for x in items], np.uint16)
    mapq = np.array([x[3] if len(x) > 3 else 60 for x in items], np.uint8)
    return S.make_reads([x[0] for x in items], [x[1] for x in items], flag, mapq)


# ---- the second reference -------------------------------------------------------------------------------------------

def ref_depth(r, Q, flag_mask, length):
    """int64[length]: +1 / -1 per counted interval (M = X; D and N advance; everything else nothing) in a difference
    array, then its running sum."""
    s, e = S.counted_intervals(r, Q, flag_mask, length)
    diff = np.zeros(length + 1, np.int64)
    np.add.at(diff, s, 1)
    np.add.at(diff, e, -1)
    return np.cumsum(diff[:length])


def ref_windows(depth, W):
    """(int64 sums, int32 minima) of the W-anchored windows, positions inside the contig only."""
    edges = np.arange(0, len(depth), W)
    if not len(edges):
        return np.zeros(0, np.int64), np.zeros(0, np.int32)
    return np.add.reduceat(depth, edges), np.minimum.reduceat(depth, edges).astype(np.int32)


def ref_classes(depth, min_cov, max_mean_depth):
    cls = np.full(len(depth), 2, np.int8)
    if max_mean_depth > 0:
        cls[depth >= max_mean_depth] = 3
    cls[depth < min_cov] = 1
    cls[depth == 0] = 0
    return cls


def ref_boundaries(depth, min_cov, max_mean_depth, step):
    """(int64 positions, int8 classes): wherever the class changes, position 0 and every multiple of `step`."""
    cls = ref_classes(depth, min_cov, max_mean_depth)
    b = np.zeros(len(depth), bool)
    b[1:] = cls[1:] != cls[:-1]
    b[::step] = True
    at = np.flatnonzero(b)
    return at, cls[at]


def runs_of(at, cls, length):
    """[(start, end, class)] int32 rows from boundaries: what gd_callable returns."""
    if not len(at):
        return np.zeros((0, 3), np.int32)
    return np.stack([at, np.append(at[1:], length), cls], 1).astype(np.int32)


@lru_cache(maxsize=None)
def reference(name):
    """Per contig (depth int64, sums, minima, boundary positions, classes) of a case.  Computed once; read only."""
    c = case(name)
    out = []
    for t, L in enumerate(c.lengths):
        d = ref_depth(c.get(t), c.Q, c.flag_mask, L)
        ws, wm = ref_windows(d, c.W)
        at, cl = ref_boundaries(d, c.min_cov, c.max_mean_depth, c.step_used)
        for a in (d, ws, wm, at, cl):
            a.setflags(write=False)
        out.append((d, ws, wm, at, cl))
    return tuple(out)


@lru_cache(maxsize=None)
def oracle(name):
    """Per contig (depth int32, sums, minima, runs [n, 3]) of a case from the C oracle.  Computed once; read only."""
    c = case(name)
    out = []
    for t, L in enumerate(c.lengths):
        d = po.perbase_c(c.get(t), c.Q, 0, L, c.flag_mask)
        edges = np.arange(0, L, c.W)
        ws, wm = np.add.reduceat(d.astype(np.int64), edges), np.minimum.reduceat(d, edges)
        runs = H.oracle_runs(d, c.min_cov, c.max_mean_depth, c.step_used)
        for a in (d, ws, wm, runs):
            a.setflags(write=False)
        out.append((d, ws, wm, runs))
    return tuple(out)


# ---- the routing model ----------------------------------------------------------------------------------------------

def kept_mask(r, Q, flag_mask):
    nops = np.diff(r.cigar_off.astype(np.int64))
    return ((r.flag.astype(np.int64) & flag_mask) == 0) & (r.mapq.astype(np.int64) >= Q) & (nops > 0)


def lookback_of(c, compute=1):
    """(look-back of the last attempt, re-runs for the look-back, largest span of a kept read): see the module text.
    Without a hint (and without the index, whose span measurement would set the look-back as the records arrive) the
    first compute of a data set uses the default of 512 and leaves max(64, (span + 63) & ~63) to the next one when
    that is at most half of it (compute_complete: `want * 2 <= lookback`); `compute` = 2 asks for that one."""
    span = 0
    for t in range(len(c.lengths)):
        r = c.get(t)
        if r.n:
            k = kept_mask(r, c.Q, c.flag_mask)
            if k.any():
                span = max(span, int(np.minimum(H.ref_span(r)[k], SPAN_SAT).max()))
    if c.hint == 0:
        assert not c.index and 0 < span <= DEFAULT_LOOKBACK
        want = max(64, (span + 63) & ~63)
        return (want if compute == 2 and want * 2 <= DEFAULT_LOOKBACK else DEFAULT_LOOKBACK, 0, span)
    return (c.hint, 0, span) if span <= c.hint else ((span + 63) & ~63, 1, span)


@dataclass
class Tile:
    ctg: int
    t0: int
    tend: int
    lo_search: int                  # before the straight-line route's rounding
    lo: int
    hi: int
    nrd: int
    nst: int
    ordinary: bool


@lru_cache(maxsize=None)
def _tiles(name, fast):
    c = case(name)
    lookback = lookback_of(c)[0]
    out = []
    for ctg, L in enumerate(c.lengths):
        r = c.get(ctg)
        pos, off = r.pos.astype(np.int64), r.cigar_off.astype(np.int64)
        for t0 in range(0, L, T):
            tend = min(t0 + T, L)
            frm = t0 - lookback if t0 > lookback else 0
            if c.index:
                frm &= ~63
            lo_s = int(np.searchsorted(pos, frm, "left"))
            hi = int(np.searchsorted(pos, tend, "left"))
            lo = lo_s & ~3 if fast else lo_s
            nrd, nst = hi - lo, int(off[hi] - off[lo])
            out.append(Tile(ctg, t0, tend, lo_s, lo, hi, nrd, nst,
                            tend - t0 == T and nrd <= ORD_READS and nst <= FAST_CQ))
    return tuple(out)


def tiles(c, fast=True):
    """Every tile of the job, in tile order, as gd_prep_kernel resolves it on the last attempt."""
    return _tiles(c.name, fast)


def tile_at(c, ctg, t0, fast=True):
    return next(t for t in tiles(c, fast) if t.ctg == ctg and t.t0 == t0)


def n_slow(c):
    return sum(not t.ordinary for t in tiles(c))


def fast_phase_a(c, t):
    """Straight-line kernel, phase A of one ordinary tile: dict(inline, multi, queued, walked, by_wave) -- by_wave the
    reads of three or more ops per wave (lane = (i - lo) // 4, wave = lane // 64), slots the set of their slots."""
    r = c.get(t.ctg)
    nops = np.diff(r.cigar_off.astype(np.int64))[t.lo:t.hi]
    kept = kept_mask(r, c.Q, c.flag_mask)[t.lo:t.hi]
    multi = kept & (nops > 2)
    i = np.flatnonzero(multi)
    by_wave = [int((i // (4 * WAVE) == w).sum()) for w in range(NW)]
    m = int(multi.sum())
    return dict(inline=int((kept & (nops <= 2)).sum()), multi=m, queued=min(m, QCAP), walked=max(0, m - QCAP),
                by_wave=by_wave, slots=set((i % 4).tolist()), dropped_multi=int((~kept & (nops > 2)).sum()))


def wave_rank_order(c, t, wave):
    """Read indices (contig-wide) of one wave's reads of three or more ops in the order of their ranks when that wave
    is the only one with any: slot-major, then by lane."""
    r = c.get(t.ctg)
    nops = np.diff(r.cigar_off.astype(np.int64))
    kept = kept_mask(r, c.Q, c.flag_mask)
    out = []
    for u in range(U):
        for lane in range(WAVE):
            i = t.lo + 4 * (wave * WAVE + lane) + u
            if i < t.hi and kept[i] and nops[i] > 2:
                out.append(i)
    return out


def generic_phase_a(c, t):
    """Generic kernel, phase A of one tile: dict(batches, staged, waves) -- waves[w] the list of what wave w's queue
    did per batch: ("queue", qn after), ("drain+queue", qn after) or ("slots", the four per-slot counts)."""
    r = c.get(t.ctg)
    nops = np.diff(r.cigar_off.astype(np.int64))
    kept = kept_mask(r, c.Q, c.flag_mask)
    first = r.cigar[np.minimum(r.cigar_off[:-1].astype(np.int64), max(r.n_ops - 1, 0))].astype(np.int64) if r.n_ops else np.zeros(r.n, np.int64)
    simple = kept & (nops == 1) & ((first & 15) == 0) & ((first >> 4) >= 1) & ((first >> 4) <= 0x0fffffff)
    cx = kept & ~simple
    waves = [[] for _ in range(NW)]
    qn = [0] * NW
    for base in range(0, t.nrd, NT * U):
        for w in range(NW):
            cnt = []
            for u in range(U):
                i = t.lo + base + u * NT + w * WAVE + np.arange(WAVE)
                i = i[i < t.hi]
                cnt.append(int(cx[i].sum()))
            tot = sum(cnt)
            if not tot:
                continue
            drained = qn[w] + tot > WAVE
            if drained:
                qn[w] = 0
            if tot <= WAVE:
                qn[w] += tot
                waves[w].append(("drain+queue" if drained else "queue", qn[w]))
            else:
                waves[w].append(("slots", tuple(cnt)))
    return dict(batches=(t.nrd + NT * U - 1) // (NT * U), staged=t.nst <= GEN_CQ, waves=waves, queued=int(cx[t.lo:t.hi].sum()))


@dataclass
class Quarter:
    win0: int
    wleft: int
    sleft: int
    rows: list                      # per row: ("none",) / ("one", rel) / ("several", n boundaries)
    noisy: dict                     # term -> bool: minimum, maximum, carry_low, carry_high, forced
    carry: int

    @property
    def any_noisy(self):
        return any(self.noisy.values())


def quarter(c, t, w, depth):
    """Phase B of wave `w` of the ordinary tile `t` (depth: the contig's per-base vector)."""
    W, step = c.W, min(c.step_used, 0x7fffffff)
    cpos0 = t.t0 + w * CHUNK
    wleft = W - cpos0 % W
    sleft = 0 if cpos0 % step == 0 else step - cpos0 % step
    wleft = FAST_BIG if wleft > FAST_FAR else wleft
    sleft = FAST_BIG if sleft > FAST_FAR else sleft
    chunk0 = w * CHUNK
    nb = FAST_BIG if wleft >= FAST_BIG else chunk0 + wleft
    nf = FAST_BIG if sleft >= FAST_BIG else chunk0 + sleft
    wstep = FAST_BIG if W > FAST_FAR else W
    rows = []
    for r in range(ROWS):
        rb = chunk0 + r * 256
        if nb >= rb + 256:
            rows.append(("none",))
        elif nb + wstep >= rb + 256:
            rows.append(("one", nb - rb))
            nb = min(nb + wstep, FAST_BIG)
        else:
            n = 0
            while nb < rb + 256:
                n += 1
                nb = min(nb + wstep, FAST_BIG)
            rows.append(("several", n))
    d = depth[cpos0:cpos0 + CHUNK]
    carry = int(depth[cpos0 - 1]) if cpos0 > 0 else 0
    lo_thr = max(c.min_cov, 1)
    hi_thr = c.max_mean_depth if c.max_mean_depth > 0 else 0x7fffffff
    noisy = dict(minimum=bool(d.min() < lo_thr), maximum=bool(c.max_mean_depth > 0 and d.max() >= hi_thr),
                 carry_low=carry < lo_thr, carry_high=carry >= hi_thr, forced=nf < chunk0 + CHUNK)
    return Quarter(cpos0 // W, wleft, sleft, rows, noisy, carry)


def quarters(c):
    """(tile, wave, Quarter) of every quarter of every ordinary tile of the job."""
    ref = reference(c.name)
    return [(t, w, quarter(c, t, w, ref[t.ctg][0])) for t in tiles(c) if t.ordinary for w in range(NW)]


def boundaries(c):
    """(total boundaries of the job, boundaries per group of SUPER tiles)."""
    ref = reference(c.name)
    groups = np.zeros((c.n_tiles + SUPER - 1) // SUPER, np.int64)
    tile_beg = 0
    for t, L in enumerate(c.lengths):
        np.add.at(groups, (tile_beg + ref[t][3] // T) // SUPER, 1)
        tile_beg += (L + T - 1) // T
    return int(groups.sum()), groups.tolist()


def capacity_reruns(c):
    """Re-runs because the job has more boundaries than a fresh context's boundary list holds."""
    return int(boundaries(c)[0] > max(CAP_RUNS0, 2 * c.n_tiles))


# ---- building records -----------------------------------------------------------------------------------------------

def plateau(a, b, d, piece=400):
    """d reads deep over [a, b): chains of `M` reads of at most `piece` bases (adjacent intervals cancel at the shared
    edge); the chains are staggered so that no two reads of a level start together."""
    out = []
    for k in range(d):
        x = a
        first = piece - 37 * k % piece if k else piece
        while x < b:
            n = min(first if x == a else piece, b - x)
            out.append((x, "%dM" % n))
            x += n
    return out


def profile(segments, end):
    """Reads whose depth is the step function segments = [(start, depth), ...] up to `end` (levels stacked)."""
    out = []
    top = max(d for _, d in segments)
    for level in range(1, top + 1):
        a = None
        for (s, d), nxt in zip(segments, segments[1:] + [(end, 0)]):
            if d >= level and a is None:
                a = s
            if a is not None and (nxt[1] < level or nxt[0] == end):
                stop = nxt[0]
                out += plateau(a, stop, 1, piece=400 - 31 * level)
                a = None
    return out


def ramp(a, b, every=8, base=40, mod=13, mul=9):
    """Staggered `M` reads over [a, b): the depth wanders, no two neighbouring positions share a running sum."""
    return [(p, "%dM" % (base + (i % mod) * mul)) for i, p in enumerate(range(a, b, every))]


def dips(positions, arm=30):
    """One read `<arm>M1D<arm>M` per position: its deletion is that position (a single-position dip of the depth)."""
    return [(p - arm, "%dM1D%dM" % (arm, arm)) for p in positions if p - arm >= 0]


def background(L, skip=()):
    """Ordinary short-read shaped filler over a contig, outside the (a, b) ranges of `skip`."""
    out = []
    for i, p in enumerate(range(0, L - 160, 23)):
        if any(a - 200 <= p < b for a, b in skip):
            continue
        out.append((p, ("150M", "20S130M", "100M50S", "70M2D78M", "150M")[i % 5]))
    return out


# ---- the cases: prep / classification ---------------------------------------------------------------------------------

def _exact(name, edge, n_before_mod4, n_in, ops_extra=0, lookback_reads=0, n_two=0, **kw):
    """Five tiles; tile 2's read range is crafted: `lookback_reads` reads in the 128 positions before it (the look-back), `n_in` reads
    inside it, and the reads before the look-back start number n_before_mod4 modulo 4 (what rounding lo down adds).
    n_two of the inside reads have two ops, ops_extra more ops go to one `M`-`I` chain read."""
    L, t0 = 5 * T, 2 * T
    items = []
    n_before = 400 + n_before_mod4                                   # in tiles 0 and 1, away from the look-back
    items += [(100 + 15 * i, "120M") for i in range(n_before)]
    assert 100 + 15 * n_before < t0 - 128 - 200
    items += [(t0 - 128 + (i % 128), "50M") for i in range(lookback_reads)]
    for i in range(n_in):
        p = t0 + (i * (T - 200)) // max(n_in, 1)
        items.append((p, "60M20S" if i < n_two else "80M"))
    if ops_extra:
        items.append((t0 + T - 150, "".join("%d%s" % (2, "MI"[k % 2]) for k in range(ops_extra))))
    items += [(3 * T + 200 + 40 * i, "100M") for i in range(90)]     # tile 3 and 4: ordinary neighbours
    return Case(name, edge, [L], {0: reads_of(items)}, hint=128, family="prep", mark=dict(ctg=0, t0=t0), **kw)


def prep_cases():
    out = [
        _exact("prep-1024", "a full tile with exactly 1024 candidate reads: ordinary", 0, 1000, lookback_reads=24),
        _exact("prep-1025", "a full tile with exactly 1025 candidate reads: slow", 0, 1001, lookback_reads=24),
        _exact("prep-round-1023+1", "1023 reads from the look-back start, rounding adds 1: ordinary", 1, 1003, lookback_reads=20),
        _exact("prep-round-1022+2", "1022 reads from the look-back start, rounding adds 2: ordinary", 2, 1002, lookback_reads=20),
        _exact("prep-round-1024+1", "1024 reads from the look-back start, rounding adds 1: slow", 1, 1004, lookback_reads=20),
        _exact("prep-round-1022+3", "1022 reads from the look-back start, rounding adds 3: slow", 3, 1002, lookback_reads=20),
        _exact("prep-ops-1280", "exactly 1280 ops in [clo, chi): ordinary", 0, 900, lookback_reads=20, n_two=300, ops_extra=60),
        _exact("prep-ops-1281", "exactly 1281 ops in [clo, chi): slow", 0, 900, lookback_reads=20, n_two=300, ops_extra=61),
        _exact("prep-both", "1024 reads and 1280 ops at once: ordinary", 0, 1003, lookback_reads=20, n_two=200, ops_extra=57),
    ]
    # a tile nobody reaches next to a dense one; a tile whose only candidates are filtered; reads of zero ops
    L = 6 * T
    items = [(T + 3 * i, "90M") for i in range(1300)]                # tile 1 dense (slow), tile 2 .. 3 empty
    items += [(3 * T + 500 + 7 * i, "100M", (0x4, 0x100, 0x200, 0x400, 0)[i % 5], 0 if i % 5 == 4 else 60) for i in range(300)]
    items += [(4 * T + 9 * i, ("", "50M", "", "10M5D10M")[i % 4]) for i in range(400)]
    items += [(5 * T + 11 * i, "75M") for i in range(300)]
    out.append(Case("prep-empty-filtered-zero-ops", "a tile without candidates, one whose candidates are all filtered, reads of zero ops",
                    [L], {0: reads_of(items)}, hint=128, family="prep", mark=dict(empty=2 * T, filtered=3 * T, zero=4 * T)))
    for n_extra, name in ((0, "prep-contigs-9"), (8, "prep-contigs-17")):
        lens = [T - 1, T, T + 1, 1, 0, 700, T] + [T] * n_extra + [T + 5]
        reads = {t: reads_of(background(Lc) + ([(Lc - 1, "30M")] if Lc > 1 else [(0, "1M")])) for t, Lc in enumerate(lens)
                 if t not in (4, 5)}
        out.append(Case(name, "contig lengths T - 1, T, T + 1, 1, an empty contig (length 0) and one without reads: exactly the "
                        "clipped tiles are slow; %d tiles leave workgroups past the last one" % (9 + n_extra), lens, reads,
                        family="prep"))
    # the position index: `from` not a multiple of 64, a clipped tile whose end is not one, buckets past the last read
    L = 3 * T + 1000 + 37
    items = background(2 * T + 300) + [(T - 100 + i, "90M") for i in range(0, 100, 3)]
    out.append(Case("prep-index-edges", "look-back start not a multiple of 64, tend & 63 != 0 on the clipped tile, the index's "
                    "buckets k and k + 1 past the last read's", [L], {0: reads_of(items)}, hint=200, family="prep", mark=dict(t0=T)))
    return out


STEP_BACKS = (63, 64, 65, 1100, 1400)


def noindex_cases():
    """OPT_INGEST_INDEX = 0: gd_prep_kernel searches `pos` itself (lower_bound_hint, the look-back step-back, `have`).
    One job of six contigs, laid out so that the lanes 63 of the prep waves (tiles 63, 127, 191, 255) fall where a
    search of the tile's END has to miss; prep_searches() and step_back_probes() say what each search does."""
    def piled(first):
        """66 tiles, more than 2 * 8192 reads piled into one tenth and one read into the tenth at the other end."""
        L, n = 66 * T, 2 * 8192 + 700
        a = 0 if first else L - L // 10
        items = [(L - 300 if first else 100, "100M")]
        items += [(a + (i * (L // 10 - 200)) // n, "50M") for i in range(n)]
        return L, reads_of(items)
    # contig 0: look-back starts 63, 64, 65, 1100 and 1400 reads before the tile's first read
    it0 = []
    for k, back in enumerate(STEP_BACKS):
        t0 = (k + 1) * T
        it0 += [(t0 - 128 + (i * 128) // back, "40M") for i in range(back)]
        it0 += [(t0 + 20 * i, "60M") for i in range(100)]
    L0 = (len(STEP_BACKS) + 2) * T
    # contig 1: sparse filler that puts tile 63 of the job on tile 1 of contig 2
    L1 = 55 * T
    it1 = [(p, "90M") for p in range(0, L1 - 100, 211)]
    # contig 2: one read in tile 0, 9000 in tile 1 (lane 63: its end lies 8729 reads past the guess), one near the end
    L2 = 66 * T
    it2 = [(50, "80M")] + [(T + (i * (T - 100)) // 9000, "50M") for i in range(9000)] + [(L2 - 500, "80M")]
    # contig 3: no reads, 23 tiles: lane 63 of the third wave is tile 40 of contig 4, before its pile
    L4, r4 = piled(first=False)
    L5, r5 = piled(first=True)
    return [Case("noindex-search", "no index: the guessed start of a tile misses by more than 8192 reads to the left (reads piled "
                 "into the last tenth) and to the right (into the first tenth), so does the guessed end in lane 63; the look-back "
                 "start lies 63, 64, 65, 1100 and 1400 reads before s0; five prep waves, contigs' last tiles next to others' first",
                 [L0, L1, L2, 23 * T, L4, L5], {0: reads_of(it0), 1: reads_of(it1), 2: reads_of(it2), 4: r4, 5: r5},
                 hint=192, index=False, W=1000, family="noindex")]


HINT_R = 8192


def hint_branch(a, key, guess):
    """Which way lower_bound_hint goes: "left" (the answer lies at or before the probe 8192 below the guess), "right"
    (past the probe 8192 above it), "bracket" (between the probes); "start" / "end" when that probe is the array's
    first / last element, "empty" without elements."""
    n = len(a)
    if n == 0:
        return "empty"
    g = min(guess, n - 1)
    pl = g - HINT_R if g > HINT_R else 0
    ph = g + HINT_R if n - 1 - g > HINT_R else n - 1
    if a[pl] >= key:
        return "left" if pl else "start"
    if a[ph] >= key:
        return "bracket"
    return "right" if ph < n - 1 else "end"


def prep_searches(c):
    """[(which, ctg, t0, branch, answer - guess)] of every lower_bound_hint call of gd_prep_kernel without the index:
    "s0" for every tile but a contig's first; "hi" where the next lane does not have the answer -- lane 63 of a prep wave,
    the job's and a contig's last tile."""
    out = []
    tl = tiles(c)
    for gid, t in enumerate(tl):
        pos = c.get(t.ctg).pos.astype(np.int64)
        n, L = len(pos), c.lengths[t.ctg]
        s0 = 0
        if t.t0:
            s0 = int(np.searchsorted(pos, t.t0))
            out.append(("s0", t.ctg, t.t0, hint_branch(pos, t.t0, t.t0 * n // L), s0 - t.t0 * n // L))
        have = gid % WAVE != WAVE - 1 and gid + 1 < len(tl) and tl[gid + 1].ctg == t.ctg and t.t0 + T == t.tend
        if not have:
            g1 = t.tend * n // L
            guess = g1 - s0 if g1 > s0 else 0
            out.append(("hi", t.ctg, t.t0, hint_branch(pos[s0:], t.tend, guess), t.hi - s0 - guess))
    return out


def step_back_probes(c, t):
    """Probes of the look-back step-back (64, 256, 1024, 4096 ... reads before s0) until one lies before `from`."""
    pos = c.get(t.ctg).pos.astype(np.int64)
    frm = t.t0 - lookback_of(c)[0] if t.t0 > lookback_of(c)[0] else 0
    hi2, step, probes = int(np.searchsorted(pos, t.t0)), 64, 0
    if frm == 0:
        return 0
    while hi2 > 0:
        p = max(hi2 - step, 0)
        probes += 1
        if pos[p] < frm:
            break
        hi2, step = p, step * 4
    return probes


# ---- the cases: straight-line kernel, phase A ---------------------------------------------------------------------------

PAIR_LENS = ((0, 37), (1, 37), (37, 1), (37, 0), (37, 41))


def phase_a_cases():
    out = []
    # every ordered pair of op codes 0 .. 8, every single op code, one pair each of the codes 9 .. 15
    L, t0 = 5 * T, 2 * T
    items, k = [], 0
    for a in range(9):
        for b in range(9):
            for la, lb in PAIR_LENS:
                items.append((t0 + 7 + (k * 9) % (T - 100), [(la, a), (lb, b)]))
                k += 1
    for a in range(9):
        for l in (0, 1, 53):
            items.append((t0 + 11 + (k * 9) % (T - 100), [(l, a)]))
            k += 1
    for a in range(9, 16):
        items.append((t0 + 13 + (k * 9) % (T - 100), [(25, a), (40, (a + 1 - 9) % 7 + 9)]))
        items.append((t0 + 17 + (k * 9) % (T - 100), [(25, a), (40, 0)]))
        k += 1
    for a in (2, 3):                                                 # a leading D / N from the tile before and two tiles before
        for b in range(9):
            items.append((t0 - 300 - 9 * b, [(400 + b, a), (50, b)]))
            items.append((t0 - T - 300 - 9 * b, [(T + 400 + b, a), (50, b)]))
            items.append((t0 - T - 500 - 9 * b, [(50, b), (T + 600 + b, a)]))
    out.append(Case("a-pairs", "every one- and two-op CIGAR of the codes 0 - 8 (lengths 0, 1, more), pairs of 9 - 15, starts "
                    "inside the tile, in the tile before and two tiles before: all inline", [L], {0: reads_of(items)},
                    hint=8704, W=64, family="phase-a", mark=dict(t0=t0)))
    # interval ends and starts on the tile's edges
    L, t0 = 4 * T, T
    # (the contig's first read has three ops, reaches the tile and is its first staged op: the look-back reaches position 0)
    items = [(0, "%dM2I20M" % (T + 104))] + background(L, skip=[(t0 - 400, t0 + 300), (t0 + T - 400, t0 + T + 300)])
    items += [(t0 - 200, "%dN5M" % (200 + T - 1)), (t0 - 201, "%dN5M" % (201 + T)),       # start carried to t0 + T - 1, t0 + T
              (t0 - 100, "99M"), (t0 - 100, "100M"), (t0 - 100, "101M"), (t0 - 1, "1M"), (t0 - 1, "3M"),
              (t0 + T - 90, "89M"), (t0 + T - 90, "90M"), (t0 + T - 90, "91M"),
              (0, "33M"), (0, "1M"), (L - 1, "1M"), (L - 1, "50M"), (L - 40, "90M"), (L - 40, "20M5D60M")]
    out.append(Case("a-edges", "a leading N that carries the start to t0 + T - 1 and to t0 + T; reads ending at t0 - 1, t0, "
                    "t0 + 1, t0 + T - 1, t0 + T, t0 + T + 1; pos = t0 - 1, 0, L - 1; a read past the end of a full last tile",
                    [L], {0: reads_of(items)}, family="phase-a", mark=dict(t0=t0)))
    # 119, 120, 121 and 200 kept reads of three or more ops in one tile
    for n in (119, 120, 121, 200):
        L, t0 = 3 * T, T
        items = [(10 + 30 * i, "100M") for i in range(120)] + [(2 * T + 30 * i, "100M") for i in range(120)]
        tile_items, m = [], 0
        # evenly over the 960 reads -- every wave -- and, where the stride is a multiple of four, staggered over the slots
        picks = {k * 960 // (n - 1) + (k % 4 if 960 // (n - 1) >= 8 else 0) for k in range(n - 1)}
        assert len(picks) == n - 1 and max(picks) < 960
        for i in range(1024 - 64):                                   # four reads per lane, 240 lanes: all four waves
            p = t0 + 10 + 4 * i
            want = i in picks
            if want:
                tile_items.append((p, "20M%d%s30M" % (1 + i % 3, "IDN"[i % 3])))
                m += 1
            elif i % 47 == 3:
                tile_items.append((p, "25M3I25M", 0x400))            # a filtered multi-op read between them
            else:                                                    # inline reads and reads without ops (no share of the 1280)
                tile_items.append((p, ("", "70M", "", "10S60M", "", "50M2D")[i % 6]))
        # the longest span of the job belongs to the tile's last multi-op read
        tile_items.append((t0 + T - 200, "40M300N40M2I8M"))
        m += 1
        assert m == n, (m, n)
        out.append(Case("a-queue-%d" % n, "%d kept reads of three or more ops in one ordinary tile (the queue holds 120)" % n,
                        [L], {0: reads_of(items + tile_items)}, hint=512, family="phase-a", mark=dict(t0=t0, n=n)))
    # one wave holds all 124 multi-op reads: the ranks are known, the longest span belongs to a read walked in place
    L, t0 = 3 * T, T
    items = [(10 + 30 * i, "100M") for i in range(100)] + [(2 * T + 30 * i, "100M") for i in range(120)]
    tile_items = []
    for i in range(600):
        lane, u = i // 4, i % 4
        multi = lane <= 30
        cg = "20M2D20M1I5M" if multi else "66M"
        if lane == 30 and u == 3:
            cg = "30M540N30M1I9M"                                    # rank 123: walked in place; span 609 > the hint
        tile_items.append((t0 + 5 * i, cg))
    out.append(Case("a-walked-span", "124 multi-op reads in wave 0: ranks 120 - 123 are walked in place, the last of them has "
                    "the job's longest span (one look-back re-run)", [L], {0: reads_of(items + tile_items)}, hint=512,
                    family="lookback", mark=dict(t0=t0)))
    # 1024 reads over one position
    L, t0 = 3 * T, T
    items = [(t0 + 1000 + i, "%dM" % (1100 - i)) for i in range(1024)]
    out.append(Case("a-depth-1024", "1024 reads cover one position: the deepest an ordinary tile gets; one window sum takes "
                    "the whole tile", [L], {0: reads_of(items + background(2700)[:108] + [(2 * T + 400 + 9 * i, "80M") for i in range(300)])},
                    W=4096, hint=1152, family="phase-a", mark=dict(t0=t0)))
    return out


# ---- the cases: look-back ---------------------------------------------------------------------------------------------

def lookback_cases():
    out = []
    t0 = 2 * T
    def mk(name, edge, extra, hint=512):
        items = background(4 * T, skip=[(t0 - 700, t0 + 200)]) + extra
        return Case(name, edge, [4 * T], {0: reads_of(items)}, hint=hint, family="lookback", mark=dict(t0=t0))
    out.append(mk("lb-exact-500", "a look-back that is no multiple of 64 (500) and a kept read spanning exactly it: no re-run, the "
                  "look-back stays 500", [(t0 - 500, "500M")], hint=500))
    tight = mk("lb-tighten", "no hint, no index: the first compute looks back the default 512, finds spans of at most 150 and "
               "leaves a look-back of 192 to the second", [], hint=0)
    tight.index = False
    out.append(tight)
    out.append(mk("lb-exact", "a kept read at t0 - lookback spanning exactly the look-back: no re-run", [(t0 - 512, "512M")]))
    out.append(mk("lb-over", "a kept read at t0 - lookback - 1 spanning lookback + 1: one re-run, look-back 576",
                  [(t0 - 513, "513M")]))
    out.append(mk("lb-filtered-flag", "the long read filtered by its flag: no re-run, not counted", [(t0 - 513, "513M", 0x400)]))
    out.append(mk("lb-filtered-mapq", "the long read filtered by its MAPQ: no re-run, not counted", [(t0 - 513, "513M", 0, 0)]))
    out.append(mk("lb-queued", "the long span comes from a three-op read (queued): one re-run", [(t0 - 513, "200M113N200M")]))
    return out


# ---- the cases: phase B, windows ---------------------------------------------------------------------------------------

WINDOW_SIZES = (1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 100, 200, 255, 256, 257, 1000, 1023, 1024, 1025, 1279, 4095, 4096, 4097,
                5000, FAST_FAR + 40000, 2 ** 31 - 1)


def window_case(W):
    """Two contigs (8 tiles and 17 positions; 3 tiles) under a ramp of staggered reads, with single-position dips just
    before and just after window boundaries."""
    lens = [8 * T + 17, 3 * T]
    reads = {}
    for t, L in enumerate(lens):
        items = ramp(0, L - 200)
        if W < L:
            bounds = list(range(W, L, W))
            pick = bounds[:: max(1, len(bounds) // 12)][:14]
            items += dips([b - 1 for b in pick[0::2]] + [b for b in pick[1::2]])
        marks = [T - 1, 2 * T, 2 * T + 1023, T + 1024]             # a tile's last and first, a quarter's last and first position
        items += dips(marks) + dips(marks, 33) + dips(marks, 41) + dips(marks, 52)
        reads[t] = reads_of(items)
    return Case("w-%d" % W, "window size %d: boundaries inside rows, on row, quarter and tile starts" % W, lens, reads, W=W,
                family="windows", mark=dict(dips=marks))


# ---- the cases: phase B, classes ---------------------------------------------------------------------------------------

def class_segments():
    """A depth step function over six tiles, CALLABLE (5) by default, with a class change on each structural position."""
    q = CHUNK
    seg = [(0, 5),
           (T - 10, 3), (T, 5),                              # a tile's first position: the carry at LDS index -1 decides
           (T + q - 5, 3), (T + q, 5),                       # a quarter's first position, the whole quarter CALLABLE after it
           (T + 2 * q + 256 - 7, 0), (T + 2 * q + 256, 4),   # a row's first position (carry_before)
           (T + 2 * q + 512 + 40, 6), (T + 2 * q + 512 + 44, 5),       # a lane's first position (wave_prev_lane), both ways
           (T + 2 * q + 512 + 81, 3), (T + 2 * q + 512 + 86, 6), (T + 2 * q + 512 + 91, 3), (T + 2 * q + 512 + 99, 5),   # positions 1, 2, 3 of a lane
           (2 * T - 1, 3), (2 * T + 9, 5),                   # the last position of a tile
           (2 * T + q - 30, 0), (2 * T + q, 5), (2 * T + 2 * q, 3), (2 * T + 2 * q + 50, 5),  # a CALLABLE quarter between two others
           (3 * T + 100, 6), (3 * T + 1500, 5),              # max_mean_depth and max_mean_depth - 1
           (4 * T + 700, 0), (4 * T + 900, 5), (4 * T + 2 * q + 5, 3), (4 * T + 2 * q + 9, 5),  # a CALLABLE quarter (carry included) between two others
           (5 * T + 2000, 4), (5 * T + 2100, 5)]
    return seg, 6 * T


def class_case(name, edge, **kw):
    seg, L = class_segments()
    return Case(name, edge, [L, 2 * T + 100], {0: reads_of(profile(seg, L)), 1: reads_of(profile([(0, 5), (T + 100, 3)], 2 * T + 100))},
                family="classes", mark=dict(seg=seg), **kw)


def class_cases():
    out = [class_case("cls-4-0", "class changes on position 0, a tile's, a quarter's, a row's, a lane's first position, positions "
                      "1 - 3 of a lane, a tile's last position; min_cov 4, no maximum", min_cov=4, max_mean_depth=0),
           class_case("cls-4-6", "the same with max_mean_depth 6: depths 5 and 6", min_cov=4, max_mean_depth=6),
           class_case("cls-4-4", "min_cov 4, max_mean_depth 4: nothing is CALLABLE", min_cov=4, max_mean_depth=4)]
    # (gd_set_params: the step is a multiple of the window size)
    for step, W in ((100, 100), (256, 64), (1024, 256), (4096, 1024), (3, 3), (FAST_FAR + 40000, FAST_FAR + 40000)):
        out.append(class_case("cls-step-%d" % step, "forced breaks every %d positions" % step, min_cov=4, max_mean_depth=6, step=step, W=W))
    out.append(class_case("cls-step-W", "step = W = 1000", min_cov=4, max_mean_depth=6, step=1000, W=1000))
    return out


# ---- the cases: phase C, the ordering kernel, the read-back --------------------------------------------------------------

def _fill_to(name, edge, target, **kw):
    """Contig 0 with class changes; contig 1 without reads, its length chosen so that the job has `target` boundaries
    (step 16: one forced break every 16 positions)."""
    seg, L = class_segments()
    r0 = reads_of(profile(seg, L))
    at, _ = ref_boundaries(ref_depth(r0, 1, 0x704, L), 4, 6, 16)
    need = target - len(at)
    assert need > 0
    return Case(name, edge, [L, 16 * need - 5], {0: r0}, min_cov=4, max_mean_depth=6, step=16, W=16, family="phase-c",
                mark=dict(target=target), **kw)


def phase_c_cases():
    out = [_fill_to("c-bounds-%d" % n, "exactly %d run boundaries in the job (the read-back kernel carries 4096)" % n, n)
           for n in (SPEC - 1, SPEC, SPEC + 1)]
    L = 17 * T
    out.append(Case("c-cap-grow", "more boundaries than a fresh context's list holds: one capacity re-run; step 1 over "
                    "constant depth: every position of ordinary tiles is a forced break", [L], {0: reads_of(plateau(0, L, 5))},
                    step=1, W=1, fresh=True, family="phase-c"))
    items = [(T + 2 * i, "1M") for i in range(2048)] + background(T - 200) + [(2 * T + 300 + 20 * i, "100M") for i in range(150)]
    out.append(Case("c-alternating", "depth 0 / 1 / 0 / 1 over a whole tile: a boundary on all 4096 positions (2048 reads: a "
                    "slow tile)", [3 * T], {0: reads_of(items)}, min_cov=1, family="phase-c", mark=dict(t0=T)))
    # 1030 tiles: tile 1023 is the last of group 0, tile 1024 the first of group 1
    L0 = 1025 * T
    items = profile([(1023 * T - 600, 5), (1023 * T + 100, 3), (1023 * T + 2000, 6), (1024 * T - 1, 2), (1024 * T, 5),
                     (1024 * T + 7, 0), (1024 * T + 300, 4), (1024 * T + 3000, 0)], 1024 * T + 3500)
    items += [(5 * T + 100, "150M"), (500 * T - 20, "100M")]
    seg, L2 = class_segments()
    out.append(Case("c-super-1030", "1030 tiles, two ordering groups: boundaries in the last tile of group 0 and the first of "
                    "group 1; a contig without class changes between two with", [L0, T, L2 - 2 * T],
                    {0: reads_of(items), 2: reads_of(profile(seg[:19], L2 - 2 * T))}, W=4096, min_cov=4, max_mean_depth=6,
                    family="phase-c-large"))
    return out


# ---- the cases: generic / slow kernel -----------------------------------------------------------------------------------

MULTI = "20M3I20M2D10M"
NOT_M = ("70=", "70X", "70D", "70S", "0M")


def _generic(name, edge, tile_cigars, **kw):
    """Three tiles; tile 1 holds exactly the given reads (evenly spread), nothing reaches it from tile 0."""
    n = len(tile_cigars)
    items = [(10 + 30 * i, "100M") for i in range(120)]              # 120 reads (a multiple of 4) far from the look-back
    items += [(T + (i * (T - 120)) // n, cg) for i, cg in enumerate(tile_cigars)]
    items += [(2 * T + 200 + 30 * i, "100M") for i in range(100)]
    return Case(name, edge, [3 * T], {0: reads_of(items)}, hint=128, family="generic", mark=dict(t0=T), **kw)


def generic_cases():
    out = []
    for n in (1023, 1024, 1025, 2048, 2049):
        out.append(_generic("g-reads-%d" % n, "%d candidate reads in a tile: batches of 1024" % n,
                            [MULTI if i % 8 == 2 else "90M" for i in range(n)]))
    for nst in (GEN_CQ, GEN_CQ + 1):
        cigars = ["80M"] * 1100
        cigars[500] = "".join("2%s" % "MI"[k % 2] for k in range(nst - 1099))
        out.append(_generic("g-ops-%d" % nst, "%d ops in the tile's read range (1536 are staged)" % nst, cigars))
    def owned(wave0_multi_slots):
        """1100 reads; read base + tid + u * NT belongs to thread tid: wave 0 owns tid 0 - 63."""
        cigars = ["80M"] * 1100
        for u, lanes in wave0_multi_slots:
            for l in lanes:
                cigars[u * NT + l] = MULTI
        return cigars
    out.append(_generic("g-wave-64", "64 multi-op reads of one batch owned by one wave: the queue exactly full", owned([(0, range(64))])))
    out.append(_generic("g-wave-65", "65 multi-op reads of one batch owned by one wave: slot by slot", owned([(0, range(64)), (1, [5])])))
    out.append(_generic("g-wave-256", "256 multi-op reads of one batch owned by one wave: slot by slot, every slot full",
                        owned([(u, range(64)) for u in range(4)])))
    for extra, total in ((0, 64), (1, 65)):
        cigars = ["80M"] * 1200
        for l in range(32):
            cigars[l] = MULTI
        for l in range(32 + extra):
            cigars[1024 + l] = MULTI
        out.append(_generic("g-cross-%d" % total, "qn + tot = %d across two batches of one wave" % total, cigars))
    out.append(_generic("g-not-m", "one-op reads that are not M (=, X, D, S, 0M): queued on the generic kernel, inline on the "
                        "straight-line one", [NOT_M[i % 5] if i % 3 else "75M" for i in range(600)]))
    return out


def _all_cases():
    out = prep_cases() + noindex_cases() + phase_a_cases() + lookback_cases() + [window_case(W) for W in WINDOW_SIZES]
    out += class_cases() + phase_c_cases() + generic_cases()
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return out


FAMILIES = ("prep", "noindex", "phase-a", "lookback", "windows", "classes", "phase-c", "phase-c-large", "generic")
_BUILT = {}


def case(name):
    if not _BUILT:
        _BUILT.update((c.name, c) for c in _all_cases())
    return _BUILT[name]


def names(family=None):
    case("w-1")
    return [n for n, c in _BUILT.items() if family is None or c.family == family]
