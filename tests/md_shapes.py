"""Shapes for the ten multidepth kernels of goleft_amd/csrc/gd_multidepth.hpp (and the scan helpers of gd_index.hpp they
reach through launch_scan) at their structural edges, with the two things a test needs to trust them: a CPU model of
the device's SET FORM of the block finder, and deliberately wrong variants of it (mutants) that show a case would
notice the off-by-one it is named for.

Test infrastructure only, no pytest marks: tests/test_md_shapes.py (CPU) shows that the model equals the oracle's
sequential restatement (oracle/pyoracle.py::multidepth_py) on every case, that every case kills the mutants it names
and reaches the figure it is named for; tests/test_gpu_md_shapes.py runs every case on the device.

The model is written from the comment block of gd_multidepth.hpp (`The block finder`), in the kernels' terms -- not by
translating multidepth_py.  With A = `any` (printed sites), S = `suf` (sufficient sites), N = A & ~S:
  * run starts / ends of the WHOLE contig: an S site with no S site in the max_skip + 1 positions before / after it;
    their positions are compacted in order through exclusive scans of per-word popcounts (prs, pre; ps for S itself);
  * per chunk c (i = c * chunk): z0 = first N site >= i; E = first N site p >= i + chunk + 2 with no S site in
    [max(z0, p - max_skip + 1), p), else the contig end; pa = last printed site in [z0, E); the chunk's runs are
    k_lo = #(run ends < z0) .. #(run starts < E);
  * per (chunk, run) pair: the run clipped to [z0, E), its S count from ps, flushed unless it is the chunk's last pair
    and pa < e + max_skip + 2; a flushed run of fewer than min_size sites is dropped; splitBlocks cuts the rest
    greedily, a block ending with the last S site less than `window` after its first (window <= 1: every site alone);
  * the blocks of all pairs are laid out through an exclusive scan of their counts (nblk).
Every case keeps S a subset of A: the reference only ever sees printed sites, so what the device answers for a
sufficient but unprinted site is not defined by it (include/goleft_depth.h, gd_md_load_flags).

The model's constants are restated here; kernel_constants() reads the sources' and tests/test_md_shapes.py holds the
two against each other.
"""
import os
import re
from bisect import bisect_left, bisect_right
from dataclasses import dataclass, field
from functools import lru_cache

import numpy as np

from oracle import pyoracle as po
from tests import helpers as H

THREADS, SCAN_BLOCK, SCAN_SWITCH, SCAN_THREADS, MAX_CHUNKS = 256, 4096, 4 * 4096, 1024, 1 << 20
BIG = 10 ** 7                      # a chunk or window no case reaches

SCAN_ARRAYS = ("ps", "prs", "pre", "nblk")
MUTANTS = {
    "no_word_crossing": "the run look-back and look-ahead stop at the word of p",
    "gap_ge": "a run breaks at gap >= max_skip instead of >",
    "gap_gt1": "a run breaks only at gap > max_skip + 1",
    "past_chunk_off": "the stream may end from i + chunk + 1",
    "past_chunk_late": "the stream may end only from i + chunk + 3",
    "end_lookback_off": "the end test looks back max_skip positions instead of max_skip - 1",
    "end_lookback_short": "the end test looks back max_skip - 2 positions",
    "no_z0_clamp": "an S site before z0 keeps the stream alive",
    "z0_from_i1": "z0 is searched from i + 1",
    "z0_from_im1": "z0 is searched from i - 1",
    "flush_off": "flushed when pa >= e + max_skip + 1",
    "flush_late": "flushed only when pa >= e + max_skip + 3",
    "E_flushes": "the site E itself counts as a flushing site",
    "always_flushed": "the last run of a stream is held to min_size like the others",
    "minsize_unclipped": "min_size is applied to the unclipped run",
    "minsize_gt": "a flushed run needs more than min_size sites",
    "window_le": "a block takes the site exactly `window` after its first",
    "window0_whole": "window 0 leaves a run in one block",
    "window_no_word_crossing": "the look-back from a block's window limit stops at the limit's word",
    "window_i32": "b0 + window - 1 is formed in 32 bits",
    "chunks_256": "chunks with index >= 256 get no stream",
    "tail_bits": "positions >= L in the last word are treated as present",
    "last_of_chunk": "`last run of the stream` is taken as the last run of the contig",
    "per_floor": "the single-workgroup scan gives a thread max(n // 1024, 1) elements, not the ceiling",
}
MUTANTS.update({"scan_block0:" + a: "three-launch scan of %s: elements of 4096-blocks >= 1 lose their block offset" % a
                for a in SCAN_ARRAYS})


def kernel_constants():
    """The constants the model restates, read from the text of the three sources."""
    def text(*rel):
        with open(os.path.join(H.ROOT, "goleft_amd", "csrc", *rel)) as f:
            return f.read()
    md, ix, st, aux = text("gd_multidepth.hpp"), text("gd_index.hpp"), text("gd_api_state.hpp"), text("gd_api_aux.inc")
    num = lambda pattern, t: int(re.search(pattern, t).group(1))
    word_kernels = ("runs", "compact", "chunks", "count", "blocks")
    return {
        "threads": {k: num(r"__launch_bounds__\((\d+)\) void gd_md_%s_kernel" % k, md) for k in word_kernels},
        "chunk_stride": num(r"c < j\.n_chunks; c \+= (\d+)\)", md),
        "word_stride": num(r"const int64_t k = \(int64_t\)blockIdx\.x \* (\d+) \+ threadIdx\.x;", md),
        "pair_stride": num(r"const uint32_t pair = blockIdx\.x \* (\d+)u \+ threadIdx\.x;", md),
        "scan_block": num(r"constexpr uint32_t SCAN_BLOCK = (\d+);", ix),
        "scan_block_threads": num(r"__launch_bounds__\((\d+)\) void gd_scan_apply_kernel", ix),
        "scan_per_thread": num(r"blockIdx\.x \* SCAN_BLOCK \+ threadIdx\.x \* (\d+)u;", ix),
        "unit_threads": num(r"__launch_bounds__\((\d+)\) void gd_unit_scan_kernel", ix),
        "unit_per": (num(r"const uint32_t per = \(n \+ (\d+)u\) / \d+u;", ix), num(r"const uint32_t per = \(n \+ \d+u\) / (\d+)u;", ix)),
        "scan_switch_blocks": num(r"if \(n <= (\d+)u \* gd::SCAN_BLOCK\)", st),
        "unit_launch": num(r"gd::gd_unit_scan_kernel, dim3\(1\), dim3\((\d+)\), 0, c->stream, v, n\)", st),
        "max_chunks_log2": num(r"n_chunks > \(1 << (\d+)\)", aux),
    }


# ---- the model --------------------------------------------------------------------------------------------------

@dataclass
class Pair:
    chunk: int
    run: int
    last: bool
    s: int                         # the run clipped to the chunk's stream; (-1, -1) when nothing of it is left
    e: int
    count: int
    flushed: bool
    n_blocks: int


@dataclass
class Result:
    blocks: list                   # (start, end) in output order
    nw: int
    n_runs: int
    n_chunks: int
    n_pairs: int
    n_blocks: int
    starts: list = field(default_factory=list)
    ends: list = field(default_factory=list)
    chunks: list = field(default_factory=list)     # dicts z0, E, pa, k_lo, n_pairs
    pairs: list = field(default_factory=list)


def _scan(v, name, mutant):
    """Exclusive scan of v with the total appended, as launch_scan computes it."""
    v = np.asarray(v, np.int64)
    n = len(v)
    out = np.zeros(n + 1, np.int64)
    out[1:] = np.cumsum(v)
    if n <= SCAN_SWITCH:
        if mutant == "per_floor":
            done = min(n, SCAN_THREADS * max(n // SCAN_THREADS, 1))
            out[n] = out[done]                                      # the total of what the threads took
            out[done:n] = v[done:]                                  # never scanned: the counts stay
        return out
    if mutant == "scan_block0:" + name:
        k = np.arange(n)
        out[:n] -= out[(k // SCAN_BLOCK) * SCAN_BLOCK] * (k >= SCAN_BLOCK)
    return out


def _first(lst, lo, lim):
    """first element of the sorted list in [lo, lim), else lim"""
    k = bisect_left(lst, lo)
    return lst[k] if k < len(lst) and lst[k] < lim else lim


def _last(lst, hi, floor):
    """last element of the sorted list in [floor, hi], else -1"""
    k = bisect_right(lst, hi)
    return lst[k - 1] if k and lst[k - 1] >= floor else -1


def model(any_, suf, chunk, max_skip, min_size, window, mutant=None):
    assert mutant is None or mutant in MUTANTS, mutant
    A = np.asarray(any_, bool)
    S = np.asarray(suf, bool)
    L = len(A)
    nw = (L + 31) // 32
    n_chunks = (L + chunk - 1) // chunk
    if mutant == "tail_bits":
        pad = np.ones(32 * nw - L, bool)
        A, S, L = np.concatenate([A, pad]), np.concatenate([S, pad]), 32 * nw
    res = Result([], nw, 0, n_chunks, 0, 0)
    sp = np.flatnonzero(S)
    Sl, Nl, Al = sp.tolist(), np.flatnonzero(A & ~S).tolist(), np.flatnonzero(A).tolist()
    if not len(sp):
        return res
    # B1: run starts and ends, one decision per S site
    back = fwd = max_skip + 1
    if mutant == "gap_ge":
        back = fwd = max_skip
    elif mutant == "gap_gt1":
        back = fwd = max_skip + 2
    lo, hi = sp - back, sp + fwd
    if mutant == "no_word_crossing":
        lo, hi = np.maximum(lo, sp & ~31), np.minimum(hi, sp | 31)
    prev = np.concatenate([[-1 << 40], sp[:-1]])
    nxt = np.concatenate([sp[1:], [1 << 40]])
    rs_pos, re_pos = sp[prev < lo], sp[nxt > hi]
    word_counts = lambda pos: np.bincount(pos >> 5, minlength=nw)
    true_prs, true_pre = _scan(word_counts(rs_pos), "", None), _scan(word_counts(re_pos), "", None)
    ps, prs, pre = (_scan(word_counts(p), name, mutant) for p, name in ((sp, "ps"), (rs_pos, "prs"), (re_pos, "pre")))
    n_runs = int(prs[nw])
    res.n_runs = n_runs
    if n_runs == 0:
        return res
    # B2: compaction in position order
    def compact(pos, scan, true):
        out = np.zeros(n_runs, np.int64)
        w = pos >> 5
        o = scan[w] + (np.arange(len(pos)) - true[w])
        keep = o < n_runs
        out[o[keep]] = pos[keep]
        return out.tolist()
    starts, ends = compact(rs_pos, prs, true_prs), compact(re_pos, pre, true_pre)
    res.starts, res.ends = starts, ends
    rsl, rel = rs_pos.tolist(), re_pos.tolist()

    def rank(lst, scan, p):
        if p >= L:
            return int(scan[nw])
        return int(scan[p >> 5]) + bisect_left(lst, p) - bisect_left(lst, (p >> 5) << 5)

    # B3: the stream of every chunk
    pair_off = [0]
    for c in range(n_chunks):
        i = c * chunk
        z_from = i + 1 if mutant == "z0_from_i1" else i - 1 if mutant == "z0_from_im1" else i
        z0 = _first(Nl, max(z_from, 0), L)
        E, pa, klo, khi = L, -1, 0, 0
        if z0 < L and not (mutant == "chunks_256" and c >= THREADS):
            p = z0
            frm = i + chunk + (1 if mutant == "past_chunk_off" else 3 if mutant == "past_chunk_late" else 2)
            if frm > p:
                p = _first(Nl, frm, L)
            look = max_skip if mutant == "end_lookback_off" else max_skip - 2 if mutant == "end_lookback_short" else max_skip - 1
            while p < L:
                lo_ = p - look
                if lo_ < z0 and mutant != "no_z0_clamp":
                    lo_ = z0
                if _last(Sl, p - 1, max(lo_, 0)) < 0:
                    break
                p = _first(Nl, p + 1, L)
            E = p
            klo, khi = rank(rel, pre, z0), rank(rsl, prs, E)
            pa = _last(Al, E if mutant == "E_flushes" else E - 1, z0)
        n = max(khi - klo, 0) if z0 < L else 0
        if mutant == "chunks_256" and c >= THREADS:
            n = 0
        res.chunks.append({"z0": z0, "E": E, "pa": pa, "k_lo": klo, "n_pairs": n})
        pair_off.append(pair_off[-1] + n)
    n_pairs = pair_off[-1]
    res.n_pairs = n_pairs
    if n_pairs == 0:
        return res
    # B4: the blocks of every (chunk, run) pair
    per_pair = []
    for c, ch in enumerate(res.chunks):
        z0, E = ch["z0"], ch["E"]
        for q in range(ch["n_pairs"]):
            k = ch["k_lo"] + q
            if not 0 <= k < n_runs:                                  # (a mutant's scan can point anywhere)
                per_pair.append([])
                res.pairs.append(Pair(c, k, False, -1, -1, 0, True, 0))
                continue
            last = k == n_runs - 1 if mutant == "last_of_chunk" else q + 1 == ch["n_pairs"]
            s, e = starts[k], ends[k]
            if s < z0:
                s = _first(Sl, z0, e + 1)
            if e >= E:
                e = _last(Sl, E - 1, s)
            if e < 0 or s > e:
                per_pair.append([])
                res.pairs.append(Pair(c, k, last, -1, -1, 0, True, 0))
                continue
            cs, ce = (starts[k], ends[k]) if mutant == "minsize_unclipped" else (s, e)
            count = (rank(Sl, ps, ce + 1) - rank(Sl, ps, cs)) & 0xffffffff
            reach = e + max_skip + (1 if mutant == "flush_off" else 3 if mutant == "flush_late" else 2)
            flushed = not last or ch["pa"] >= reach or mutant == "always_flushed"
            blocks = []
            if not (flushed and (count <= min_size if mutant == "minsize_gt" else count < min_size)):
                b0 = s
                while b0 <= e:
                    if window > 0:
                        lim = b0 + window - (0 if mutant == "window_le" else 1)
                        if mutant == "window_i32":
                            lim = (lim + (1 << 31)) % (1 << 32) - (1 << 31)
                        lim = lim if lim < e else e
                        floor = max(b0, (lim >> 5) << 5) if mutant == "window_no_word_crossing" else b0
                        b1 = _last(Sl, lim, floor) if lim >= floor else -1
                    else:
                        b1 = e if mutant == "window0_whole" else b0
                    if b1 < b0:
                        b1 = b0
                    blocks.append((b0, b1 + 1))
                    b0 = _first(Sl, b1 + 1, e + 1)
            per_pair.append(blocks)
            res.pairs.append(Pair(c, k, last, s, e, count, flushed, len(blocks)))
    # B5: laid out through the scan of the counts
    nblk = _scan([len(b) for b in per_pair], "nblk", mutant)
    n_blocks = int(nblk[n_pairs])
    res.n_blocks = n_blocks
    out = [(0, 0)] * n_blocks
    for q, blocks in enumerate(per_pair):
        if nblk[q + 1] == nblk[q]:
            continue
        for t, b in enumerate(blocks):
            if nblk[q] + t < n_blocks:
                out[int(nblk[q]) + t] = b
    res.blocks = out
    return res


# ---- the cases --------------------------------------------------------------------------------------------------

@dataclass
class Case:
    name: str
    any: np.ndarray
    suf: np.ndarray
    chunk: int
    max_skip: int
    min_size: int
    window: int
    kills: tuple = ()

    @property
    def params(self):
        return self.chunk, self.max_skip, self.min_size, self.window


def sites(L, S=(), N=()):
    """any / suf of length L: S sufficient sites, N printed and insufficient ones."""
    a, s = np.zeros(L, bool), np.zeros(L, bool)
    S, N = np.asarray(list(S), np.int64), np.asarray(list(N), np.int64)
    assert not len(np.intersect1d(S, N))
    s[S] = True
    a[S] = True
    a[N] = True
    return a, s


CASES = {}


def add(name, L, S, N, chunk=BIG, max_skip=2, min_size=1, window=BIG, kills=()):
    assert name not in CASES and all(k in MUTANTS for k in kills), name
    a, s = sites(L, S, N)
    CASES[name] = Case(name, a, s, chunk, max_skip, min_size, window, tuple(kills))


def _word_edges():
    add("word-bit31-bit0-skip0", 100, [31, 32], [0], max_skip=0, kills=("no_word_crossing", "gap_ge"))
    for ms in (1, 31, 32, 33, 70, 100):
        a, c = 32 * 2 + 31, 32 * 20 + 31                             # both first sites at bit 31 of a word
        add("word-straddle-skip%d" % ms, 1100, [a, a + ms + 1, c, c + ms + 2], [0], max_skip=ms,
            kills=("no_word_crossing", "gap_ge", "gap_gt1"))
    for ms in (1, 5):                                                # inside one word: the previous-bit path
        add("word-inside-skip%d" % ms, 200, [35, 35 + ms + 1, 99, 99 + ms + 2], [0], max_skip=ms, kills=("gap_ge", "gap_gt1"))


def _contig_ends():
    add("run-from-0", 50, [0, 1, 3, 4, 30, 31, 32], [2, 20], max_skip=1, min_size=3, kills=("minsize_unclipped",))
    add("last-site-L1", 1, [0], [])
    for L in (31, 32, 33, 64, 65):
        add("last-site-L%d" % L, L, [L - 1], [0], kills=() if L % 32 == 0 else ("tail_bits",))
    add("end-lookahead-cut", 45, [42], [0], max_skip=10, kills=("tail_bits",))
    # the run {10, 11} is flushed by the printed site L - 1 = 11 + max_skip + 2 and is too short
    add("flushing-site-at-L-1", 16, [10, 11], [0, 15], max_skip=2, min_size=3, kills=("tail_bits", "flush_late"))


def _z0():
    add("z0-at-chunk-start", 40, [3, 4, 11, 12, 25], [10], chunk=10, kills=("z0_from_i1",))
    add("z0-in-previous-chunk", 40, [3, 4, 11, 12, 25], [9, 30], chunk=10, kills=("z0_from_im1",))
    add("no-insufficient-site", 70, range(5, 60), [])
    # z0 = 13 > i + chunk + 1 lies inside the run 5 .. 15: chunk 0 has one pair and it yields nothing
    add("z0-past-chunk-inside-run", 40, list(range(5, 13)) + [14, 15], [13], chunk=10, max_skip=2, kills=("no_z0_clamp",))


def _E():
    add("E-at-i+1+chunk", 60, [1, 2, 13, 14], [0, 11, 20], chunk=10, max_skip=2, kills=("past_chunk_off",))
    add("E-at-i+2+chunk", 60, [1, 2, 13, 14], [0, 12, 20], chunk=10, max_skip=2, kills=("past_chunk_late",))
    # the insufficient site 20 is past the chunk; the last S site lies max_skip - 1 / max_skip behind it
    add("E-lookback-continues", 60, [1, 18, 22], [0, 20], chunk=10, max_skip=3, kills=("end_lookback_short",))
    add("E-lookback-ends", 60, [1, 17, 22], [0, 20], chunk=10, max_skip=3, kills=("end_lookback_off",))
    add("E-skip1-ends-at-once", 60, [1, 19, 21], [0, 20], chunk=10, max_skip=1, kills=("end_lookback_off",))
    add("E-skip0-ends-at-once", 60, [1, 19, 21], [0, 20], chunk=10, max_skip=0)
    add("E-site-before-far-z0", 60, [16, 20, 21], [18], chunk=10, max_skip=3, kills=("no_z0_clamp",))


def _flush():
    add("flushed-min-size-exact", 80, [5, 6, 7, 20, 21, 40, 41, 42], [0], max_skip=2, min_size=3, kills=("minsize_gt",))
    add("unflushed-short-last-run", 80, [5, 6, 7, 40], [0], max_skip=2, min_size=3, kills=("always_flushed",))
    add("later-site-at-e+skip+2", 80, [5, 6, 7, 40], [0, 44], max_skip=2, min_size=3, kills=("flush_late",))
    add("later-site-at-e+skip+1", 80, [5, 6, 7, 40], [0, 43], max_skip=2, min_size=3, kills=("flush_off", "always_flushed"))
    # chunk 0 ends at E = 17 = 13 + max_skip + 2: the reference breaks before that site can flush the cache {13};
    # the contig goes on with another run, so the last run of chunk 0 is not the last run of the contig
    add("far-site-is-E", 60, [1, 2, 3, 13, 30, 31, 32], [0, 17], chunk=10, max_skip=2, min_size=3,
        kills=("E_flushes", "last_of_chunk", "always_flushed"))
    add("z0-clips-below-min-size", 60, [3, 4, 5, 7, 8, 30, 31, 32], [6, 20], max_skip=1, min_size=3, kills=("minsize_unclipped",))


def _split():
    add("window-1", 40, [5, 6, 7, 9], [0], window=1, kills=("window_le",))
    add("window-0", 40, [5, 6, 7, 9], [0], window=0, kills=("window0_whole",))
    add("window-exact", 60, [10, 14, 15], [0], max_skip=10, window=5, kills=("window_le",))
    add("window-limit-in-empty-word", 200, [10, 20, 120], [0], max_skip=100, window=100, kills=("window_no_word_crossing",))
    add("window-max", 100, [5, 6, 40], [0], max_skip=50, window=(1 << 31) - 1, kills=("window_i32",))
    add("split-in-three", 40, range(5, 15), [0], window=4, kills=("window_le",))


def _period7(L):
    """the probe a[::7] = 1; a[3::7] = 9: an insufficient site at 0 mod 7, a sufficient one at 3 mod 7"""
    p = np.arange(L)
    return p[p % 7 == 3].tolist(), p[p % 7 == 0].tolist()


def _chunks():
    add("chunks-probe-429", 3000, *_period7(3000), chunk=7, max_skip=1, kills=("chunks_256",))
    for n in (256, 257, 600):
        add("chunks-%d-of-7" % n, 7 * n, *_period7(7 * n), chunk=7, max_skip=1, kills=("chunks_256",) if n > 256 else ())
        # chunk 1: the last chunk that can hold a pair is L - 2 (an insufficient site there, a sufficient one after it)
        S, N = _period7(n)
        S, N = [p for p in S if p < n - 2] + [n - 1], [p for p in N if p < n - 2] + [n - 2]
        add("chunks-%d-of-1" % n, n, S, N, chunk=1, max_skip=1, kills=("chunks_256",) if n > 257 else ())
    # 600 chunks, sites only in 700 .. 900 and 2800 .. 3000 and from 4190 on: empty chunks before, between and after
    S, N = _period7(4200)
    busy = lambda p: 700 <= p < 900 or 2800 <= p < 3000 or p >= 4190
    add("chunks-empty-between", 4200, [p for p in S if busy(p)], [p for p in N if busy(p)], chunk=7, max_skip=1, kills=("chunks_256",))


def _streams_to_the_end():
    k = np.arange(600)
    add("streams-to-contig-end", 6000, (5 + 10 * k).tolist(), (6 + 10 * k).tolist(), chunk=50, max_skip=2,
        kills=("scan_block0:nblk",))


SPARSE_NW = (16384, 16385, 20480, 20481)


def _sparse(nw):
    """max_skip 0, min_size 3.  Every 4096-word block holds, in its first word: bit 0 (the second site of a run that
    began at bit 31 of the word before, flushed by the insufficient site at bit 2 and one site short of min_size), a
    flushed run of 3 sites, a flushed run of 2, a run of 4; in its last word: a run of 4 that ends there and bit 31;
    and a stretch every 97 words in between."""
    S, N = [], []
    for b in range((nw + SCAN_BLOCK - 1) // SCAN_BLOCK):
        first, lastw = SCAN_BLOCK * b, min(SCAN_BLOCK * (b + 1), nw) - 1
        p = 32 * first
        S += [p, p + 4, p + 5, p + 6, p + 10, p + 11, p + 15, p + 16, p + 17, p + 18]
        N += [p + 2, p + 8, p + 13, p + 20]
        if lastw > first:
            q = 32 * lastw
            S += [q + 20, q + 21, q + 22, q + 23, q + 31]
            N += [q + 18, q + 25]
            for w in range(first + 97, lastw, 97):
                S += [32 * w + 3 + t for t in range(1 + w % 9)]
                N += [32 * w + 1, 32 * w + 14]
    kills = tuple("scan_block0:" + a for a in ("ps", "prs", "pre")) if nw > SCAN_SWITCH else ()
    add("sparse-nw-%d" % nw, 32 * nw, S, N, chunk=40000, max_skip=0, min_size=3, kills=kills)


def _unit_scan():
    for nw in (1023, 1024, 1025):
        L = 32 * nw - 7
        q = 32 * (nw - 1)
        add("unit-scan-nw-%d" % nw, L, [3, 4, q + 5, q + 6], [0, q + 1], kills=("per_floor", "tail_bits") if nw > 1024 else ("tail_bits",))


for _build in (_word_edges, _contig_ends, _z0, _E, _flush, _split, _chunks, _streams_to_the_end, _unit_scan):
    _build()
for _nw in SPARSE_NW:
    _sparse(_nw)
NAMES = tuple(CASES)
HOSTLIB_NAMES = ("word-straddle-skip33", "chunks-probe-429", "sparse-nw-16385")


def case(name):
    return CASES[name]


def oracle_blocks_of(any_, suf, chunk, max_skip, min_size, window):
    """(start, end) pairs of multidepth_py over one sample whose depth is 2 at S sites and 1 at the other printed ones."""
    d = np.asarray(any_, np.int64) + np.asarray(suf, np.int64)
    lines = po.multidepth_py("c", [d], mincov=2, maxskip=max_skip, minsize=min_size, window=window, min_samples=0.0,
                             chunk_size=chunk)
    return [tuple(map(int, l.split("\t")[1:3])) for l in lines]


@lru_cache(maxsize=None)
def oracle_blocks(name):
    """The oracle's blocks of a case, computed once (a tuple: do not write to it)."""
    c = case(name)
    assert not (c.suf & ~c.any).any(), "suf must be a subset of any"
    return tuple(oracle_blocks_of(c.any, c.suf, *c.params))


@lru_cache(maxsize=None)
def modelled(name, mutant=None):
    c = case(name)
    return model(c.any, c.suf, *c.params, mutant=mutant)


def first_difference(got, want):
    """None when the two block lists are equal, else (index, got, want) of the first block that differs."""
    got, want = [tuple(map(int, b)) for b in got], [tuple(map(int, b)) for b in want]
    for k in range(max(len(got), len(want))):
        g, w = got[k] if k < len(got) else None, want[k] if k < len(want) else None
        if g != w:
            return k, g, w
    return None


# ---- flags and sums ---------------------------------------------------------------------------------------------

FLAG_S = (4, 7, 8)
FLAG_L = (31, 32, 63, 64, 65, 255, 256, 257)
FLAG_MIN_COV = (0, 1)
FLAG_GROUPS = {7: (1, 3), 8: (1, 3)}


def flag_min_samples(S):
    return (-1, 0, S - 1, S)


def flag_reads(S, L):
    """S streams of short reads over a contig of L positions: the ends covered, a stretch that no stream covers."""
    rng = np.random.default_rng(100 * S + L)
    h0 = L // 3
    h1 = h0 + max(3, L // 8)
    out = []
    for s in range(S):
        pos = np.sort(rng.integers(0, L, size=max(2, L // 12)))
        pos = pos[(pos < h0 - 8) | (pos >= h1)]
        if s == 0 or len(pos) < 2:
            pos = np.concatenate([[0], pos[1:-1], [L - 1]])
        lens = rng.integers(1, 9, size=len(pos))
        off = np.arange(len(pos) + 1, dtype=np.uint32)
        out.append(po.Reads(pos.astype(np.int32), np.zeros(len(pos), np.uint16), np.full(len(pos), 60, np.uint8), off,
                            (lens.astype(np.uint32) << 4)))
    return out


def sums_blocks(L, suf=None):
    """Chosen [start, end) blocks of a contig of L positions with bounds at bits 0, 31 and 32 of a word: within one
    word, over exactly two, over three or more, [0, L), [L, L), [L - 1, L), and (given suf) one with no sufficient
    site when there is one."""
    want = [(0, 1), (0, 31), (0, 32), (1, 31), (31, 32), (32, 33), (32, 64), (33, 63),                # one word
            (31, 33), (0, 64), (31, 64), (32, 65), (63, 65),                                            # two
            (31, 65), (0, 65), (0, 96), (31, 97), (32, 129), (63, 257),                                 # three or more
            (0, L), (L, L), (L - 1, L)]
    out = [b for b in want if b[1] <= L]
    if suf is not None:
        gaps = np.flatnonzero(~np.asarray(suf, bool))
        if len(gaps):
            a = int(gaps[0])
            b = a
            while b < L and not suf[b]:
                b += 1
            out.append((a, b))
    return out


def sums_reference(D, suf, blocks):
    """float64 [n_blocks, S]: acc += float(d) / 1000. over the block's sufficient sites in position order."""
    out = np.zeros((len(blocks), len(D)), np.float64)
    for k, (a, b) in enumerate(blocks):
        for s in range(len(D)):
            acc = 0.0
            for p in range(int(a), int(b)):
                if suf[p]:
                    acc += float(int(D[s][p])) / 1000.
            out[k, s] = acc
    return out
