"""-m gpu: the device depthwed matrix (gd_depthwed_kernel, gd_round4g.hpp compiled by hipcc) against the text chain
of the reference at chosen window sums: means on and next to the 4-digit rounding ties, on the boundaries of every
branch of gd_depthwed_cell, on short last windows whose lengths make decimal ties, and zeros.

The records are built so that each window holds exactly its target sum (tests/helpers.py window_sum_reads), the
matrix has more than 64 samples and a row count that is not a multiple of 64 (both edges of the kernel's 64 x 64
tile), and every way the window sums are made is used: per-base output, windows only, sums only (the streaming
kernel of gd_sums_stream.hpp).  The oracle is "%.4g" of sum / len parsed back and rounded, as goleft depth and
goleft depthwed do through text; Python's %-formatting is correctly rounded, as Go's strconv is."""
import ctypes

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import helpers as H

N_SAMPLES = 100          # two tiles of the kernel's 64 samples, the second one partly filled

# W -> reference contigs as (full windows, length of the short last window; 0: the contig ends on a window boundary).
# The short lengths are the ones that make decimal ties; (0, r) is a contig of one window.  A window length's tie
# sums go to the first W below that has windows of that length.
CASES = {
    37: [(9, 1), (9, 2), (9, 4), (9, 5), (9, 8), (9, 10), (9, 20), (0, 20)],
    100: [(13, 40), (13, 40), (13, 8), (13, 0), (14, 99)],
    250: [(13, 125), (13, 125), (13, 200), (13, 40), (14, 0)],
    500: [(13, 250), (13, 250), (13, 125), (13, 40), (14, 499)],
    1000: [(13, 999), (13, 200), (13, 125), (13, 250), (13, 40), (0, 999)],
    16384: [(13, 2000), (13, 2000), (13, 8), (14, 1000), (13, 0)],
}

# (sum, len) where the double product q * 10^j rounds onto a x.5 tie that the exact product is not on: the
# remainder must be taken from the rounded product (gd_round4g.hpp), a fused multiply-add gets the wrong neighbour
FMA_PAIRS = [(123450, 1000), (649450, 1000), (92845, 100), (465225, 500)]

# means of 10^4 .. 10^5 (gd_round4g_big) on short windows: ties of the 4th digit, 9999.5 -> "1e+04"
BIG_PAIRS = [(12345, 1), (10005, 1), (10015, 1), (99995, 1), (99985, 1), (45678, 1),
             (19999, 2), (24691, 2), (20010, 2), (199990, 2)]


def _slot_lengths(W):
    return {W} | {r for _, r in CASES[W] if r}


def _branch_edges(l):
    """Sums whose mean is one unit of the sum under, on and over 0.1, 1, 10, 100 and 1000."""
    out = []
    for num, den in ((1, 10), (1, 1), (10, 1), (100, 1), (1000, 1)):
        c = num * l // den
        out += [c + d for d in (-1, 0, 1) if c + d >= 0]
    return out


def _wanted(W):
    """len -> the chosen sums this W places in windows of that length."""
    s, l = H.depthwed_tie_grid()
    keep = s < 2000 * l                                         # means below 2000: the record count is the mean
    host = {}
    for w in CASES:                                             # each length's tie sums go to one W
        for x in sorted(_slot_lengths(w)):
            host.setdefault(x, w)
    want = {}
    for x in sorted(_slot_lengths(W)):
        sums = []
        if host[x] == W:
            sums += sorted(set(s[keep & (l == x)].tolist()))
        sums += [a for a, b in FMA_PAIRS + BIG_PAIRS if b == x]
        sums += _branch_edges(x) + [0, 0]
        want[x] = sums
    return want


def _plan(W, rng):
    """-> (contig lengths, sums[sample][contig] int64 arrays): the chosen sums at random (sample, window) places of
    their window length, every other window a filler (zeros, small means, a few means up to 2000)."""
    refs = CASES[W]
    lengths = [k * W + r for k, r in refs]
    nwin = [(L + W - 1) // W for L in lengths]
    wlen = [np.minimum(np.arange(n, dtype=np.int64) * W + W, L) - np.arange(n, dtype=np.int64) * W
            for n, L in zip(nwin, lengths)]
    sums = []
    for s in range(N_SAMPLES):
        row = []
        for j in range(len(refs)):
            ln = wlen[j]
            mean = np.where(rng.random(nwin[j]) < 0.05, rng.uniform(0, 2000, nwin[j]), rng.uniform(0, 30, nwin[j]))
            f = np.floor(mean * ln).astype(np.int64)
            f[rng.random(nwin[j]) < 0.2] = 0
            row.append(f)
        sums.append(row)
    for x, chosen in _wanted(W).items():
        slots = [(s, j, w) for j in range(len(refs)) for w in np.nonzero(wlen[j] == x)[0].tolist()
                 for s in range(N_SAMPLES)]
        assert len(chosen) <= len(slots), (W, x, len(chosen), len(slots))
        for v, k in zip(chosen, rng.permutation(len(slots))[:len(chosen)].tolist()):
            s, j, w = slots[k]
            sums[s][j][w] = v
    return lengths, sums


def _oracle(sums, L, W, size):
    """One sample's cells of one contig: "%.4g" of each window's mean, parsed back, int(0.5 + x), summed over
    groups of ceil(size / W) windows (the last group of a contig may be shorter)."""
    nw = len(sums)
    st = np.arange(nw, dtype=np.int64) * W
    ln = np.minimum(st + W, L) - st
    cell = np.array([po.depthwed_cell("%.4g" % (0.0 if s == 0 else s / l)) for s, l in zip(sums.tolist(), ln.tolist())],
                    np.int64)
    g = (size + W - 1) // W
    return np.add.reduceat(cell, np.arange(0, nw, g))


def _device_matrix(eng, tids, size, shape):
    ptr, rows = eng.depthwed_device(tids, size)
    assert rows == shape[0]
    back = np.empty(shape, np.int64)
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    assert hip.hipMemcpy(back.ctypes.data, ptr, back.nbytes, 2) == 0          # hipMemcpyDeviceToHost
    return back


def _records(W, rng):
    lengths, sums = _plan(W, rng)
    n_ref = len(lengths)
    reads = {s * n_ref + j: H.window_sum_reads(rng, lengths[j], W, sums[s][j], n_filtered=3)
             for s in range(N_SAMPLES) for j in range(n_ref)}
    return lengths, sums, reads


def test_plan_places_every_chosen_sum():
    """CPU: every length of the tie grid has a W that hosts its sums, every chosen sum sits in a window of its
    length, and the records give the planned window sums (C oracle of the per-base depth)."""
    s, l = H.depthwed_tie_grid()
    hosted = set().union(*(_slot_lengths(W) for W in CASES))
    assert set(l.tolist()) <= hosted
    for W in sorted(CASES):
        lengths, sums, reads = _records(W, np.random.default_rng(W))
        n_ref = len(lengths)
        assert sum(len(r.pos) for r in reads.values()) < 4_000_000
        for x, chosen in _wanted(W).items():
            placed = []
            for j, L in enumerate(lengths):
                nw = (L + W - 1) // W
                ln = np.minimum(np.arange(nw) * W + W, L) - np.arange(nw) * W
                for smp in range(N_SAMPLES):
                    placed += sums[smp][j][ln == x].tolist()
            left = placed.copy()
            for v in chosen:
                left.remove(v)                          # raises if a chosen sum is missing
        for smp in (0, 63, 64, N_SAMPLES - 1):
            for j, L in enumerate(lengths):
                ws, _ = H.oracle_windows(po.perbase_c(reads[smp * n_ref + j], 1, 0, L), W)
                assert np.array_equal(ws, sums[smp][j]), (W, smp, j)


@pytest.mark.gpu
@pytest.mark.parametrize("W", sorted(CASES))
def test_depthwed_cells_at_rounding_ties(W):
    from goleft_amd import engine as E
    from goleft_amd.engine import DepthEngine
    lengths, sums, reads = _records(W, np.random.default_rng(W))
    n_ref = len(lengths)
    tids = np.arange(N_SAMPLES * n_ref, dtype=np.int32).reshape(N_SAMPLES, n_ref)
    sizes = [W, 3 * W + 1, max(lengths)]
    want = {}
    for size in sizes:
        cells = np.array([np.concatenate([_oracle(sums[s][j], lengths[j], W, size) for j in range(n_ref)])
                          for s in range(N_SAMPLES)]).T
        # the array restatement of depthwed.go the full-size test uses: the same cells, and the rows' extents
        second = [[po.depthwed_cells_contig(sums[s][j], lengths[j], W, size) for j in range(n_ref)]
                  for s in range(N_SAMPLES)]
        assert np.array_equal(cells, np.array([np.concatenate([c[0] for c in row]) for row in second]).T)
        ctg = np.concatenate([np.full(len(c[0]), j) for j, c in enumerate(second[0])])
        st = np.concatenate([c[1] for c in second[0]])
        en = np.concatenate([c[2] for c in second[0]])
        want[size] = cells, ctg, st, en
    rows = want[W][0].shape[0]
    assert rows > 64 and rows % 64 != 0, rows                    # a partly filled last tile of rows
    with DepthEngine(0) as eng:
        eng.set_params(window_size=W, min_mapq=1, min_cov=4)
        eng.set_contigs([lengths[j] for s in range(N_SAMPLES) for j in range(n_ref)])
        for t, r in reads.items():
            eng.push(t, r.pos, r.flag, r.mapq, r.cigar_off, r.cigar)
        for mode in ("perbase", "windows", "sums_only"):
            eng.set_outputs(perbase=mode == "perbase", sums_only=mode == "sums_only")
            eng.set_path(E.PATH_TILE if mode == "sums_only" else E.PATH_AUTO)
            eng.compute()
            if mode == "sums_only":
                assert eng.stats().tile_kernel == E.TK_SUMS_STREAM_RAW
            for s in range(N_SAMPLES):
                for j in range(n_ref):
                    assert np.array_equal(eng.window_sums(int(tids[s, j])), sums[s][j]), (mode, s, j)
            for size in sizes:
                cells, ctg, st, en = eng.depthwed(tids, size)
                w_cells, w_ctg, w_st, w_en = want[size]
                assert np.array_equal(ctg, w_ctg) and np.array_equal(st, w_st) and np.array_equal(en, w_en)
                assert cells.shape == w_cells.shape
                bad = np.argwhere(cells != w_cells)
                assert not len(bad), "%s W %d size %d: %d cells differ, first: %s" % (
                    mode, W, size, len(bad), _describe(bad[:20], cells, w_cells, ctg, st, en, sums, lengths, W, size))
                assert np.array_equal(_device_matrix(eng, tids, size, cells.shape), cells)


def _describe(bad, cells, want, ctg, st, en, sums, lengths, W, size):
    out = []
    for k, s in bad.tolist():
        j = int(ctg[k])
        item = "[contig %d %d-%d sample %d: got %d want %d" % (j, st[k], en[k], s, cells[k, s], want[k, s])
        if size == W:
            w = int(st[k]) // W
            item += ", sum %d len %d" % (sums[s][j][w], min(lengths[j], (w + 1) * W) - w * W)
        out.append(item + "]")
    return " ".join(out)
