"""GPU: gd_chunk_debias (goleft_amd/csrc/gd_chunkdebias.hpp, gd_api_chunkdebias.inc) through the C ABI against the
restatement of dcnv's ChunkDebiaser (tests/debias_ref.py).  Every compared value is bit for bit: out and out64 as their bit
patterns, chunk_of_row, the chunk count and the medians; nothing is left out and there is no tolerance.

The shapes follow the kernel's mapping: 64 columns a workgroup (one per lane), 8 waves x 8 rows a
turn of a chunk's rows, at most 4096 workgroups a column tile with the chunks strided over them, 8-bit digits from the top,
big chunks not cut."""
import ctypes as C

import numpy as np
import pytest

from goleft_amd import _lib
from tests import debias_ref as DR

pytestmark = pytest.mark.gpu

E_INVALID, E_RANGE, E_CAPACITY = -1, -5, -8
COLS = 64                # columns of a workgroup (CD_COLS)
WAVE_TURN = 8            # rows a wave has in flight (CD_ROWS); also the waves of a workgroup (CD_WAVES)
TURN = 64                # rows of a workgroup's turn (CD_TURN = CD_WAVES * CD_ROWS)
GRID = 4096              # workgroups of a column tile (CD_MAX_GRID): more chunks than this are strided over them
SAMPLE_COUNTS = (1, 63, 64, 65, 129)
EDGE_SIZES = (1, 2, 3, WAVE_TURN - 1, WAVE_TURN, WAVE_TURN + 1, TURN - 1, TURN, TURN + 1, 2 * TURN - 1, 2 * TURN, 2 * TURN + 1)
FLT_MAX = np.finfo(np.float32).max
DENORM = np.float32(1e-45)                       # the smallest denormal, bits 1


class Ctx:
    def __init__(self):
        self.lib = _lib.load()
        self.h = C.c_void_p()
        assert self.lib.gd_create(0, C.byref(self.h)) == 0

    def err(self):
        return self.lib.gd_last_error(self.h)

    def close(self):
        self.lib.gd_destroy(self.h)

    def run(self, depths, vals, window, rows=None, n=None, med_rows=None, want64=True):
        d = np.ascontiguousarray(depths, np.float32)
        v = np.ascontiguousarray(vals, np.float64)
        rows, n = (d.shape[0] if rows is None else rows), (d.shape[1] if n is None else n)
        out = np.full(d.shape, np.nan, np.float32)
        out64 = np.full(d.shape, np.nan, np.float64)
        cor = np.full(max(d.shape[0], 1), 0xffffffff, np.uint32)
        cap = d.shape[0] if med_rows is None else med_rows
        med = np.full((max(cap, 1), d.shape[1]), np.nan, np.float32)
        nc = C.c_size_t(2 ** 63)
        rc = self.lib.gd_chunk_debias(self.h, d.ctypes.data, rows, n, v.ctypes.data, float(window), out.ctypes.data,
                                      out64.ctypes.data if want64 else None, cor.ctypes.data, C.byref(nc), med.ctypes.data, cap)
        return rc, out, out64, cor, nc.value, med


@pytest.fixture(scope="module")
def ctx():
    c = Ctx()
    yield c
    c.close()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def check(ctx, m, vals, window):
    """the whole result against the restatement; returns the restatement's"""
    m = np.ascontiguousarray(m, np.float32)
    w64, w32, wcor, wC, wmed = DR.debias(m, vals, window)
    rc, out, out64, cor, nc, med = ctx.run(m, vals, window)
    assert rc == 0, ctx.err().decode()
    assert nc == wC
    assert np.array_equal(cor, wcor)
    assert np.array_equal(bits(med[:wC]), bits(wmed))
    assert np.array_equal(bits(out64), bits(w64))
    assert np.array_equal(bits(out), bits(w32))
    return w64, w32, wcor, wC, wmed


def float_matrix(seed, rows, n):
    """any finite float32 >= 0 as its bit pattern (denormals included), a third of the cells zero, some of them -0.0"""
    rng = np.random.default_rng(seed)
    m = rng.integers(0, 0x7f800000, size=(rows, n), dtype=np.int64).astype(np.uint32).view(np.float32).copy()
    z = rng.random((rows, n))
    m[z < 0.33] = 0.0
    m[z < 0.05] = -0.0
    return m


def depth_matrix(seed, rows, n):
    """depths as a cohort has them: integers around a sample's level (many duplicates), some zero"""
    rng = np.random.default_rng(seed)
    m = rng.poisson(rng.uniform(5.0, 300.0, size=(1, n)), size=(rows, n)).astype(np.float32)
    m[rng.random((rows, n)) < 0.2] = 0.0
    return m


def vals_of_sizes(sizes, seed):
    """vals (window 0.5) that cut sum(sizes) rows into chunks of these sizes in value order, the rows of a chunk
    scattered over the matrix"""
    v = np.repeat(np.arange(len(sizes), dtype=np.float64), sizes)
    return np.random.default_rng(seed).permutation(v)


@pytest.mark.parametrize("n", SAMPLE_COUNTS)
def test_sample_counts_with_every_chunk_size_edge(ctx, n):
    vals = vals_of_sizes(EDGE_SIZES, n)
    _, _, cor, C_, _ = check(ctx, float_matrix(100 + n, len(vals), n), vals, 0.5)
    assert C_ == len(EDGE_SIZES) and sorted(np.bincount(cor).tolist()) == sorted(EDGE_SIZES)
    check(ctx, depth_matrix(200 + n, len(vals), n), vals, 0.5)


def test_the_widest_matrix(ctx):
    vals = vals_of_sizes((1, 5, TURN + 1), 7)
    check(ctx, float_matrix(7, len(vals), 4096), vals, 0.5)


@pytest.mark.parametrize("n", (1, 65))
def test_one_chunk_of_all_rows(ctx, n):
    rows = 3 * TURN + 5
    vals = np.random.default_rng(3).random(rows)
    _, _, cor, C_, _ = check(ctx, float_matrix(31 + n, rows, n), vals, 1.0)
    assert C_ == 1 and not cor.any()
    check(ctx, depth_matrix(32 + n, rows, n), np.full(rows, 0.41), 0.01)                 # all vals equal


def test_a_chunk_a_row_and_more_chunks_than_workgroups(ctx):
    rows = GRID + 5
    vals = np.random.default_rng(4).permutation(rows).astype(np.float64)
    _, _, cor, C_, med = check(ctx, float_matrix(41, rows, 3), vals, 0.5)
    assert C_ == rows and np.array_equal(cor, vals.astype(np.uint32))
    rows = 70
    vals = np.random.default_rng(5).permutation(rows).astype(np.float64)
    _, _, _, C_, _ = check(ctx, depth_matrix(42, rows, 65), vals, 0.5)
    assert C_ == rows


def test_a_chunk_at_both_ends_and_the_middle_of_the_matrix(ctx):
    rows = 2 * TURN + 3
    vals = np.full(rows, 0.3)
    vals[[0, rows // 2, rows - 1]] = 0.7         # the upper chunk: first, middle and last row
    vals[[1, rows - 2]] = 0.1                    # the lowest: second and last but one
    _, _, cor, C_, _ = check(ctx, depth_matrix(51, rows, 9), vals, 0.05)
    assert C_ == 3 and cor[0] == cor[rows // 2] == cor[-1] == 2 and cor[1] == cor[-2] == 0


def test_ties_and_the_exact_window(ctx):
    W = 0.25
    at, above = 0.5 + W, np.nextafter(0.5 + W, np.inf)
    m = depth_matrix(61, 8, 5)
    # ties on both sides of a boundary
    _, _, cor, C_, _ = check(ctx, m, [0.5, 0.5, above, above, 0.5, above, above, 0.5], W)
    assert C_ == 2 and cor.tolist() == [0, 0, 1, 1, 0, 1, 1, 0]
    # a gap of exactly W stays in the chunk, one ulp more opens the next
    _, _, cor, C_, _ = check(ctx, m, [0.5, at, 0.5, at, at, 0.5, 0.5, at], W)
    assert C_ == 1
    _, _, cor, C_, _ = check(ctx, m, [0.5, at, above, at, at, 0.5, above, at], W)
    assert C_ == 2 and cor.tolist() == [0, 0, 1, 0, 0, 0, 1, 0]
    _, _, cor, C_, _ = check(ctx, m[:2], [0.1, 0.3], 0.2)
    assert C_ == 1
    _, _, cor, C_, _ = check(ctx, m[:2], [0.1 + 0.2, 0.1], 0.2)
    assert C_ == 2 and cor.tolist() == [1, 0]


def test_the_zero_count_quirk(ctx):
    # one chunk of n rows; column s has k zeros: n = 3k - 1, 3k, 3k + 1 and neighbours
    for n in (1, 2, 3, 5, 6, 7, 8, 9, 10, TURN + 2, 3 * TURN, 3 * TURN + 1):
        ks = sorted({0, 1, n // 3, (n + 1) // 3, (n + 2) // 3, n // 2, n - 1, n} & set(range(n + 1)))
        rng = np.random.default_rng(n)
        m = rng.integers(1, 40, (n, len(ks))).astype(np.float32)
        for s, k in enumerate(ks):
            z = rng.permutation(n)[:k]
            m[z, s] = 0.0
            m[z[::2], s] = -0.0
        _, _, _, _, med = check(ctx, m, np.zeros(n), 1.0)
        for s, k in enumerate(ks):
            assert (med[0, s] == 0) == (n < 3 * k or k == n), (n, k)
    # an all-zero chunk beside full ones, the zeros of both signs
    vals = vals_of_sizes((TURN, 5, TURN + 3), 9)
    m = depth_matrix(71, len(vals), 66) + 1
    m[vals == 1.0] = 0.0
    m[np.flatnonzero(vals == 1.0)[:2], ::2] = -0.0
    w64, w32, _, _, med = check(ctx, m, vals, 0.5)
    assert not med[1].any() and not w64[vals == 1.0].any() and np.all(med[0] > 0) and np.all(med[2] > 0)


def test_columns_built_for_each_pass(ctx):
    # the cells of a column's chunk equal in all but one byte, once for each byte a pass decides
    rng = np.random.default_rng(81)
    n = TURN + 9
    base = np.uint32(0x2a5b6c7d)
    cols = []
    for byte in range(4):
        digits = rng.integers(0, 128 if byte == 3 else 256, n).astype(np.uint32)
        if byte == 3:
            digits = np.minimum(digits, 0x7e)    # (stay finite)
        cols.append((base & ~np.uint32(0xff << (8 * byte))) | (digits << np.uint32(8 * byte)))
    cols.append(np.full(n, base, np.uint32))                                  # every cell the same
    cols.append(rng.integers(1, 0x00800000, n).astype(np.uint32))            # denormals only
    cols.append(np.where(rng.random(n) < 0.5, rng.integers(1, 0x00800000, n), 0).astype(np.uint32))
    m = np.stack(cols, 1).view(np.float32)
    check(ctx, m, np.zeros(n), 1.0)
    check(ctx, m, vals_of_sizes((n - 12, 12), 2), 0.5)
    # FLT_MAX over a denormal median: inf as a float32, finite as a float64
    m = np.array([[FLT_MAX, 3.0], [DENORM, 3.0], [DENORM, FLT_MAX]], np.float32)
    w64, w32, _, _, med = check(ctx, m, np.zeros(3), 1.0)
    assert bits(med)[0, 0] == 1 and np.isinf(w32[0, 0]) and np.isfinite(w64[0, 0]) and w32[2, 1] == FLT_MAX / np.float32(3.0)
    # random bit patterns of every magnitude, many chunks
    vals = np.round(np.random.default_rng(82).normal(0.41, 0.05, 700), 3)
    _, _, _, C_, _ = check(ctx, float_matrix(83, 700, 67), vals, 0.01)
    assert 10 < C_ < 60


def test_permuting_rows_permutes_the_output(ctx):
    rng = np.random.default_rng(91)
    rows, n = 300, 70
    vals = np.round(rng.normal(0.41, 0.05, rows), 2)
    m = depth_matrix(92, rows, n)
    rc, out, out64, cor, nc, med = ctx.run(m, vals, 0.03)
    assert rc == 0
    p = rng.permutation(rows)
    rc, pout, pout64, pcor, pnc, pmed = ctx.run(m[p], vals[p], 0.03)
    assert rc == 0 and pnc == nc
    assert np.array_equal(bits(pout), bits(out[p])) and np.array_equal(bits(pout64), bits(out64[p]))
    assert np.array_equal(pcor, cor[p]) and np.array_equal(bits(pmed[:nc]), bits(med[:nc]))


def test_outputs_may_be_left_out_and_calls_repeat(ctx):
    m = depth_matrix(95, 40, 5)
    vals = np.random.default_rng(96).random(40)
    _, w32, _, _, _ = check(ctx, m, vals, 0.1)
    d, v = np.ascontiguousarray(m), np.ascontiguousarray(vals)
    out = np.empty_like(d)
    assert ctx.lib.gd_chunk_debias(ctx.h, d.ctypes.data, 40, 5, v.ctypes.data, 0.1, out.ctypes.data, None, None, None, None, 0) == 0
    assert np.array_equal(bits(out), bits(w32))
    t = (C.c_double * 7)()
    assert ctx.lib.gd_chunk_debias_timing(ctx.h, t, 7) == 0
    assert t[4] == len(DR.chunks(vals, 0.1)[1]) - 1 and t[5] >= 1 and all(x >= 0 for x in t)


def test_refused_inputs_leave_the_context_usable(ctx):
    good = depth_matrix(97, 6, 4)
    vals = np.array([0.1, 0.5, 0.1, 0.9, 0.5, 0.1])

    def fine():
        check(ctx, good, vals, 0.1)

    wide = np.zeros((1, 4097), np.float32)
    for rows, n, want in ((6, 0, E_RANGE), (6, -1, E_RANGE), (1, 4097, E_RANGE), (0, 4, E_RANGE), (2 ** 31, 4, E_RANGE)):
        src = wide if n == 4097 else good
        assert ctx.run(src, np.zeros(max(src.shape[0], 1)), 0.1, rows=rows, n=n)[0] == want, (rows, n)
        fine()
    for bad in (np.nan, np.inf, -1.0, -DENORM):
        m = good.copy()
        m[3, 2] = bad
        assert ctx.run(m, vals, 0.1)[0] == E_INVALID
        assert b"row 3, sample 2" in ctx.err()
        fine()
    for bad in (np.nan, np.inf, -np.inf):
        v = vals.copy()
        v[4] = bad
        assert ctx.run(good, v, 0.1)[0] == E_INVALID
        assert b"row 4" in ctx.err()
        fine()
    for w in (0.0, -0.0, -0.01, np.nan, np.inf):
        assert ctx.run(good, vals, w)[0] == E_INVALID
        assert b"window" in ctx.err()
        fine()
    rc, _, _, _, nc, _ = ctx.run(good, vals, 0.1, med_rows=2)                # three chunks
    assert rc == E_CAPACITY and nc == 3
    fine()
    assert ctx.run(good, vals, 0.1, med_rows=3)[0] == 0
