"""GPU: gd_moving_debias and gd_moving_debias_cells (goleft_amd/csrc/gd_movdebias.hpp, gd_api_movdebias.inc) through the C
ABI against the restatement of dcnv's GeneralDebiaser (tests/movdebias_ref.py).  Every compared value is bit for bit: out
and med as their bit patterns; nothing is left out and there is no tolerance -- the selection is exact, the one division is
a correctly rounded float64 division, and the mean of the two middle values of a partial window is exact in float64.

The shapes are tests/movdebias_shapes.py's, which names the structural edge each one reaches."""
import ctypes as C

import numpy as np
import pytest

from goleft_amd import _lib
from tests import movdebias_ref as MR
from tests import movdebias_shapes as MS

pytestmark = pytest.mark.gpu

E_INVALID, E_RANGE = -1, -5
OPT_SEGMENT = 26                                 # GD_OPT_MOVDEBIAS_SEGMENT
FLT_MAX = np.finfo(np.float32).max
DENORM = np.float32(1e-45)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


class Ctx:
    def __init__(self):
        self.lib = _lib.load()
        self.h = C.c_void_p()
        assert self.lib.gd_create(0, C.byref(self.h)) == 0
        self.hip = C.CDLL("libamdhip64.so")
        self.hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]

    def err(self):
        return self.lib.gd_last_error(self.h)

    def close(self):
        self.lib.gd_destroy(self.h)

    def segment(self, rows):
        assert self.lib.gd_set_option(self.h, OPT_SEGMENT, rows) == 0, self.err().decode()

    def run(self, depths, vals, window, rows=None, n=None, want_med=True):
        d = np.ascontiguousarray(depths, np.float32)
        v = np.ascontiguousarray(vals, np.float64)
        rows, n = (d.shape[0] if rows is None else rows), (d.shape[1] if n is None else n)
        out = np.full(d.shape, np.nan, np.float32)
        med = np.full(d.shape, np.nan, np.float64)
        rc = self.lib.gd_moving_debias(self.h, d.ctypes.data, rows, n, v.ctypes.data, int(window), out.ctypes.data,
                                       med.ctypes.data if want_med else None)
        return rc, out, med

    def upload(self, a):
        a = np.ascontiguousarray(a)
        p = C.c_void_p()
        assert self.lib.gd_device_alloc(self.h, max(a.nbytes, 1), C.byref(p)) == 0
        assert self.hip.hipMemcpy(p, a.ctypes.data, a.nbytes, 1) == 0                  # hipMemcpyHostToDevice
        return p

    def read(self, p, shape, dtype):
        out = np.empty(shape, dtype)
        assert self.lib.gd_device_read(self.h, out.ctypes.data, p, out.nbytes) == 0
        return out

    def free(self, *ptrs):
        for p in ptrs:
            assert self.lib.gd_device_free(self.h, p) == 0

    def cells(self, p_cells, p_out, rows, n, vals, window):
        v = np.ascontiguousarray(vals, np.float64)
        return self.lib.gd_moving_debias_cells(self.h, p_cells, rows, n, v.ctypes.data, int(window), p_out)


@pytest.fixture(scope="module")
def ctx():
    c = Ctx()
    yield c
    c.close()


def check(ctx, m, vals, window):
    """the whole result against the restatement; returns the restatement's"""
    m = np.ascontiguousarray(m, np.float32)
    want, wmed = MR.debias(m, vals, window)
    rc, out, med = ctx.run(m, vals, window)
    assert rc == 0, ctx.err().decode()
    assert np.array_equal(bits(med), bits(wmed))
    assert np.array_equal(bits(out), bits(want))
    return want, wmed


@pytest.mark.parametrize("W", MS.WINDOWS)
def test_every_row_count_edge_of_a_window(ctx, W):
    for rows in MS.edge_rows(W):
        for kind in ("random", "reversed"):
            check(ctx, MS.float_matrix(1000 * W + rows, rows, 65), MS.vals_of(kind, rows, rows), W)
        check(ctx, MS.depth_matrix(1000 * W + rows + 1, rows, 3), MS.vals_of("tied", rows, rows), W)


@pytest.mark.parametrize("n", MS.SAMPLE_COUNTS)
def test_sample_counts_across_a_seam(ctx, n):
    rows = MS.SEG_SMALL + 44                     # a segment and a bit
    check(ctx, MS.float_matrix(100 + n, rows, n), MS.vals_of("random", n, rows), 9)
    check(ctx, MS.depth_matrix(200 + n, rows, n), MS.vals_of("tied", n, rows), 9)


def test_the_widest_matrix(ctx):
    check(ctx, MS.float_matrix(7, 12, 4096), MS.vals_of("random", 7, 12), 9)


@pytest.mark.parametrize("W", (1, 9, 63, 65, 255))
def test_rows_around_a_segment(ctx, W):
    for rows in MS.seam_rows(W):
        kind = "reversed" if rows & 1 else "random"
        check(ctx, MS.depth_matrix(300 + W + rows, rows, 5), MS.vals_of(kind, rows, rows), W)
    rows = MS.segment_of(W) + 1
    check(ctx, MS.float_matrix(400 + W, rows, 66), MS.vals_of("tied", W, rows), W)


@pytest.mark.parametrize("W", (3, 9, 17, 65))
def test_the_segment_length_changes_nothing(ctx, W):
    rows, n = 700, 70
    m, vals = MS.depth_matrix(500 + W, rows, n), MS.vals_of("tied", 500 + W, rows)
    want, wmed = MR.debias(m, vals, W)
    try:
        seen = []
        for seg in (0, 1, 7, 8, 9, 64, W, 699, 700, 5000):
            ctx.segment(seg)
            rc, out, med = ctx.run(m, vals, W)
            assert rc == 0, ctx.err().decode()
            seen.append(out.tobytes() + med.tobytes())
        assert all(s == seen[0] for s in seen)
        assert seen[0] == want.tobytes() + wmed.tobytes()
    finally:
        ctx.segment(0)
    assert ctx.lib.gd_set_option(ctx.h, OPT_SEGMENT, -1) == E_INVALID


def test_hand_made_columns_and_extremes(ctx):
    # the columns tests/test_movdebias_ref.py works out by hand
    _, med = check(ctx, np.array([[4], [8], [2], [16], [5]], np.float32), np.arange(5.0), 1)
    assert med[:, 0].tolist() == [4, 2, 16, 5, 5]
    _, med = check(ctx, np.array([[10], [20], [1000], [2000], [30], [60], [40]], np.float32), np.arange(7.0), 3)
    assert med[:, 0].tolist() == [15, 15, 20, 30, 40, 40, 40]
    # medians below 1 (the divisor is 1), an all-zero column with a -0.0, denormals, FLT_MAX
    rows = 40
    m = np.zeros((rows, 5), np.float32)
    m[:, 0] = 0.25
    m[::7, 0] = 0.5
    m[5, 1] = -0.0
    m[:, 2] = DENORM
    m[::3, 2] = np.float32(3e-45)
    m[:, 3] = FLT_MAX
    m[::4, 3] = 0.0
    m[:, 4] = np.arange(rows) * 3 + 2
    for W in (1, 3, 9, 17):
        want, med = check(ctx, m, np.arange(float(rows)), W)
        assert np.array_equal(bits(want[:, :3]), bits(m[:, :3])) and not bits(med[:, 1]).any()
    # the mean of two FLT_MAX is finite in float64
    want, med = check(ctx, np.full((2, 1), FLT_MAX, np.float32), [0.0, 1.0], 3)
    assert med[0, 0] == float(FLT_MAX) and want[0, 0] == 1.0


def test_tied_covariates_go_by_row(ctx):
    rows = 90
    m = MS.depth_matrix(61, rows, 4)
    check(ctx, m, np.zeros(rows), 9)                             # all tied: the matrix's own order
    check(ctx, m, np.repeat([0.5, 0.25, 0.75], 30), 9)
    check(ctx, m, np.tile([0.5, 0.25, 0.75], 30), 3)


def test_permuting_rows_permutes_the_output(ctx):
    rng = np.random.default_rng(91)
    rows, n = 300, 70
    vals = rng.permutation(rows).astype(np.float64)             # (no ties: the order does not depend on the rows' places)
    m = MS.depth_matrix(92, rows, n)
    rc, out, med = ctx.run(m, vals, 9)
    assert rc == 0
    p = rng.permutation(rows)
    rc, pout, pmed = ctx.run(m[p], vals[p], 9)
    assert rc == 0
    assert np.array_equal(bits(pout), bits(out[p])) and np.array_equal(bits(pmed), bits(med[p]))


def test_med_may_be_left_out_and_calls_repeat(ctx):
    m, vals = MS.depth_matrix(95, 40, 5), MS.vals_of("random", 96, 40)
    want, _ = check(ctx, m, vals, 9)
    rc, out, med = ctx.run(m, vals, 9, want_med=False)
    assert rc == 0 and np.array_equal(bits(out), bits(want)) and np.isnan(med).all()
    t = (C.c_double * 4)()
    assert ctx.lib.gd_moving_debias_timing(ctx.h, t, 4) == 0
    assert all(x >= 0 for x in t) and t[2] > 0


def test_the_engine_method_is_the_abi_call(ctx):
    from goleft_amd.engine import DepthEngine
    m, vals = MS.depth_matrix(97, 300, 66), MS.vals_of("tied", 98, 300)
    want, wmed = MR.debias(m, vals, 9)
    with DepthEngine(0) as eng:
        out = eng.moving_debias(m, vals, 9)
        assert np.array_equal(bits(out), bits(want))
        out, med = eng.moving_debias(m, vals, 9, want_med=True)
        assert np.array_equal(bits(out), bits(want)) and np.array_equal(bits(med), bits(wmed))
        assert len(eng.moving_debias_timing()) == 4


# ------------------------------------------------------------------------------------------------------ the resident form

EDGE_CELLS = (0, 1, 2 ** 24, 2 ** 24 + 1, 2 ** 24 + 3, 2 ** 53 + 1, 2 ** 63 - 1)


@pytest.mark.parametrize("rows,n,W", ((5, 1, 9), (300, 65, 9), (257, 200, 17), (70, 64, 65)))
def test_cells_are_the_host_form_on_float_cells(ctx, rows, n, W):
    rng = np.random.default_rng(rows + n)
    cells = rng.poisson(40.0, (rows, n)).astype(np.int64)
    cells[rng.random((rows, n)) < 0.1] = 0
    flat = cells.reshape(-1)
    flat[:len(EDGE_CELLS)][:flat.size] = EDGE_CELLS[:flat.size]  # (float)cell rounds to nearest even
    vals = MS.vals_of("tied", rows, rows)
    rc, want, _ = ctx.run(cells.astype(np.float32), vals, W)
    assert rc == 0, ctx.err().decode()
    assert np.array_equal(bits(want), bits(MR.debias(cells.astype(np.float32), vals, W)[0]))
    p, q = ctx.upload(cells), ctx.upload(np.full((rows, n), np.nan, np.float32))
    try:
        assert ctx.cells(p, q, rows, n, vals, W) == 0, ctx.err().decode()
        assert np.array_equal(bits(ctx.read(q, (rows, n), np.float32)), bits(want))
        assert np.array_equal(ctx.read(p, (rows, n), np.int64), cells)       # the cells are only read
    finally:
        ctx.free(p, q)


def test_cells_refusals_leave_the_context_usable(ctx):
    good = np.arange(24, dtype=np.int64).reshape(6, 4) * 7
    vals = np.array([0.1, 0.5, 0.1, 0.9, 0.5, 0.1])
    want = MR.debias(good.astype(np.float32), vals, 3)[0]
    primed = np.full((6, 4), 7.5, np.float32)

    def fine():
        p, q = ctx.upload(good), ctx.upload(primed)
        try:
            assert ctx.cells(p, q, 6, 4, vals, 3) == 0, ctx.err().decode()
            assert np.array_equal(bits(ctx.read(q, (6, 4), np.float32)), bits(want))
        finally:
            ctx.free(p, q)

    fine()
    for at in (0, 13, 23):                       # a negative cell: found by the pass that converts, d_out untouched
        bad = good.copy()
        bad.reshape(-1)[at] = -1
        p, q = ctx.upload(bad), ctx.upload(primed)
        try:
            assert ctx.cells(p, q, 6, 4, vals, 3) == E_INVALID and b"negative" in ctx.err()
            assert np.array_equal(bits(ctx.read(q, (6, 4), np.float32)), bits(primed))
        finally:
            ctx.free(p, q)
        fine()
    p = ctx.upload(good)
    try:
        last = p.value + good.nbytes - 1
        for out in (p.value, last, p.value - good.size * 4 + 1, p.value + 8):
            assert ctx.cells(p, C.c_void_p(out), 6, 4, vals, 3) == E_INVALID and b"overlap" in ctx.err(), out - p.value
        assert np.array_equal(ctx.read(p, good.shape, np.int64), good)
        q = ctx.upload(primed)
        try:
            # gd_moving_debias's own refusals
            for rows, n, W, code in ((6, 0, 3, E_RANGE), (6, 4097, 3, E_RANGE), (6, 4, 2, E_RANGE), (6, 4, 257, E_RANGE),
                                     (6, 4, 13, E_RANGE), (2 ** 31, 4, 3, E_RANGE)):
                assert ctx.cells(p, q, rows, n, np.zeros(6), W) == code, (rows, n, W)
            v = vals.copy()
            v[2] = np.nan
            assert ctx.cells(p, q, 6, 4, v, 3) == E_INVALID and b"row 2" in ctx.err()
            assert ctx.lib.gd_moving_debias_cells(ctx.h, None, 6, 4, vals.ctypes.data, 3, q) == E_INVALID
            assert ctx.lib.gd_moving_debias_cells(ctx.h, p, 6, 4, vals.ctypes.data, 3, None) == E_INVALID
            assert np.array_equal(bits(ctx.read(q, (6, 4), np.float32)), bits(primed))
        finally:
            ctx.free(q)
    finally:
        ctx.free(p)
    fine()


# --------------------------------------------------------------------------------------------------------- the refusals

def test_refused_inputs_leave_the_context_usable(ctx):
    good = MS.depth_matrix(97, 6, 4)
    vals = np.array([0.1, 0.5, 0.1, 0.9, 0.5, 0.1])

    def fine():
        check(ctx, good, vals, 3)

    def untouched(out, med):
        return np.isnan(out).all() and np.isnan(med).all()

    fine()
    wide = np.zeros((1, 4097), np.float32)
    for rows, n in ((6, 0), (6, -1), (1, 4097), (2 ** 31, 4)):
        src = wide if n == 4097 else good
        rc, out, med = ctx.run(src, np.zeros(max(src.shape[0], 1)), 1, rows=rows, n=n)
        assert rc == E_RANGE and untouched(out, med), (rows, n)
        fine()
    for W in (0, 2, 4, 8, 256, 257, -1, -3, 2 ** 31 - 1):       # even, or outside 1 .. 255
        rc, out, med = ctx.run(good, vals, W)
        assert rc == E_RANGE and b"window" in ctx.err() and untouched(out, med), W
        fine()
    for W, rows in ((3, 1), (9, 4), (13, 6), (255, 127), (1, 0)):   # fewer rows than mid: Go indexes past the column
        big = MS.depth_matrix(1, max(rows, 1), 4)
        rc, out, med = ctx.run(big, np.zeros(max(rows, 1)), W, rows=rows)
        assert rc == E_RANGE and b"rows" in ctx.err() and untouched(out, med), (W, rows)
        fine()
    assert ctx.run(good, vals, 11)[0] == 0       # mid = 6 = rows
    for bad in (np.nan, np.inf, -1.0, -DENORM):
        m = good.copy()
        m[3, 2] = bad
        rc, out, med = ctx.run(m, vals, 3)
        assert rc == E_INVALID and b"row 3, sample 2" in ctx.err() and untouched(out, med)
        fine()
    for bad in (np.nan, np.inf, -np.inf):
        v = vals.copy()
        v[4] = bad
        rc, out, med = ctx.run(good, v, 3)
        assert rc == E_INVALID and b"row 4" in ctx.err() and untouched(out, med)
        fine()
    d, v = np.ascontiguousarray(good), np.ascontiguousarray(vals)
    o = np.empty_like(d)
    assert ctx.lib.gd_moving_debias(ctx.h, None, 6, 4, v.ctypes.data, 3, o.ctypes.data, None) == E_INVALID
    assert ctx.lib.gd_moving_debias(ctx.h, d.ctypes.data, 6, 4, None, 3, o.ctypes.data, None) == E_INVALID
    assert ctx.lib.gd_moving_debias(ctx.h, d.ctypes.data, 6, 4, v.ctypes.data, 3, None, None) == E_INVALID
    fine()
