"""GPU: a depth matrix that stays in HBM (goleft_amd/csrc/gd_devmat.hpp, gd_api_devmat.inc) through
the C ABI: gd_chunk_debias_cells, gd_device_scale, gd_sample_medians_device, gd_emdepth_device, gd_emcnv_add_device, and the
composed goleft_amd.emdepth.cohort_cnvs.

Everything compared is compared exactly -- floats as their bit patterns, outputs of a device twin as the bytes of its host
twin -- and there is no tolerance anywhere: the resident entries run the kernels of the host entries on the same bits, and
the one new piece of arithmetic, (float)cell, is a single rounding numpy's astype(float32) makes too.

The shapes follow the kernels' mapping: 64 columns a workgroup (one per lane), a wave a row and 4 waves a workgroup, 4 rows
of a wave in flight a turn, at most 2048 workgroups a column tile, so 2048 x 4 rows before the stride loop turns and
4 x 2048 x 4 before a wave's whole turn of four rows runs twice."""
import ctypes as C
import functools
import subprocess

import numpy as np
import pytest

from goleft_amd import _lib
from tests import debias_ref as DR
from tests import emcnv_ref as CR
from tests import emcnv_shapes as CS
from tests import emdepth_ref as R
from tests import emdepth_shapes as ES
from tests import helpers as H
from tests import scales_ref as SR

pytestmark = pytest.mark.gpu

E_INVALID, E_RANGE = -1, -5
WAVES, GRID, ROWS_IN_FLIGHT = 4, 2048, 4         # DM_WAVES, DM_MAX_GRID, DM_ROWS
SWEEP = GRID * WAVES                             # rows one sweep of the grid covers
SAMPLE_COUNTS = (1, 63, 64, 65, 129, 4096)
ROW_COUNTS = (1, 2, 3, 4, 5, 65)
EDGE_CELLS = (0, 1, 2 ** 24, 2 ** 24 + 1, 2 ** 24 + 3, 2 ** 53 + 1, 2 ** 63 - 1)
FLT_MAX = np.finfo(np.float32).max
DENORM = np.float32(1e-45)
KEYS = ("sample", "psize", "emit_row", "member_off", "member_row", "depth", "cn", "log2fc")
DTYPES = (np.uint32, np.uint32, np.uint32, np.uint64, np.uint32, np.float32, np.uint8, np.float32)


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

    def ok(self, rc):
        assert rc == 0, self.err().decode()

    def err(self):
        return self.lib.gd_last_error(self.h)

    def close(self):
        self.lib.gd_destroy(self.h)

    def alloc(self, nbytes):
        p = C.c_void_p()
        self.ok(self.lib.gd_device_alloc(self.h, nbytes, C.byref(p)))
        return p

    def upload(self, a):
        a = np.ascontiguousarray(a)
        p = self.alloc(a.nbytes)
        if a.nbytes:
            assert self.hip.hipMemcpy(p, a.ctypes.data, a.nbytes, 1) == 0              # hipMemcpyHostToDevice
        return p

    def free(self, *ptrs):
        for p in ptrs:
            self.ok(self.lib.gd_device_free(self.h, p))

    def read(self, p, shape, dtype):
        out = np.empty(shape, dtype)
        self.ok(self.lib.gd_device_read(self.h, out.ctypes.data, p, out.nbytes))
        return out

    # ---- gd_chunk_debias and its resident form
    def debias_host(self, depths, vals, window):
        d, v = np.ascontiguousarray(depths, np.float32), np.ascontiguousarray(vals, np.float64)
        out, cor, med, nc = np.empty_like(d), np.empty(d.shape[0], np.uint32), np.empty(d.shape, np.float32), C.c_size_t()
        self.ok(self.lib.gd_chunk_debias(self.h, d.ctypes.data, d.shape[0], d.shape[1], v.ctypes.data, float(window),
                                         out.ctypes.data, None, cor.ctypes.data, C.byref(nc), med.ctypes.data, d.shape[0]))
        return out, cor, nc.value, med[:nc.value]

    def debias_cells(self, p_cells, p_out, rows, n, vals, window, med_rows=None):
        """(rc, chunk_of_row, n_chunks, med) with the host outputs primed, so that an untouched one shows"""
        v = np.ascontiguousarray(vals, np.float64)
        cap = rows if med_rows is None else med_rows
        held = min(rows, 1 << 20)                                # (a refused row count allocates nothing here either)
        cor, nc = np.full(max(held, 1), 0xffffffff, np.uint32), C.c_size_t(2 ** 63)
        med = np.full((max(min(cap, held), 1), max(n, 1)), np.nan, np.float32)
        rc = self.lib.gd_chunk_debias_cells(self.h, p_cells, rows, n, v.ctypes.data, float(window), p_out, cor.ctypes.data,
                                            C.byref(nc), med.ctypes.data, cap)
        return rc, cor, nc.value, med

    # ---- the three twins
    def em_outputs(self, rows, n):
        return [np.full((rows, 9), np.nan), np.full(rows, 255, np.uint8), np.full((rows, n), 255, np.uint8),
                np.full((rows, n), np.nan, np.float32)]

    def emdepth(self, d, p=None):
        """gd_emdepth on d, or gd_emdepth_device on the device matrix p of d's shape: (rc, outputs)"""
        out = self.em_outputs(*d.shape)
        ptrs = [o.ctypes.data for o in out]
        if p is None:
            return self.lib.gd_emdepth(self.h, d.ctypes.data, d.shape[0], d.shape[1], *ptrs), out
        return self.lib.gd_emdepth_device(self.h, p, d.shape[0], d.shape[1], *ptrs), out

    def medians(self, d, p=None):
        med, nz = np.full(d.shape[1], np.nan, np.float32), np.full(d.shape[1], 2 ** 64 - 1, np.uint64)
        fn = self.lib.gd_sample_medians if p is None else self.lib.gd_sample_medians_device
        return fn(self.h, d.ctypes.data if p is None else p, d.shape[0], d.shape[1], med.ctypes.data, nz.ctypes.data), [med, nz]

    def add(self, d, st, en, cn=None, p=None):
        fn = self.lib.gd_emcnv_add if p is None else self.lib.gd_emcnv_add_device
        return fn(self.h, (d.ctypes.data if d.size else None) if p is None else p, d.shape[0], st.ctypes.data if st.size else None,
                  en.ctypes.data if en.size else None, cn.ctypes.data if cn is not None else None)

    def calls(self):
        nc, nm = C.c_uint64(), C.c_uint64()
        self.ok(self.lib.gd_emcnv_finish(self.h, C.byref(nc), C.byref(nm)))
        sizes = (nc.value,) * 3 + (nc.value + 1,) + (nm.value,) * 4
        out = [np.zeros(k, dt) for k, dt in zip(sizes, DTYPES)]
        self.ok(self.lib.gd_emcnv_read(self.h, *[o.ctypes.data for o in out]))
        self.ok(self.lib.gd_emcnv_end(self.h))
        return dict(zip(KEYS, out))

    def cnvs(self, d, st, en, cuts, p=None):
        """begin .. read, the rows cut at `cuts`; on the device matrix p when given"""
        rows, n = d.shape
        self.ok(self.lib.gd_emcnv_begin(self.h, n))
        cn = np.full(d.shape, 255, np.uint8)
        edges = [0] + [c for c in cuts if 0 < c < rows] + [rows]
        for r0, r1 in zip(edges[:-1], edges[1:]):
            at = None if p is None else C.c_void_p(p.value + r0 * n * 4)
            self.ok(self.add(d[r0:r1], st[r0:r1], en[r0:r1], cn[r0:r1], at))
        out = self.calls()
        out["site_cn"] = cn
        return out


@pytest.fixture(scope="module")
def ctx():
    c = Ctx()
    yield c
    c.close()


def same_bytes(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------- conversion and debias

def cell_matrix(seed, rows, n, edges=True):
    """cohort-like integer cells with many duplicates and zeros, every edge cell of the conversion among them"""
    rng = np.random.default_rng(seed)
    m = rng.poisson(rng.uniform(5.0, 300.0, size=(1, n)), size=(rows, n)).astype(np.int64)
    m[rng.random((rows, n)) < 0.2] = 0
    if not edges:
        return m
    flat = m.reshape(-1)
    at = rng.permutation(flat.size)[:len(EDGE_CELLS)]
    flat[at] = np.array(EDGE_CELLS, np.int64)[:len(at)]
    return m


def check_debias(ctx, cells, vals, window):
    """gd_chunk_debias_cells against the restatement and against gd_chunk_debias, both on cells.astype(float32)"""
    cells = np.ascontiguousarray(cells, np.int64)
    rows, n = cells.shape
    f = cells.astype(np.float32)                                 # one rounding, to nearest even
    _, w32, wcor, wC, wmed = DR.debias(f, vals, window)
    h32, hcor, hC, hmed = ctx.debias_host(f, vals, window)
    p, q = ctx.upload(cells), ctx.alloc(f.nbytes)
    try:
        rc, cor, nc, med = ctx.debias_cells(p, q, rows, n, vals, window)
        ctx.ok(rc)
        out = ctx.read(q, (rows, n), np.float32)
        back = ctx.read(p, (rows, n), np.int64)
    finally:
        ctx.free(p, q)
    assert np.array_equal(back, cells)                           # the cells are only read
    assert nc == wC == hC
    assert np.array_equal(cor, wcor) and np.array_equal(cor, hcor)
    assert np.array_equal(bits(med[:nc]), bits(wmed)) and np.array_equal(bits(med[:nc]), bits(hmed))
    assert np.array_equal(bits(out), bits(w32)) and np.array_equal(bits(out), bits(h32))
    assert not np.isinf(out).any()                               # (a median is a cell >= 1: no quotient of an int64 overflows)
    return out, med[:nc]


def test_the_conversion_rounds_once_to_nearest_even(ctx):
    cells = np.array([EDGE_CELLS], np.int64).T.repeat(2, 1)      # one chunk a row: rows 0 .. 6 are their own medians
    want = np.array([0, 1, 2 ** 24, 2 ** 24, 2 ** 24 + 4, 2 ** 53, 2 ** 63], np.float64).astype(np.float32)
    assert np.array_equal(cells[:, 0].astype(np.float32), want)  # (numpy's rounding is the one the header states)
    out, med = check_debias(ctx, cells, np.arange(len(EDGE_CELLS), dtype=np.float64), 0.5)
    assert np.array_equal(bits(med[:, 0]), bits(want))
    # in one chunk the quotients keep the rounded cells apart: the median is 2^24
    out, med = check_debias(ctx, cells, np.zeros(len(EDGE_CELLS)), 0.5)
    assert med[0, 0] == np.float32(2 ** 24) and out[4, 0] == np.float32((2 ** 24 + 4) / 2 ** 24) and out[3, 0] == 1.0


@pytest.mark.parametrize("n", SAMPLE_COUNTS)
def test_debias_sample_and_row_counts(ctx, n):
    for rows in ROW_COUNTS if n < 4096 else (1, 5):
        vals = np.random.default_rng(rows).integers(0, 3, rows).astype(np.float64)
        check_debias(ctx, cell_matrix(1000 * n + rows, rows, n), vals, 0.5)


@pytest.mark.parametrize("rows", (SWEEP + 5, ROWS_IN_FLIGHT * SWEEP + 5))
def test_debias_more_rows_than_the_grid_holds(ctx, rows):
    """the stride loop turns: one row at a time past one sweep, whole turns of four twice past four sweeps"""
    vals = np.round(np.random.default_rng(rows).normal(0.41, 0.05, rows), 2)
    check_debias(ctx, cell_matrix(rows, rows, 3), vals, 0.03)


def test_debias_a_chunk_whose_median_is_zero(ctx):
    cells = cell_matrix(77, 70, 66, edges=False) + 1
    vals = np.repeat([0.0, 1.0, 2.0], (30, 5, 35))[np.random.default_rng(5).permutation(70)]
    cells[vals == 1.0] = 0                                       # an all-zero chunk: its cells stay
    cells[np.flatnonzero(vals == 2.0)[:30], 7] = 0               # n < 3k: the median is a zero
    out, med = check_debias(ctx, cells, vals, 0.5)
    assert not med[1].any() and med[2, 7] == 0 and np.all(med[0] > 0)
    assert np.array_equal(out[vals == 2.0][:, 7], cells[vals == 2.0][:, 7].astype(np.float32))


def test_an_overflowing_quotient_needs_a_float_matrix(ctx):
    # FLT_MAX over a denormal median is inf as a float32: only gd_chunk_debias can be handed one
    m = np.array([[FLT_MAX], [DENORM], [DENORM]], np.float32)
    out, _, _, med = ctx.debias_host(m, np.zeros(3), 1.0)
    assert bits(med)[0, 0] == 1 and np.isinf(out[0, 0])
    # the largest cell over the smallest median stays finite
    out, _ = check_debias(ctx, np.array([[2 ** 63 - 1], [1], [1]], np.int64), np.zeros(3), 1.0)
    assert out[0, 0] == np.float32(2.0 ** 63)


def test_debias_refusals_leave_the_host_outputs_and_the_context(ctx):
    good = cell_matrix(91, 6, 4)
    vals = np.array([0.1, 0.5, 0.1, 0.9, 0.5, 0.1])

    def fine():
        check_debias(ctx, good, vals, 0.1)

    def untouched(cor, nc, med):
        return (cor == 0xffffffff).all() and nc == 2 ** 63 and np.isnan(med).all()

    for shape, at in (((6, 4), (0, 0)), ((6, 4), (5, 3)), ((1, 1), (0, 0)), ((SWEEP + 3, 2), (SWEEP + 2, 1))):
        cells = np.full(shape, 7, np.int64)
        cells[at] = -1
        p, q = ctx.upload(cells), ctx.alloc(cells.size * 4)
        try:
            rc, cor, nc, med = ctx.debias_cells(p, q, shape[0], shape[1], np.zeros(shape[0]), 0.1)
            assert rc == E_INVALID and b"negative" in ctx.err() and untouched(cor, nc, med), (shape, at)
        finally:
            ctx.free(p, q)
        fine()
    p = ctx.upload(good)
    q = ctx.alloc(good.size * 4)
    try:
        last = p.value + good.nbytes - 1
        for out in (p.value, last, p.value - good.size * 4 + 1, p.value + 8):
            rc, cor, nc, med = ctx.debias_cells(p, C.c_void_p(out), 6, 4, vals, 0.1)
            assert rc == E_INVALID and b"overlap" in ctx.err() and untouched(cor, nc, med), out - p.value
        assert np.array_equal(ctx.read(p, good.shape, np.int64), good)
        fine()
        # gd_chunk_debias's own refusals
        for rows, n in ((6, 0), (6, 4097), (0, 4), (2 ** 31, 4)):
            assert ctx.debias_cells(p, q, rows, n, vals, 0.1)[0] == E_RANGE, (rows, n)
        for w in (0.0, -0.01, np.nan, np.inf):
            assert ctx.debias_cells(p, q, 6, 4, vals, w)[0] == E_INVALID and b"window" in ctx.err()
        v = vals.copy()
        v[4] = np.nan
        assert ctx.debias_cells(p, q, 6, 4, v, 0.1)[0] == E_INVALID and b"row 4" in ctx.err()
        assert ctx.debias_cells(None, q, 6, 4, vals, 0.1)[0] == E_INVALID
        assert ctx.debias_cells(p, None, 6, 4, vals, 0.1)[0] == E_INVALID
        rc, _, nc, _ = ctx.debias_cells(p, q, 6, 4, vals, 0.1, med_rows=2)               # three chunks
        assert rc == -8 and nc == 3
        fine()
        # the timing is this call's: three small tables up, the medians back
        ctx.ok(ctx.debias_cells(p, q, 6, 4, vals, 0.1)[0])
        t = (C.c_double * 7)()
        ctx.ok(ctx.lib.gd_chunk_debias_timing(ctx.h, t, 7))
        assert t[4] == 3 and t[5] == 3 and t[2] > 0 and all(x >= 0 for x in t)
    finally:
        ctx.free(p, q)


# ------------------------------------------------------------------------------------------------- the check kernel

def through(ctx, entry, d, p):
    """(rc, whether every host output is as it was primed) of one *_device entry on the device matrix p of d's shape"""
    rows, n = d.shape
    if entry == "medians":
        rc, (med, nz) = ctx.medians(d, p)
        return rc, np.isnan(med).all() and (nz == 2 ** 64 - 1).all()
    if entry == "emdepth":
        rc, out = ctx.emdepth(d, p)
        return rc, np.isnan(out[0]).all() and (out[1] == 255).all() and (out[2] == 255).all() and np.isnan(out[3]).all()
    cn = np.full(d.shape, 255, np.uint8)
    rc = ctx.add(d, np.arange(rows, dtype=np.uint32) * 1000, np.arange(1, rows + 1, dtype=np.uint32) * 1000, cn, p)
    return rc, (cn == 255).all()


@pytest.mark.parametrize("entry", ("medians", "emdepth", "emcnv"))
def test_the_check_names_the_cell(ctx, entry):
    rows, n = 6, 65
    good = ES.integer_rows(5, rows, n).astype(np.float32) + 1
    if entry == "emcnv":
        ctx.ok(ctx.lib.gd_emcnv_begin(ctx.h, n))
    for bad in (np.float32(np.nan), np.float32(np.inf), np.float32(-1.0), -DENORM):
        for r, s in ((0, 0), (rows - 1, n - 1), (2, 64)):
            d = good.copy()
            d[r, s] = bad
            p = ctx.upload(d)
            try:
                rc, untouched = through(ctx, entry, d, p)
                assert rc == E_INVALID and untouched, (bad, r, s)
                assert b"row %d, sample %d is not" % (r, s) in ctx.err(), ctx.err()
                assert np.array_equal(bits(ctx.read(p, d.shape, np.float32)), bits(d))
            finally:
                ctx.free(p)
    # the first of two is named, whichever workgroup finds it
    d = good.copy()
    d[5, 3] = d[1, 64] = np.nan
    p = ctx.upload(d)
    try:
        assert through(ctx, entry, d, p)[0] == E_INVALID and b"row 1, sample 64" in ctx.err()
    finally:
        ctx.free(p)
    # what the host lets pass passes: -0.0, a denormal, FLT_MAX
    d = good.copy()
    d[0, 0], d[2, 64], d[rows - 1, n - 1], d[3, 1] = -0.0, DENORM, FLT_MAX, 0.0
    p = ctx.upload(d)
    try:
        rc, untouched = through(ctx, entry, d, p)
        ctx.ok(rc)
        assert not untouched
    finally:
        ctx.free(p)
    if entry == "emcnv":
        ctx.ok(ctx.lib.gd_emcnv_end(ctx.h))


def test_a_refused_block_leaves_the_calls_of_the_others(ctx):
    case = CS.cases()["psize"]
    d, st, en = case.depths, case.starts, case.ends
    want = ctx.cnvs(d, st, en, (11,))
    bad = d[11:].copy()
    bad[3, 2] = np.nan
    p, pb = ctx.upload(d), ctx.upload(bad)
    try:
        ctx.ok(ctx.lib.gd_emcnv_begin(ctx.h, d.shape[1]))
        cn = np.full(d.shape, 255, np.uint8)
        ctx.ok(ctx.add(d[:11], st[:11], en[:11], cn[:11], p))
        assert ctx.add(bad, st[11:], en[11:], cn[11:], pb) == E_INVALID and b"row 3, sample 2" in ctx.err()
        assert (cn[11:] == 255).all()
        ctx.ok(ctx.add(d[11:], st[11:], en[11:], cn[11:], C.c_void_p(p.value + 11 * d.shape[1] * 4)))
        got = ctx.calls()
        got["site_cn"] = cn
    finally:
        ctx.free(p, pb)
    assert len(got["sample"]) > 0 and all(got[k].tobytes() == want[k].tobytes() for k in want)


# -------------------------------------------------------------------------------------------------------- the scale

def scale_matrix(seed, rows, n):
    """(matrix, factors): random bit patterns of non-negative finite floats; products that are denormal, that underflow
    to zero and that overflow to inf among them"""
    rng = np.random.default_rng(seed)
    m = rng.integers(0, 0x7f800000, size=(rows, n), dtype=np.int64).astype(np.uint32).view(np.float32).copy()
    f = rng.integers(0, 0x7f800000, size=n, dtype=np.int64).astype(np.uint32).view(np.float32).copy()
    f[::3] = rng.uniform(0.5, 2.0, size=len(f[::3])).astype(np.float32)
    m[0, 0], f[0] = np.float32(1e-30), np.float32(1e-10)         # a denormal product
    if n > 1:
        m[rows - 1, n - 1], f[n - 1] = FLT_MAX, np.float32(2.0)  # inf
    if n > 2:
        m[0, 1], f[1] = DENORM, np.float32(0.25)                 # rounds to zero
    return m, f


@pytest.mark.parametrize("n", (1, 63, 64, 65, 129))
def test_scale_gives_numpys_float32_product(ctx, n):
    for rows in (1, 5, 65, ROWS_IN_FLIGHT * SWEEP + 5 if n == 1 else SWEEP + 5 if n == 65 else 2):
        m, f = scale_matrix(10 * n + rows, rows, n)
        with np.errstate(over="ignore", under="ignore"):
            want = m * f[None, :]
        assert want.dtype == np.float32
        if rows == 5:
            assert (np.isinf(want).any() or n == 1) and ((want != 0) & (np.abs(want) < np.finfo(np.float32).tiny)).any()
        p = ctx.upload(m)
        try:
            ctx.ok(ctx.lib.gd_device_scale(ctx.h, p, rows, n, f.ctypes.data))
            got = ctx.read(p, m.shape, np.float32)
        finally:
            ctx.free(p)
        assert np.array_equal(bits(got), bits(want)), (rows, n)


def test_scale_refusals_leave_the_matrix(ctx):
    m, f = scale_matrix(3, 5, 65)
    p = ctx.upload(m)
    try:
        for bad in (np.nan, -0.5, np.inf, -np.inf, -DENORM):
            for s in (0, 64):
                g = f.copy()
                g[s] = bad
                assert ctx.lib.gd_device_scale(ctx.h, p, 5, 65, g.ctypes.data) == E_INVALID
                assert b"sample %d" % s in ctx.err()
        for n in (0, -1, 4097):
            assert ctx.lib.gd_device_scale(ctx.h, p, 5, n, f.ctypes.data) == E_RANGE
        assert ctx.lib.gd_device_scale(ctx.h, p, 5, 65, None) == E_INVALID
        assert ctx.lib.gd_device_scale(ctx.h, None, 5, 65, f.ctypes.data) == E_INVALID
        ctx.ok(ctx.lib.gd_device_scale(ctx.h, None, 0, 65, f.ctypes.data))
        assert np.array_equal(bits(ctx.read(p, m.shape, np.float32)), bits(m))
        g = f.copy()
        g[0] = -0.0                                              # (>= 0, as the host's checks have it)
        ctx.ok(ctx.lib.gd_device_scale(ctx.h, p, 5, 65, g.ctypes.data))
    finally:
        ctx.free(p)


# ------------------------------------------------------------------------------------- device twins equal host twins

TWIN_SAMPLES = (1, 3, 64, 65)


@pytest.mark.parametrize("n", TWIN_SAMPLES)
def test_medians_and_emdepth_twins_give_the_hosts_bytes(ctx, n):
    for name in ("int_n%d" % n, "float_n%d" % n):
        d = ES.cases()[name].depths
        p = ctx.upload(d)
        try:
            rc_h, host = ctx.emdepth(d)
            rc_d, dev = ctx.emdepth(d, p)
            assert rc_h == 0 and rc_d == 0, ctx.err()
            assert same_bytes(dev, host), name
            assert not np.isnan(dev[0]).all()
            rc_h, host = ctx.medians(d)
            rc_d, dev = ctx.medians(d, p)
            assert rc_h == 0 and rc_d == 0, ctx.err()
            assert same_bytes(dev, host), name
            assert np.array_equal(bits(dev[0]), bits(SR.sample_medians(d)[0]))
            assert np.array_equal(bits(ctx.read(p, d.shape, np.float32)), bits(d))       # read only
        finally:
            ctx.free(p)


@pytest.mark.parametrize("name", ("one_sample", "random_n3", "random_n64", "random_n65"))
def test_emcnv_twin_gives_the_hosts_bytes(ctx, name):
    case = CS.cases()[name]
    d, st, en = case.depths, case.starts, case.ends
    rows = d.shape[0]
    assert d.shape[1] in TWIN_SAMPLES
    p = ctx.upload(d)
    try:
        whole = ctx.cnvs(d, st, en, ())
        assert len(whole["sample"]) > 0
        for cuts in ((), (1,), tuple(range(1, rows))):           # the whole matrix, a cut at 1 row, a cut at every row
            got = ctx.cnvs(d, st, en, cuts, p)
            assert all(got[k].tobytes() == whole[k].tobytes() for k in whole), cuts
    finally:
        ctx.free(p)


def test_twins_refuse_the_ranges_their_hosts_refuse(ctx):
    d = np.ones((3, 4097), np.float32)
    p = ctx.upload(d)
    try:
        for n in (2, 4097, 0, -1):
            view = np.ones((3, max(n, 1)), np.float32)
            out = ctx.em_outputs(3, max(n, 1))
            rc_h = ctx.lib.gd_emdepth(ctx.h, view.ctypes.data, 3, n, *[o.ctypes.data for o in out])
            rc_d = ctx.lib.gd_emdepth_device(ctx.h, p, 3, n, *[o.ctypes.data for o in out])
            assert rc_h == rc_d == E_RANGE, n
            assert np.isnan(out[0]).all()
        med, nz = np.empty(4097, np.float32), np.empty(4097, np.uint64)
        for rows, n in ((3, 0), (3, 4097), (0, 5), (2 ** 31, 5)):
            rc_h = ctx.lib.gd_sample_medians(ctx.h, d.ctypes.data, rows, n, med.ctypes.data, nz.ctypes.data)
            rc_d = ctx.lib.gd_sample_medians_device(ctx.h, p, rows, n, med.ctypes.data, nz.ctypes.data)
            assert rc_h == rc_d == E_RANGE, (rows, n)
        ctx.ok(ctx.lib.gd_sample_medians_device(ctx.h, p, 3, 2, med.ctypes.data, nz.ctypes.data))       # (two samples have medians)
        # no rows: nothing runs, nothing is written
        out = ctx.em_outputs(1, 9)
        ctx.ok(ctx.lib.gd_emdepth_device(ctx.h, None, 0, 9, *[o.ctypes.data for o in out]))
        assert np.isnan(out[0]).all()
        assert ctx.lib.gd_emdepth_device(ctx.h, None, 3, 9, *[o.ctypes.data for o in out]) == E_INVALID
        # the emcnv state rules
        st = np.arange(3, dtype=np.uint32)
        assert ctx.lib.gd_emcnv_add_device(ctx.h, p, 3, st.ctypes.data, st.ctypes.data, None) == -4      # no begin
        ctx.ok(ctx.lib.gd_emcnv_begin(ctx.h, 5))
        ctx.ok(ctx.lib.gd_emcnv_add_device(ctx.h, None, 0, None, None, None))
        assert ctx.lib.gd_emcnv_add_device(ctx.h, p, 3, None, st.ctypes.data, None) == E_INVALID
        ctx.ok(ctx.lib.gd_emcnv_finish(ctx.h, None, None))
        assert ctx.lib.gd_emcnv_add_device(ctx.h, p, 3, st.ctypes.data, st.ctypes.data, None) == -4      # after finish
        ctx.ok(ctx.lib.gd_emcnv_end(ctx.h))
    finally:
        ctx.free(p)


# -------------------------------------------------------------------------------------------------- the composed path

RUNS = ((9, 12, 4, 3), (28, 32, 6, 4), (21, 24, 1, 0), (1, 3, 3, 3))      # (first row, row after the last, sample, copy number)


def planted():
    """The construction of tests/test_gpu_debias_cli.py -- 40 x 9 integer cells, a level and a GC slope per sample, 3 % noise,
    its eight planted one-row CNVs -- with four CNVs of two to four rows planted besides: a call needs a member, and a
    member a row above it in the same state.  (cells, truth, starts, ends)"""
    from tests import test_gpu_debias_cli as DC
    truth = DC.truth()
    for r0, r1, s, c in RUNS:
        assert (truth[r0:r1, s] == 2).all()
        truth[r0:r1, s] = c
    rng = np.random.default_rng(7)
    t = (np.array([DC.GC_LEVELS[r % 5] for r in range(DC.ROWS)]) - 0.45) / 0.15
    bias = 1.0 + np.outer(t, DC.SLOPES)
    noise = 1.0 + rng.uniform(-0.03, 0.03, (DC.ROWS, DC.N))
    cells = np.floor(60.0 * np.array(DC.LEVELS) * bias * noise * truth / 2.0).astype(np.int64)
    assert cells.min() >= 0 and cells.max() < 2 ** 24
    st = np.array([(i % 25) * 1000 for i in range(DC.ROWS)], np.uint32)
    return DC, cells, truth, st, st + np.uint32(1000)


@functools.lru_cache(maxsize=None)
def chained(level, with_vals):
    """(factors, level, emcnv_ref result): debias_ref -> scales_ref -> emcnv_ref on the CPU, held -- before any device
    call -- to what tests/test_gpu_debias_cli.py holds its matrix to: after the debiasing the restatement alone finds
    exactly the planted CNVs, no cell sits on an adjustCN margin, every row's comparisons are wider than 1e-9 relative;
    and no cell is within 1e-9 of a state threshold of emdepth.Cache"""
    DC, cells, truth, st, en = planted()
    m = cells.astype(np.float32)
    med_read, nz = SR.sample_medians(m)
    assert (nz > 0).all()
    T = SR.level_of(med_read) if level is None else float(level)
    if with_vals:
        _, m, cor, C_, _ = DR.debias(m, DC.vals(), DC.WINDOW)
        assert C_ == 5 and np.bincount(cor).tolist() == [8] * 5 and np.isfinite(m).all()
        f = SR.scales(SR.sample_medians(m)[0], T)
    else:
        f = SR.scales(med_read, T)
    depths = (m * f[None, :]).astype(np.float32)
    rows = R.em_matrix(depths)
    cn = DC.held(rows)                           # asserts: no pair excluded, every gap above 1e-9
    if with_vals:
        assert np.array_equal(cn, truth)
    else:
        assert (cn != truth).any()               # (undebiased, the copy numbers follow the covariate)
    res = CR.run(depths, st, en, rows)
    assert res.near == []
    return f, T, res


def compare_calls(got, res):
    """cohort_cnvs' third value against the restatement: cn exactly, and every call's sample, emit row, psize, member
    rows and member cn exactly; nothing is left out"""
    want = CS.flatten(res.cnvs)
    assert np.array_equal(got["site_cn"], np.array([r.cn for r in res.rows], np.uint8))
    for k in ("sample", "emit_row", "psize", "member_off", "member_row", "cn"):
        assert np.array_equal(got[k], want[k]), k
    assert got["depth"].tobytes() == want["depth"].tobytes()


LEVELS = (60.0, None, 45.0)


def engine_upload(eng, a):
    p = eng.device_alloc(a.nbytes)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert hip.hipMemcpy(p, a.ctypes.data, a.nbytes, 1) == 0     # hipMemcpyHostToDevice
    return p


@pytest.fixture(scope="module")
def cohort40():
    from goleft_amd.engine import DepthEngine
    DC, cells, _, st, en = planted()
    for level in LEVELS:                         # the preconditions, on the CPU, before the device runs
        for with_vals in (True, False):
            chained(level, with_vals)
    with DepthEngine(0) as eng:
        p = engine_upload(eng, cells)
        yield DC, cells, st, en, eng, p
        eng.device_free(p)


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("with_vals", (True, False))
def test_cohort_cnvs_is_the_restatements_chained(cohort40, level, with_vals):
    from goleft_amd import emdepth
    DC, cells, st, en, eng, p = cohort40
    f, T, res = chained(level, with_vals)
    if with_vals:                                # the planted runs, less the member a run's first row is not
        assert [(c.sample, c.rows) for c in res.cnvs] == [(1, [22, 23]), (3, [2]), (4, [10, 11]), (6, [29, 30, 31])]
    for block in (None, 7):
        gf, gT, got = emdepth.cohort_cnvs(eng, p, DC.ROWS, DC.N, st, en, vals=DC.vals() if with_vals else None,
                                          window=DC.WINDOW, level=level, block_rows=block, site_cn=True)
        assert gT == T and np.array_equal(bits(gf), bits(f))
        compare_calls(got, res)
    # without site_cn the calls are the same and no matrix comes back
    got = emdepth.cohort_cnvs(eng, p, DC.ROWS, DC.N, st, en, vals=DC.vals() if with_vals else None, level=level)[2]
    assert got["site_cn"] is None and np.array_equal(got["member_row"], CS.flatten(res.cnvs)["member_row"])


def cli_calls(text):
    """(sample index, number of sites) of every line of a --cnvs file"""
    lines = text.split("\n")
    assert lines[0].startswith("#sample\t") and lines[-1] == ""
    return [(int(f[1]), int(f[3])) for f in (ln.split("\t") for ln in lines[1:-1])]


@pytest.mark.parametrize("with_vals", (True, False))
def test_cohort_cnvs_is_the_command_lines(cohort40, with_vals, tmp_path):
    from goleft_amd import emdepth
    DC, cells, st, en, eng, p = cohort40
    plain, gc, calls = tmp_path / "m.bed", tmp_path / "gc.txt", tmp_path / "calls.tsv"
    plain.write_text(DC.matrix_text(cells))
    gc.write_text("".join("%r\n" % float(v) for v in DC.vals()))
    args = (["--gc-values", str(gc)] if with_vals else ["--normalize"]) + ["--level", "%g" % DC.LEVEL, "--cnvs", str(calls), str(plain)]
    run = subprocess.run([DC.EXE, "emdepth"] + args, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    _, _, got = emdepth.cohort_cnvs(eng, p, DC.ROWS, DC.N, st, en, vals=DC.vals() if with_vals else None, window=DC.WINDOW,
                                    level=DC.LEVEL, site_cn=True)
    assert run.stdout == DC.matrix_text(got["site_cn"])
    mine = list(zip(got["sample"].tolist(), np.diff(got["member_off"]).astype(np.int64).tolist()))
    assert len(mine) > 0 and cli_calls(calls.read_text()) == mine


def test_cohort_cnvs_names_the_sample_it_cannot_scale(cohort40):
    from goleft_amd import emdepth
    from goleft_amd.engine import GdError
    DC, cells, st, en, eng, p = cohort40
    empty = cells.copy()
    empty[:, 4] = 0
    q = engine_upload(eng, empty)
    try:
        for vals, level in ((DC.vals(), None), (DC.vals(), 60.0), (None, None), (None, 60.0)):
            with pytest.raises(ValueError, match="sample 4 "):
                emdepth.cohort_cnvs(eng, q, DC.ROWS, DC.N, st, en, vals=vals, level=level)
    finally:
        eng.device_free(q)
    with pytest.raises(ValueError, match="sample 0.*not finite"):                        # 1e300 over a median near 1
        emdepth.cohort_cnvs(eng, p, DC.ROWS, DC.N, st, en, vals=DC.vals(), level=1e300)
    for level in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError, match="level"):
            emdepth.cohort_cnvs(eng, p, DC.ROWS, DC.N, st, en, level=level)
    with pytest.raises(GdError):
        emdepth.cohort_cnvs(eng, p, DC.ROWS, DC.N, st, en, vals=DC.vals(), window=0.0)
    # the engine goes on
    assert len(emdepth.cohort_cnvs(eng, p, DC.ROWS, DC.N, st, en, vals=DC.vals(), level=60.0)[2]["sample"]) > 0


# ----------------------------------------------------------------------------------------------------------- end to end

@pytest.mark.parametrize("n_samples", ES.COHORT_SAMPLES)
def test_records_to_calls_without_the_matrix_leaving_the_device(n_samples):
    """BAM records -> window sums -> gd_depthwed_device -> cohort_cnvs on the device pointer, against the same chain on the
    matrix read back through gd_depthwed and the host-matrix entry points."""
    from goleft_amd import emdepth
    from goleft_amd.engine import DepthEngine
    sums, cells = ES.cohort(n_samples)
    case = CS.cases()["cohort_n%d" % n_samples]
    n_ref = len(ES.COHORT_LENGTHS)
    rng = np.random.default_rng(n_samples)
    tids = np.arange(n_samples * n_ref, dtype=np.int32).reshape(n_samples, n_ref)
    vals = np.round(np.random.default_rng(40 + n_samples).normal(0.41, 0.05, cells.shape[0]), 2)
    with DepthEngine(0) as eng:
        eng.set_params(window_size=ES.COHORT_W, min_mapq=1, min_cov=4)
        eng.set_contigs([ES.COHORT_LENGTHS[j] for s in range(n_samples) for j in range(n_ref)])
        for s in range(n_samples):
            for j in range(n_ref):
                r = H.window_sum_reads(rng, ES.COHORT_LENGTHS[j], ES.COHORT_W, sums[s][j])
                eng.push(int(tids[s, j]), r.pos, r.flag, r.mapq, r.cigar_off, r.cigar)
        eng.compute()
        back = eng.depthwed(tids, ES.COHORT_W)[0]
        assert np.array_equal(back, cells)
        ptr, rows = eng.depthwed_device(tids, ES.COHORT_W)
        assert rows == cells.shape[0]
        for with_vals in (True, False):
            for level in (None, 50.0):
                # the host-matrix route, as the command line takes it
                m = back.astype(np.float32)
                T = float(sorted(eng.sample_medians(m)[0].tolist())[n_samples // 2]) if level is None else level
                if with_vals:
                    m = eng.chunk_debias(m, vals, 0.03)[0]
                f = emdepth.scales(eng.sample_medians(m)[0], T)
                want = eng.emdepth_cnvs(m * f[None, :], case.starts, case.ends)
                gf, gT, got = emdepth.cohort_cnvs(eng, ptr, rows, n_samples, case.starts, case.ends,
                                                  vals=vals if with_vals else None, window=0.03, level=level, block_rows=7,
                                                  site_cn=True)
                assert gT == T and np.array_equal(bits(gf), bits(f))
                want.pop("timing"), got.pop("timing")
                assert all(got[k].tobytes() == want[k].tobytes() for k in want), (with_vals, level)
        assert np.array_equal(eng.depthwed(tids, ES.COHORT_W)[0], cells)                 # the cells were only read
