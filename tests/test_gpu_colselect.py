"""GPU: gd_sample_medians / gd_sample_medians_cells (goleft_amd/csrc/gd_colselect.hpp) through the C ABI against the
restatement of dcnv's SampleMedians (tests/scales_ref.py).  Every compared value is bit for bit: the medians as their bit
patterns, the non-zero counts as integers; nothing is left out and there is no tolerance.  Both element kinds run every
shape.

The shapes follow the kernel's mapping: 64 columns a workgroup (one per lane), 8 waves x 8 rows a
slab, at most 512 workgroups a launch shared evenly by the column tiles, 8-bit digits from the top; int64 columns start with a
pass over the cells' lengths in bytes."""
import ctypes as C
import functools

import numpy as np
import pytest

from goleft_amd import _lib
from tests import emdepth_shapes as ES
from tests import helpers as H
from tests import scales_ref as SR

pytestmark = pytest.mark.gpu

E_INVALID, E_RANGE = -1, -5
COLS = 64                # columns of a workgroup (CS_COLS)
SLAB = 64                # rows of a workgroup's turn (CS_SLAB = CS_WAVES * CS_ROWS)
GRID = 512               # workgroups of a launch (CS_MAX_GRID), shared evenly by the column tiles
SAMPLE_COUNTS = (1, 63, 64, 65, 129)
ROW_COUNTS = (1, 2, 3, SLAB - 1, SLAB, SLAB + 1)
STRIDE_ROWS = GRID * SLAB + 1                    # one more than a full grid of one column tile covers in one sweep
FLT_MAX = np.finfo(np.float32).max
DENORM = np.float32(1e-45)                       # the smallest denormal, bits 1


class Ctx:
    def __init__(self):
        self.lib = _lib.load()
        self.h = C.c_void_p()
        assert self.lib.gd_create(0, C.byref(self.h)) == 0
        self.hip = C.CDLL("libamdhip64.so")
        self.hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]

    def ok(self, rc):
        assert rc == 0, self.lib.gd_last_error(self.h).decode()

    def close(self):
        self.lib.gd_destroy(self.h)

    def run(self, depths, rows=None, n=None, count=True):
        d = np.ascontiguousarray(depths, np.float32)
        rows, n = (d.shape[0] if rows is None else rows), (d.shape[1] if n is None else n)
        med = np.full(max(n, 1), np.nan, np.float32)
        nz = np.full(max(n, 1), 2 ** 64 - 1, np.uint64)
        rc = self.lib.gd_sample_medians(self.h, d.ctypes.data, rows, n, med.ctypes.data, nz.ctypes.data if count else None)
        return rc, med, nz

    def upload(self, cells):
        cells = np.ascontiguousarray(cells, np.int64)
        p = C.c_void_p()
        self.ok(self.lib.gd_device_alloc(self.h, cells.nbytes, C.byref(p)))
        assert self.hip.hipMemcpy(p, cells.ctypes.data, cells.nbytes, 1) == 0           # hipMemcpyHostToDevice
        return p

    def run_cells(self, cells, rows=None, n=None):
        cells = np.ascontiguousarray(cells, np.int64)
        rows, n = (cells.shape[0] if rows is None else rows), (cells.shape[1] if n is None else n)
        med = np.full(max(n, 1), -7, np.int64)
        nz = np.full(max(n, 1), 2 ** 64 - 1, np.uint64)
        p = self.upload(cells)
        try:
            rc = self.lib.gd_sample_medians_cells(self.h, p, rows, n, med.ctypes.data, nz.ctypes.data)
        finally:
            self.ok(self.lib.gd_device_free(self.h, p))
        return rc, med, nz


@pytest.fixture(scope="module")
def ctx():
    c = Ctx()
    yield c
    c.close()


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


def int_matrix(seed, rows, n):
    """non-negative int64 of every length in bytes, mixed within a column, a quarter zero"""
    rng = np.random.default_rng(seed)
    m = rng.integers(0, 2 ** 63, size=(rows, n), dtype=np.int64) >> rng.integers(0, 64, size=(rows, n), dtype=np.int64)
    m[rng.random((rows, n)) < 0.25] = 0
    return m


def check_float(ctx, m):
    want, want_nz = SR.sample_medians(m)
    rc, med, nz = ctx.run(m)
    ctx.ok(rc)
    assert np.array_equal(med.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(nz, want_nz)


def check_cells(ctx, m):
    want, want_nz = SR.sample_medians(m)
    rc, med, nz = ctx.run_cells(m)
    ctx.ok(rc)
    assert np.array_equal(med, want)
    assert np.array_equal(nz, want_nz)


@pytest.mark.parametrize("n", SAMPLE_COUNTS)
def test_sample_counts(ctx, n):
    check_float(ctx, float_matrix(10 + n, 70, n))
    check_float(ctx, depth_matrix(20 + n, 70, n))
    check_cells(ctx, int_matrix(30 + n, 70, n))
    check_cells(ctx, depth_matrix(40 + n, 70, n).astype(np.int64))


def test_the_widest_matrix(ctx):
    check_float(ctx, float_matrix(50, 3, 4096))
    check_cells(ctx, int_matrix(51, 3, 4096))


@pytest.mark.parametrize("rows", ROW_COUNTS)
def test_row_counts_around_a_slab(ctx, rows):
    check_float(ctx, float_matrix(60 + rows, rows, 9))
    check_float(ctx, depth_matrix(61 + rows, rows, 9))
    check_cells(ctx, int_matrix(62 + rows, rows, 9))


def test_the_stride_loop_turns(ctx):
    check_float(ctx, depth_matrix(70, STRIDE_ROWS, 3))
    check_float(ctx, float_matrix(71, STRIDE_ROWS, 3))
    check_cells(ctx, int_matrix(72, STRIDE_ROWS, 3))
    # ... and with two column tiles, which share the grid (256 workgroups each)
    check_float(ctx, depth_matrix(73, STRIDE_ROWS // 2 + 1, 65))
    check_cells(ctx, depth_matrix(74, STRIDE_ROWS // 2 + 1, 65).astype(np.int64))


ROWS = 41


def columns_to_matrix(cols, dtype):
    m = np.zeros((ROWS, len(cols)), dtype)
    for s, col in enumerate(cols):
        col = np.array(col, dtype)
        assert len(col) <= ROWS
        m[:len(col), s] = col
    return m


@functools.lru_cache(maxsize=None)
def float_columns():
    """columns in which one pass after the other decides, beside an all-zero one"""
    bits = lambda a: np.array(a, np.uint32).view(np.float32)
    rng = np.random.default_rng(80)
    base = np.float32(37.5).view(np.uint32)
    return [
        bits(base & ~np.uint32(0xff) | rng.permutation(ROWS).astype(np.uint32)),          # equal but in the lowest byte
        bits((rng.permutation(ROWS).astype(np.uint32) + 2) << 24 | np.uint32(0x123456)),   # ... in the highest byte
        bits(rng.permutation(ROWS).astype(np.uint32) * 3 + 1),                             # denormals only
        [0, DENORM, 0],                                                                    # the smallest denormal among zeros
        [FLT_MAX] * 5 + [1.0] * 3,                                                         # n = 8: sorted[k + 5] = FLT_MAX
        [FLT_MAX, FLT_MAX, np.nextafter(FLT_MAX, np.float32(0))] * 4,
        [0.0] * ROWS,                                                                      # all zero: 0 and 0
        [-0.0] * 20 + [3.0, 1.0, 2.0],                                                     # -0.0 is a zero: n = 3, sorted[k + 1] = 2
        [-0.0, 5.0],
        [7.0] * ROWS,
        bits(base & ~np.uint32(0xff00) | (rng.permutation(ROWS).astype(np.uint32) << 8)),  # ... in the second byte
        bits(base & ~np.uint32(0xff0000) | (rng.permutation(ROWS).astype(np.uint32) << 16)),
    ]


@functools.lru_cache(maxsize=None)
def int_columns():
    rng = np.random.default_rng(81)
    perm = lambda: rng.permutation(ROWS).astype(np.int64)
    return [
        (0x1234567890 << 8) | perm(),                                     # equal but in the lowest byte
        ((perm() + 1) << 40) | 0x55aa55aa55,                              # ... in the highest used byte (six bytes)
        ((perm() + 1) << 56) | 0x11223344556677,                          # ... in the top byte of an int64
        2 ** 32 + perm() * 1000003,                                       # values >= 2^32
        [2 ** 53, 2 ** 53 + 1],                                           # n = 2: sorted[k + 1] = 2^53 + 1
        [2 ** 53 + 1, 2 ** 53, 2 ** 53],                                  # n = 3: sorted[k + 1] = 2^53
        [2 ** 63 - 1] * 3 + [2 ** 63 - 2] * 2,
        [0] * ROWS,                                                       # all zero: 0 and 0
        [1] + [0] * 30,                                                   # one byte while its neighbours need eight
        perm() + 250,                                                     # straddles the one-byte / two-byte lengths
        [255, 256, 255, 256, 256],
        (perm() << 16) | 0xabcd,
    ]


def test_float_columns_built_for_each_pass(ctx):
    m = columns_to_matrix(float_columns(), np.float32)
    assert np.signbit(m).any() and (m == FLT_MAX).any()
    want, want_nz = SR.sample_medians(m)
    assert want[6] == 0 and want_nz[6] == 0 and want[7] == 2 and want_nz[7] == 3 and want[4] == FLT_MAX
    assert want[3] == DENORM and want_nz[3] == 1 and want[8] == 5
    check_float(ctx, m)
    for s in range(m.shape[1]):                  # each alone too: one column tile, one live lane
        check_float(ctx, m[:, s:s + 1])


def test_int64_columns_built_for_each_pass(ctx):
    m = columns_to_matrix(int_columns(), np.int64)
    want, want_nz = SR.sample_medians(m)
    assert want[4] == 2 ** 53 + 1 and want[5] == 2 ** 53 and want[6] == 2 ** 63 - 1 and want[7] == 0 and want_nz[7] == 0
    assert want[8] == 1 and want[3] >= 2 ** 32
    check_cells(ctx, m)
    for s in range(m.shape[1]):
        check_cells(ctx, m[:, s:s + 1])
    # small answers only: the leading digit passes are not run, and the answers do not change
    small = m[:, [8, 9, 10]]
    check_cells(ctx, small)
    t = (C.c_double * 4)()
    ctx.ok(ctx.lib.gd_sample_medians_timing(ctx.h, t, 4))
    assert t[3] == 3                             # the lengths, then two digits
    assert t[1] > 0 and t[2] > 0 and t[0] == 0


def test_counts_may_be_left_out_and_calls_repeat(ctx):
    m = depth_matrix(90, 130, 65)
    want, _ = SR.sample_medians(m)
    for _ in range(2):
        rc, med, nz = ctx.run(m, count=False)
        ctx.ok(rc)
        assert np.array_equal(med.view(np.uint32), want.view(np.uint32)) and (nz == 2 ** 64 - 1).all()
    t = (C.c_double * 4)()
    ctx.ok(ctx.lib.gd_sample_medians_timing(ctx.h, t, 4))
    assert t[0] > 0 and t[1] > 0 and t[2] > 0 and t[3] == 4


@pytest.mark.parametrize("n_samples", ES.COHORT_SAMPLES)
def test_cells_of_a_real_depthwed(n_samples):
    """BAM records -> window sums -> gd_depthwed_device -> gd_sample_medians_cells, the matrix never leaving the device;
    then the factors, and emdepth on the same cells with them."""
    from goleft_amd import emdepth
    from goleft_amd.engine import DepthEngine
    sums, cells = ES.cohort(n_samples)
    n_ref = len(ES.COHORT_LENGTHS)
    rng = np.random.default_rng(n_samples)
    tids = np.arange(n_samples * n_ref, dtype=np.int32).reshape(n_samples, n_ref)
    want, want_nz = SR.sample_medians(cells)
    with DepthEngine(0) as eng:
        eng.set_params(window_size=ES.COHORT_W, min_mapq=1, min_cov=4)
        eng.set_contigs([ES.COHORT_LENGTHS[j] for s in range(n_samples) for j in range(n_ref)])
        for s in range(n_samples):
            for j in range(n_ref):
                r = H.window_sum_reads(rng, ES.COHORT_LENGTHS[j], ES.COHORT_W, sums[s][j])
                eng.push(int(tids[s, j]), r.pos, r.flag, r.mapq, r.cigar_off, r.cigar)
        eng.compute()
        ptr, rows = eng.depthwed_device(tids, ES.COHORT_W)
        assert rows == cells.shape[0]
        med, nz = eng.sample_medians_cells(ptr, rows, n_samples)
        assert med.dtype == np.int64 and np.array_equal(med, want) and np.array_equal(nz, want_nz)
        assert eng.sample_medians_timing()[1] > 0
        fmed, fnz = eng.sample_medians(cells.astype(np.float32))
        assert np.array_equal(fmed, want.astype(np.float32)) and np.array_equal(fnz, want_nz)
        scale = emdepth.scales(med)
        assert np.array_equal(scale.view(np.uint32), SR.scales(want).view(np.uint32))
        assert np.array_equal(emdepth.scales(med, level=1).view(np.uint32), SR.scales(want, level=1).view(np.uint32))
        # the factors are what emdepth_cells takes
        lam, it, cn, fc = eng.emdepth_cells(ptr, rows, n_samples, scale)
        assert cn.shape == (rows, n_samples)


def test_refused_inputs_leave_the_context_usable(ctx):
    good = depth_matrix(95, 70, 9)
    cells = good.astype(np.int64)

    def still_works():
        check_float(ctx, good)
        check_cells(ctx, cells)

    for n, rows in ((0, 70), (4097, 70), (9, 0), (-1, 70)):
        rc, med, nz = ctx.run(good, rows=rows, n=n)
        assert rc == E_RANGE and np.isnan(med).all() and (nz == 2 ** 64 - 1).all(), (n, rows)
        rc, med, nz = ctx.run_cells(cells, rows=rows, n=n)
        assert rc == E_RANGE and (med == -7).all(), (n, rows)
        still_works()
    assert ctx.lib.gd_sample_medians(ctx.h, good.ctypes.data, 2 ** 31, 1, None, None) == E_RANGE
    for bad in (np.nan, -1.0, np.inf, -np.inf):
        d = good.copy()
        d[3, 2] = bad
        rc, med, nz = ctx.run(d)
        assert rc == E_INVALID and np.isnan(med).all(), bad
        assert b"row 3, sample 2" in ctx.lib.gd_last_error(ctx.h)
        still_works()
    # a negative device cell cannot be seen before anything runs: the first pass finds it, and nothing is written
    c = cells.copy()
    c[5, 1] = -3
    rc, med, nz = ctx.run_cells(c)
    assert rc == E_INVALID and (med == -7).all() and (nz == 2 ** 64 - 1).all()
    assert b"negative" in ctx.lib.gd_last_error(ctx.h)
    still_works()
