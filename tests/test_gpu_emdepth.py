"""GPU: gd_emdepth / gd_emdepth_cells (goleft_amd/csrc/gd_emdepth.hpp) through the C ABI against the restatement of
emdepth.EMDepth (tests/emdepth_ref.py), on the matrices of tests/emdepth_shapes.py.

The contract:
  * exact-sum rows (integers times one power of two): lambda bit for bit, iters equal;
  * general float32 rows whose every comparison in the restatement is wider than 1e-9 relative: iters equal and
    |lambda - ref| <= 4 N 2^-53 |ref| (a sum of N non-negative terms in any order is off by at most (N - 1) 2^-53; the
    factor 4 covers the division and the fallback's products);
  * cn equal but where adjustCN compared two pmf values within 1e-9 relative or below 1e-290;
  * log2fc: infinities and NaN identical, finite values within one float32 ulp.
At most 1 % of rows and of adjusted cells are left out; tests/test_emdepth_ref.py asserts that on the CPU."""
import ctypes as C
import itertools

import numpy as np
import pytest

from goleft_amd import _lib
from tests import emdepth_shapes as S
from tests import helpers as H

pytestmark = pytest.mark.gpu

E_INVALID, E_RANGE = -1, -5


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

    def outputs(self, rows, n, want=(True, True, True, True)):
        bufs = (np.full((rows, 9), np.nan), np.full(rows, 255, np.uint8), np.full((rows, n), 255, np.uint8),
                np.full((rows, n), np.nan, np.float32))
        return [b if w else None for b, w in zip(bufs, want)]

    def run(self, depths, want=(True, True, True, True)):
        d = np.ascontiguousarray(depths, np.float32)
        rows, n = d.shape
        out = self.outputs(rows, n, want)
        rc = self.lib.gd_emdepth(self.h, d.ctypes.data, rows, n, *[o.ctypes.data if o is not None else None for o in out])
        return rc, out

    def upload(self, cells):
        cells = np.ascontiguousarray(cells, np.int64)
        p = C.c_void_p()
        self.ok(self.lib.gd_device_alloc(self.h, cells.nbytes, C.byref(p)))
        assert self.hip.hipMemcpy(p, cells.ctypes.data, cells.nbytes, 1) == 0           # hipMemcpyHostToDevice
        return p

    def run_cells(self, dptr, rows, n, scale):
        out = self.outputs(rows, n)
        s = None if scale is None else np.ascontiguousarray(scale, np.float32)
        rc = self.lib.gd_emdepth_cells(self.h, dptr, rows, n, s.ctypes.data if s is not None else None,
                                       *[o.ctypes.data for o in out])
        return rc, out


@pytest.fixture(scope="module")
def ctx():
    c = Ctx()
    yield c
    c.close()


def compare(name, got):
    """Holds one case's device results to the contract; prints the figures first."""
    case = S.cases()[name]
    ref = S.reference(name)
    keep, out, adjusted = S.plan(case, ref)
    assert S.within_caps(keep, out, adjusted), name
    lam, iters, cn, fc = got
    rows, n = case.depths.shape
    r_lam = np.array([r.lam for r in ref], np.float64)
    r_it = np.array([r.iters for r in ref], np.uint8)
    r_cn = np.array([r.cn for r in ref], np.uint8)
    r_fc = np.array([r.log2fc for r in ref], np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.where(r_lam != 0, np.abs(lam - r_lam) / np.abs(r_lam), np.abs(lam - r_lam))
    print("%s: rows %d (%d compared) n %d, lambda bits differ in %d rows, max relative lambda error %.3g, iters differ in %d rows, "
          "cn differ in %d cells (%d left out of %d adjusted)" % (
              name, rows, int(keep.sum()), n, int((lam.view(np.uint64) != r_lam.view(np.uint64)).any(1).sum()),
              float(rel[keep].max()) if keep.any() else 0.0, int((iters != r_it)[keep].sum()),
              int((cn != r_cn)[keep].sum()), len(out), adjusted))
    assert np.array_equal(iters[keep], r_it[keep])
    if case.exact:
        assert np.array_equal(lam.view(np.uint64), r_lam.view(np.uint64))
    else:
        assert np.all(np.abs(lam - r_lam)[keep] <= (4 * n * 2.0 ** -53 * np.abs(r_lam))[keep])
    mask = np.repeat(keep[:, None], n, 1)
    for i, s in out:
        mask[i, s] = False
    assert np.array_equal(cn[mask], r_cn[mask])
    a, b = fc[keep], r_fc[keep]
    assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isposinf(a), np.isposinf(b))
    assert np.array_equal(np.isneginf(a), np.isneginf(b))
    fin = np.isfinite(b)
    assert np.all(np.abs(a[fin].astype(np.float64) - b[fin].astype(np.float64)) <= np.spacing(np.abs(b[fin])).astype(np.float64))


F32 = sorted(k for k, c in S.cases().items() if c.kind == "f32")
CELLS = sorted(k for k, c in S.cases().items() if c.kind == "cells")


@pytest.mark.parametrize("name", F32)
def test_host_float32(ctx, name):
    rc, out = ctx.run(S.cases()[name].depths)
    ctx.ok(rc)
    compare(name, out)


@pytest.mark.parametrize("name", CELLS)
def test_uploaded_cells(ctx, name):
    case = S.cases()[name]
    p = ctx.upload(case.cells)
    try:
        rc, out = ctx.run_cells(p, case.cells.shape[0], case.cells.shape[1], case.scale)
        ctx.ok(rc)
        compare(name, out)
    finally:
        ctx.ok(ctx.lib.gd_device_free(ctx.h, p))


@pytest.mark.parametrize("n_samples", S.COHORT_SAMPLES)
def test_cells_of_a_real_depthwed(n_samples):
    """BAM records -> window sums -> gd_depthwed_device -> gd_emdepth_cells, the matrix never leaving the device."""
    from goleft_amd.engine import DepthEngine
    sums, cells = S.cohort(n_samples)
    n_ref = len(S.COHORT_LENGTHS)
    rng = np.random.default_rng(n_samples)
    tids = np.arange(n_samples * n_ref, dtype=np.int32).reshape(n_samples, n_ref)
    with DepthEngine(0) as eng:
        eng.set_params(window_size=S.COHORT_W, min_mapq=1, min_cov=4)
        eng.set_contigs([S.COHORT_LENGTHS[j] for s in range(n_samples) for j in range(n_ref)])
        for s in range(n_samples):
            for j in range(n_ref):
                r = H.window_sum_reads(rng, S.COHORT_LENGTHS[j], S.COHORT_W, sums[s][j])
                eng.push(int(tids[s, j]), r.pos, r.flag, r.mapq, r.cigar_off, r.cigar)
        eng.compute()
        assert np.array_equal(eng.depthwed(tids, S.COHORT_W)[0], cells)
        for name in ("cohort_n%d", "cohort_pow2_n%d", "cohort_scaled_n%d"):
            case = S.cases()[name % n_samples]
            ptr, rows = eng.depthwed_device(tids, S.COHORT_W)
            assert rows == cells.shape[0]
            compare(name % n_samples, eng.emdepth_cells(ptr, rows, n_samples, case.scale))
            assert eng.emdepth_timing()[1] > 0
        # the float32 form through the same handle
        compare("cohort_n%d" % n_samples, eng.emdepth(cells.astype(np.float32)))


def test_null_outputs_in_every_combination(ctx):
    depths = S.cases()["int_n65"].depths
    rc, full = ctx.run(depths)
    ctx.ok(rc)
    for want in itertools.product((False, True), repeat=4):
        rc, out = ctx.run(depths, want)
        ctx.ok(rc)
        for o, f in zip(out, full):
            assert o is None or o.tobytes() == f.tobytes(), want


def test_two_calls_give_identical_bytes(ctx):
    for name in ("float_n200", "float_n257"):
        a = ctx.run(S.cases()[name].depths)[1]
        b = ctx.run(S.cases()[name].depths)[1]
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_no_rows(ctx):
    out = ctx.outputs(1, 9)
    ptrs = [o.ctypes.data for o in out]
    assert ctx.lib.gd_emdepth(ctx.h, None, 0, 9, *ptrs) == 0
    assert ctx.lib.gd_emdepth_cells(ctx.h, None, 0, 9, None, *ptrs) == 0
    assert np.isnan(out[0]).all() and (out[1] == 255).all()      # nothing was written


def test_refused_inputs_leave_the_context_usable(ctx):
    good = S.cases()["int_n5"].depths
    for n in (2, 0, -1, 4097):
        d = np.ones((3, max(n, 1)), np.float32)
        out = ctx.outputs(3, max(n, 1))
        assert ctx.lib.gd_emdepth(ctx.h, d.ctypes.data, 3, n, *[o.ctypes.data for o in out]) == E_RANGE, n
        assert ctx.lib.gd_emdepth_cells(ctx.h, None, 3, n, None, *[o.ctypes.data for o in out]) == E_RANGE, n
        assert np.isnan(out[0]).all()
    assert b"2 samples" in ctx.lib.gd_last_error(ctx.h) or b"4096" in ctx.lib.gd_last_error(ctx.h)
    for bad in (np.nan, -1.0, np.inf, -np.inf):
        d = good.copy()
        d[3, 2] = bad
        rc, out = ctx.run(d)
        assert rc == E_INVALID and np.isnan(out[0]).all(), bad
        assert b"row 3, sample 2" in ctx.lib.gd_last_error(ctx.h)
    case = S.cases()["cells_n5"]
    p = ctx.upload(case.cells)
    try:
        for bad in (np.nan, -0.5, np.inf):
            scale = np.ones(5, np.float32)
            scale[4] = bad
            rc, out = ctx.run_cells(p, case.cells.shape[0], 5, scale)
            assert rc == E_INVALID and np.isnan(out[0]).all(), bad
        rc, out = ctx.run_cells(p, case.cells.shape[0], 5, None)
        ctx.ok(rc)
        compare("cells_n5", out)
    finally:
        ctx.ok(ctx.lib.gd_device_free(ctx.h, p))
    rc, out = ctx.run(good)
    ctx.ok(rc)
    compare("int_n5", out)


def test_timing_reports_the_last_call(ctx):
    rc, _ = ctx.run(S.cases()["int_n200"].depths)
    ctx.ok(rc)
    t = (C.c_double * 3)()
    ctx.ok(ctx.lib.gd_emdepth_timing(ctx.h, t, 3))
    assert t[0] > 0 and t[1] > 0 and t[2] > 0
