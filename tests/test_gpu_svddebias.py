"""GPU: gd_svd_debias, gd_svd_debias_cells and gd_svd_debias_device (goleft_amd/csrc/gd_svddebias.hpp,
gd_api_svddebias.inc) through the C ABI against the numpy float64 oracle (tests/svddebias_ref.py) on the cases of
tests/svddebias_shapes.py, whose cut tests/test_svddebias_ref.py shows to be unambiguous.

Per cell, none left out: n_removed is the oracle's, then |out - ref| <= 2^-24 |ref| + 2^-36 max_j |a_ij|.  The first term
is the one rounding to float32 (the comparison is with the oracle's float64 result before its own narrowing); the second
covers float64 sums taken in tile, slab and lane order instead of LAPACK's -- about 1000 times what the two float64 routes
differ by on the CPU, and 1/4000 of a float32 half-ulp of the row's scale.  The largest second-term error of each case is
printed as a fraction of the row maximum (DESIGN.md section 3.16 records the largest of all).

The spectrum: within 2^-36 s[0] for the values above 2^-20 s[0]; below that the Gram route resolves sqrt(eps) s[0] only,
and the bound is 2^-20 s[0]."""
import ctypes as C

import numpy as np
import pytest

from goleft_amd import _lib
from tests import svddebias_ref as SR
from tests import svddebias_shapes as SS

pytestmark = pytest.mark.gpu

E_INVALID, E_RANGE = -1, -5


class Ctx:
    def __init__(self):
        self.lib = _lib.load()
        self.h = C.c_void_p()
        assert self.lib.gd_create(0, C.byref(self.h)) == 0
        self.hip = C.CDLL("libamdhip64.so")
        self.hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]

    def err(self):
        return self.lib.gd_last_error(self.h).decode()

    def close(self):
        self.lib.gd_destroy(self.h)

    def run(self, depths, pct, zscore, rows=None, n=None, want_s=True, want_n=True):
        """(rc, out, s, n_removed) of gd_svd_debias"""
        d = np.ascontiguousarray(depths, np.float32)
        rows, n = (d.shape[0] if rows is None else rows), (d.shape[1] if n is None else n)
        out = np.full(d.shape, np.nan, np.float32)
        s = np.full(max(min(rows, n), 1), np.nan, np.float64)
        k = C.c_int(-1)
        rc = self.lib.gd_svd_debias(self.h, d.ctypes.data, rows, n, float(pct), int(zscore), out.ctypes.data,
                                    s.ctypes.data if want_s else None, C.byref(k) if want_n else None)
        return rc, out, s, k.value

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

    def resident(self, fn, p_in, p_out, rows, n, pct, zscore):
        s = np.full(min(rows, n), np.nan, np.float64)
        k = C.c_int(-1)
        rc = fn(self.h, p_in, rows, n, float(pct), int(zscore), p_out, s.ctypes.data, C.byref(k))
        return rc, s, k.value


@pytest.fixture(scope="module")
def ctx():
    c = Ctx()
    yield c
    c.close()


def hold(name, A, out, s, k, want):
    """the contract of the module docstring; returns the largest second-term error as a fraction of the row maximum"""
    assert k == want["n"], (name, k, want["n"])
    ref = want["out64"]
    rowmax = A.astype(np.float64).max(axis=1, keepdims=True)
    err = np.abs(out.astype(np.float64) - ref)
    second = np.maximum(err - 2.0 ** -24 * np.abs(ref), 0.0)
    worst = float((second / np.maximum(rowmax, 1e-300)).max())
    print("%s: second-term error %.3g of the row maximum (bound %.3g)" % (name, worst, 2.0 ** -36))
    assert (err <= 2.0 ** -24 * np.abs(ref) + 2.0 ** -36 * rowmax).all(), (name, worst)
    ws = want["s"]
    assert s.shape == ws.shape
    big = ws > 2.0 ** -20 * ws[0]
    ds = np.abs(s - ws)
    print("%s: spectrum off by %.3g s[0] above 2^-20 s[0], %.3g s[0] below" % (
        name, float(ds[big].max() / ws[0]) if big.any() else 0.0, float(ds[~big].max() / ws[0]) if (~big).any() else 0.0))
    assert (ds[big] <= 2.0 ** -36 * ws[0]).all(), (name, float(ds[big].max() / ws[0]))
    assert (ds[~big] <= 2.0 ** -20 * ws[0]).all(), (name, float(ds[~big].max() / ws[0]))
    return worst


@pytest.mark.parametrize("name", SS.NAMES)
def test_every_case_against_the_oracle_twice(ctx, name):
    c = SS.case(name)
    rc, out, s, k = ctx.run(c["A"], c["pct"], c["zscore"])
    assert rc == 0, ctx.err()
    hold(name, c["A"], out, s, k, c)
    rc, out2, s2, k2 = ctx.run(c["A"], c["pct"], c["zscore"])
    assert rc == 0 and k2 == k
    assert out2.tobytes() == out.tobytes() and s2.tobytes() == s.tobytes()


def test_flat_rows_come_out_unchanged(ctx):
    c = SS.case(SS.FLAT)
    rc, out, _, k = ctx.run(c["A"], c["pct"], 1)
    assert rc == 0 and k == 3
    for r, v in SS.FLAT_ROWS.items():
        assert (out[r] == np.float32(v)).all(), r
    # without the z-score they are ordinary rows of the matrix
    want = SR.svd_debias(c["A"], c["pct"], False)
    rc, out, s, k = ctx.run(c["A"], c["pct"], 0)
    assert rc == 0, ctx.err()
    hold("flat rows, raw", c["A"], out, s, k, dict(n=want[2], out64=want[3], s=want[1]))


def test_an_all_zero_matrix(ctx):
    for z in (0, 1):
        rc, out, s, k = ctx.run(np.zeros((70, 66), np.float32), 0.0, z)
        assert rc == 0 and k == 0 and not out.any() and not s.any()


@pytest.mark.parametrize("name", ["n65_slab+1_z", "n257_3slab+7", "n5_all"])
def test_the_three_forms_give_the_same_bytes(ctx, name):
    c = SS.case(name)
    A = c["A"]
    rows, n = A.shape
    assert float(A.max()) < 2 ** 24 and (A == np.floor(A)).all()                      # the float32 conversion is exact
    rc, out, s, k = ctx.run(A, c["pct"], c["zscore"])
    assert rc == 0
    p_cells, p_f, p_out = ctx.upload(A.astype(np.int64)), ctx.upload(A), ctx.upload(np.full(A.shape, np.nan, np.float32))
    try:
        rc, s1, k1 = ctx.resident(ctx.lib.gd_svd_debias_cells, p_cells, p_out, rows, n, c["pct"], c["zscore"])
        assert rc == 0, ctx.err()
        assert ctx.read(p_out, A.shape, np.float32).tobytes() == out.tobytes() and s1.tobytes() == s.tobytes() and k1 == k
        assert ctx.read(p_cells, A.shape, np.int64).tobytes() == A.astype(np.int64).tobytes()
        # the device form into another matrix, then in place
        assert self_fill(ctx, p_out, A.shape)
        rc, s2, k2 = ctx.resident(ctx.lib.gd_svd_debias_device, p_f, p_out, rows, n, c["pct"], c["zscore"])
        assert rc == 0, ctx.err()
        assert ctx.read(p_out, A.shape, np.float32).tobytes() == out.tobytes() and s2.tobytes() == s.tobytes() and k2 == k
        assert ctx.read(p_f, A.shape, np.float32).tobytes() == A.tobytes()
        rc, s3, k3 = ctx.resident(ctx.lib.gd_svd_debias_device, p_f, p_f, rows, n, c["pct"], c["zscore"])
        assert rc == 0, ctx.err()
        assert ctx.read(p_f, A.shape, np.float32).tobytes() == out.tobytes() and s3.tobytes() == s.tobytes() and k3 == k
    finally:
        ctx.free(p_cells, p_f, p_out)


def self_fill(ctx, p, shape):
    a = np.full(shape, np.nan, np.float32)
    return ctx.hip.hipMemcpy(p, a.ctypes.data, a.nbytes, 1) == 0


def good(ctx):
    c = SS.case("n5_rank_z")
    rc, out, _, k = ctx.run(c["A"], c["pct"], c["zscore"])
    assert rc == 0 and k == c["n"] and np.isfinite(out).all(), ctx.err()


def test_null_outputs_are_accepted(ctx):
    c = SS.case("n63_slab-1_z")
    rc, out, s, k = ctx.run(c["A"], c["pct"], 1)
    rc2, out2, s2, k2 = ctx.run(c["A"], c["pct"], 1, want_s=False, want_n=False)
    assert rc == 0 and rc2 == 0 and out2.tobytes() == out.tobytes()
    assert np.isnan(s2).all() and k2 == -1


def test_sizes_and_shares_out_of_range(ctx):
    A = SS.case("n5_all")["A"]
    for rows, n in ((300, 1), (1, 1025), (0, 5)):
        rc, _, _, _ = ctx.run(A, 1.0, 0, rows=rows, n=n)
        assert rc == E_RANGE and ctx.err(), (rows, n)
        good(ctx)
    for pct in (float("nan"), -1.0, float("inf"), -float("inf")):
        rc, _, _, _ = ctx.run(A, pct, 1)
        assert rc == E_RANGE and "share" in ctx.err(), pct
        good(ctx)


@pytest.mark.parametrize("bad", [np.nan, -1.0, np.inf, -np.inf])
def test_a_cell_that_is_no_depth_is_named(ctx, bad):
    A = SS.case("n65_rank")["A"].copy()
    A[37, 64] = bad
    rc, _, _, _ = ctx.run(A, 1.0, 1)
    assert rc == E_INVALID and "row 37, sample 64" in ctx.err(), ctx.err()
    good(ctx)
    p_f, p_out = ctx.upload(A), ctx.upload(A)
    try:
        rc, _, _ = ctx.resident(ctx.lib.gd_svd_debias_device, p_f, p_out, A.shape[0], A.shape[1], 1.0, 1)
        assert rc == E_INVALID and "row 37, sample 64" in ctx.err(), ctx.err()
        assert ctx.read(p_out, A.shape, np.float32).tobytes() == A.tobytes()         # nothing written
    finally:
        ctx.free(p_f, p_out)
    good(ctx)


def test_a_negative_cell_of_the_int64_form_is_named(ctx):
    A = SS.case("n65_rank")["A"].astype(np.int64)
    A[3, 1] = -2
    p_cells, p_out = ctx.upload(A), ctx.upload(np.zeros(A.shape, np.float32))
    try:
        rc, _, _ = ctx.resident(ctx.lib.gd_svd_debias_cells, p_cells, p_out, A.shape[0], A.shape[1], 1.0, 0)
        assert rc == E_INVALID and "row 3, sample 1" in ctx.err(), ctx.err()
    finally:
        ctx.free(p_cells, p_out)
    good(ctx)


def test_a_result_that_overlaps_its_input_is_refused(ctx):
    A = SS.case("n65_rank")["A"]
    rows, n = A.shape
    p_cells = ctx.upload(A.astype(np.int64))
    p_f = ctx.upload(A)
    try:
        for off in (0, 4, rows * n * 8 - 4):
            rc, _, _ = ctx.resident(ctx.lib.gd_svd_debias_cells, p_cells, C.c_void_p(p_cells.value + off), rows, n, 1.0, 1)
            assert rc == E_INVALID and "overlap" in ctx.err(), off
        good(ctx)
        assert ctx.read(p_cells, A.shape, np.int64).tobytes() == A.astype(np.int64).tobytes()
        # the device form takes the matrix itself, not a part of it
        rc, _, _ = ctx.resident(ctx.lib.gd_svd_debias_device, p_f, C.c_void_p(p_f.value + 4 * n), rows - 1, n, 1.0, 1)
        assert rc == E_INVALID and "itself" in ctx.err()
        assert ctx.read(p_f, A.shape, np.float32).tobytes() == A.tobytes()
    finally:
        ctx.free(p_cells, p_f)
    good(ctx)


def test_the_timing_is_positive_after_a_call(ctx):
    good(ctx)
    t = (C.c_double * 5)()
    assert ctx.lib.gd_svd_debias_timing(ctx.h, t, 5) == 0
    assert all(v > 0 for v in t), list(t)
