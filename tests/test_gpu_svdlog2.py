"""GPU: gd_svd_debias_scaled, gd_svd_debias_scaled_cells and gd_svd_debias_scaled_device (goleft_amd/csrc/gd_svdlog2.hpp,
gd_api_svddebias.inc) through the C ABI against the numpy float64 oracle (tests/svdlog2_ref.py, route (a)) on the cases of
tests/svdlog2_shapes.py, whose cut tests/test_svdlog2_ref.py shows to be unambiguous.

centre_cells is the oracle's bit for bit; n_removed is the oracle's; the spectrum is held as tests/test_gpu_svddebias.py
holds it.  Per cell, none left out: |out - ref| <= 2^-24 |ref| + (1 + ref) ln 2 DELTA.  The first term is the one rounding
to float32 (ref is the oracle's float64 result before its own narrowing); DELTA bounds the error of the exponent z' + c,
which 2^x - 1 carries into the cell as (1 + ref) ln 2 per unit.

DELTA = 2^-41 (4.5e-13).  Measured on the MI355X against route (a), the second term was 0 in every case: no cell of any case
was further from the oracle than the one float32 rounding allows, so a float32 result does not resolve the device's exponent
error, and 16 times that measurement bounds nothing.  What DELTA then has to cover is the oracle's own uncertainty: its two
float64 routes differ by up to 1.51e-14 in the exponent on these cases (tests/test_svdlog2_ref.py prints it per case), and
the next power of two above 16 times that is 2^-41.  The error each case implies is printed before it is held, once past
the 2^-24 |ref| allowance and once past the half ulp of the float32 the device wrote, which is the tighter reading and was
0 in every case as well (DESIGN.md section 3.17 records both)."""
import ctypes as C

import numpy as np
import pytest

from tests import svddebias_shapes as SS
from tests import svdlog2_shapes as LS
from tests import test_gpu_svddebias as TS

pytestmark = pytest.mark.gpu

E_INVALID, E_RANGE = -1, -5
NONE, ZSCORE, LOG2 = 0, 1, 2
DELTA = 2.0 ** -41
LN2 = float(np.log(2.0))


class Ctx(TS.Ctx):
    def scaled(self, depths, pct, scaler, rows=None, n=None, want=True):
        """(rc, out, s, n_removed, centre_cells) of gd_svd_debias_scaled; the outputs are NaN / -1 where nothing was written"""
        d = np.ascontiguousarray(depths, np.float32)
        rows, n = (d.shape[0] if rows is None else rows), (d.shape[1] if n is None else n)
        out = np.full(d.shape, np.nan, np.float32)
        s = np.full(max(min(rows, n), 1), np.nan, np.float64)
        m = np.full(max(n, 1), np.nan, np.float32)
        k = C.c_int(-1)
        rc = self.lib.gd_svd_debias_scaled(self.h, d.ctypes.data, rows, n, float(pct), int(scaler), out.ctypes.data,
                                           s.ctypes.data if want else None, C.byref(k) if want else None,
                                           m.ctypes.data if want else None)
        return rc, out, s, k.value, m

    def resident_scaled(self, fn, p_in, p_out, rows, n, pct, scaler):
        s = np.full(min(rows, n), np.nan, np.float64)
        m = np.full(n, np.nan, np.float32)
        k = C.c_int(-1)
        rc = fn(self.h, p_in, rows, n, float(pct), int(scaler), p_out, s.ctypes.data, C.byref(k), m.ctypes.data)
        return rc, s, k.value, m


@pytest.fixture(scope="module")
def ctx():
    c = Ctx()
    yield c
    c.close()


def hold(name, out, s, k, m, want):
    """the contract of the module docstring; returns the exponent error the worst cell implies"""
    assert m.tobytes() == want["m"].tobytes(), (name, np.flatnonzero(m != want["m"])[:8])
    assert k == want["n"], (name, k, want["n"])
    ref = want["out64"]
    err = np.abs(out.astype(np.float64) - ref)
    second = np.maximum(err - 2.0 ** -24 * np.abs(ref), 0.0) / ((1.0 + ref) * LN2)
    worst = float(second.max())
    past_ulp = np.maximum(err - 0.5 * np.spacing(np.abs(out)).astype(np.float64), 0.0) / ((1.0 + ref) * LN2)
    print("%s: the worst cell implies an exponent error of %.3g past 2^-24 |ref|, %.3g past the half ulp (DELTA %.3g)" % (
        name, worst, float(past_ulp.max()), DELTA))
    assert (err <= 2.0 ** -24 * np.abs(ref) + (1.0 + ref) * LN2 * DELTA).all(), (name, worst)
    ws = want["s"]
    assert s.shape == ws.shape
    big = ws > 2.0 ** -20 * ws[0]
    ds = np.abs(s - ws)
    top = ws[0] if ws[0] > 0 else 1.0
    print("%s: spectrum off by %.3g s[0] above 2^-20 s[0], %.3g s[0] below" % (
        name, float(ds[big].max() / top) if big.any() else 0.0, float(ds[~big].max() / top) if (~big).any() else 0.0))
    assert (ds[big] <= 2.0 ** -36 * ws[0]).all(), (name, float(ds[big].max() / top))
    assert (ds[~big] <= 2.0 ** -20 * ws[0]).all(), (name, float(ds[~big].max() / top))
    return worst


def good(ctx):
    c = LS.case("n3_three_rows")
    rc, out, _, k, m = ctx.scaled(c["A"], c["pct"], LOG2)
    assert rc == 0 and k == c["n"] and np.isfinite(out).all() and m.tobytes() == c["m"].tobytes(), ctx.err()


@pytest.mark.parametrize("name", LS.NAMES)
def test_every_case_against_the_oracle_twice(ctx, name):
    c = LS.case(name)
    rc, out, s, k, m = ctx.scaled(c["A"], c["pct"], LOG2)
    assert rc == 0, ctx.err()
    hold(name, out, s, k, m, c)
    rc, out2, s2, k2, m2 = ctx.scaled(c["A"], c["pct"], LOG2)
    assert rc == 0 and k2 == k
    assert out2.tobytes() == out.tobytes() and s2.tobytes() == s.tobytes() and m2.tobytes() == m.tobytes()


def test_the_low_depth_case_clamps_and_lifts(ctx):
    c = LS.case(LS.LOW)
    rc, out, _, _, _ = ctx.scaled(c["A"], c["pct"], LOG2)
    assert rc == 0 and (out >= 0).all()
    assert (out[c["out64"] == 0] <= LN2 * DELTA).all() and (out == 0).any()
    assert (out[c["A"] == 0] > 0).any()


def test_one_row_and_an_all_zero_matrix_remove_nothing(ctx):
    c = LS.case("n3_one_row")
    for pct in (0.0, c["pct"]):
        rc, out, s, k, m = ctx.scaled(c["A"], pct, LOG2)
        assert rc == 0 and k == 0 and not s.any() and m.tobytes() == c["A"][0].tobytes()
        assert (np.abs(out.astype(np.float64) - c["A"]) <= 2.0 ** -24 * c["A"] + (1.0 + c["A"]) * LN2 * DELTA).all()
    rc, out, s, k, m = ctx.scaled(np.zeros((70, 66), np.float32), 0.0, LOG2)
    assert rc == 0 and k == 0 and not out.any() and not s.any() and not m.any()


@pytest.mark.parametrize("name", ["n65_slab+1", LS.LOW, "n2_slab+1_all", LS.SELECT])
def test_the_three_forms_give_the_same_bytes(ctx, name):
    c = LS.case(name)
    A = c["A"]
    rows, n = A.shape
    rc, out, s, k, m = ctx.scaled(A, c["pct"], LOG2)
    assert rc == 0
    whole = bool((A == np.floor(A)).all() and float(A.max()) < 2 ** 24)               # the float32 conversion is exact
    assert whole == (name != LS.SELECT)
    p_f, p_out = ctx.upload(A), ctx.upload(np.full(A.shape, np.nan, np.float32))
    p_cells = ctx.upload(A.astype(np.int64)) if whole else None
    same = lambda s1, k1, m1: s1.tobytes() == s.tobytes() and k1 == k and m1.tobytes() == m.tobytes()
    try:
        if whole:
            rc, s1, k1, m1 = ctx.resident_scaled(ctx.lib.gd_svd_debias_scaled_cells, p_cells, p_out, rows, n, c["pct"], LOG2)
            assert rc == 0, ctx.err()
            assert ctx.read(p_out, A.shape, np.float32).tobytes() == out.tobytes() and same(s1, k1, m1)
            assert ctx.read(p_cells, A.shape, np.int64).tobytes() == A.astype(np.int64).tobytes()
            assert TS.self_fill(ctx, p_out, A.shape)
        # the device form into another matrix, then in place
        rc, s2, k2, m2 = ctx.resident_scaled(ctx.lib.gd_svd_debias_scaled_device, p_f, p_out, rows, n, c["pct"], LOG2)
        assert rc == 0, ctx.err()
        assert ctx.read(p_out, A.shape, np.float32).tobytes() == out.tobytes() and same(s2, k2, m2)
        assert ctx.read(p_f, A.shape, np.float32).tobytes() == A.tobytes()
        rc, s3, k3, m3 = ctx.resident_scaled(ctx.lib.gd_svd_debias_scaled_device, p_f, p_f, rows, n, c["pct"], LOG2)
        assert rc == 0, ctx.err()
        assert ctx.read(p_f, A.shape, np.float32).tobytes() == out.tobytes() and same(s3, k3, m3)
    finally:
        ctx.free(p_f, p_out, *([p_cells] if whole else []))


@pytest.mark.parametrize("name", ["n65_slab+1_z", "n257_3slab+7", "n5_all"])
def test_scalers_0_and_1_are_the_existing_entry_points(ctx, name):
    c = SS.case(name)
    A = c["A"]
    rows, n = A.shape
    for z in (0, 1):
        rc, out, s, k = ctx.run(A, c["pct"], z)
        rc2, out2, s2, k2, m2 = ctx.scaled(A, c["pct"], ZSCORE if z else NONE)
        assert rc == 0 and rc2 == 0, ctx.err()
        assert out2.tobytes() == out.tobytes() and s2.tobytes() == s.tobytes() and k2 == k
        assert np.isnan(m2).all()                                                     # untouched unless the scaler is log2
    p_f, p_out = ctx.upload(A), ctx.upload(np.full(A.shape, np.nan, np.float32))
    try:
        rc, s3, k3, m3 = ctx.resident_scaled(ctx.lib.gd_svd_debias_scaled_device, p_f, p_out, rows, n, c["pct"], c["zscore"])
        assert rc == 0 and k3 == c["n"] and np.isnan(m3).all(), ctx.err()
        assert ctx.read(p_out, A.shape, np.float32).tobytes() == ctx.run(A, c["pct"], c["zscore"])[1].tobytes()
    finally:
        ctx.free(p_f, p_out)


def untouched(out, s, k, m):
    return np.isnan(out).all() and np.isnan(s).all() and k == -1 and np.isnan(m).all()


def test_a_scaler_that_is_none_of_the_three_is_refused(ctx):
    c = LS.case("n64_cs")
    A = c["A"]
    for scaler in (3, -1, 256, 2 ** 31 - 1):
        rc, out, s, k, m = ctx.scaled(A, c["pct"], scaler)
        assert rc == E_RANGE and "scaler" in ctx.err() and untouched(out, s, k, m), scaler
        good(ctx)
    p_f, p_out = ctx.upload(A), ctx.upload(np.full(A.shape, np.nan, np.float32))
    p_cells = ctx.upload(A.astype(np.int64))
    try:
        for fn, p in ((ctx.lib.gd_svd_debias_scaled_device, p_f), (ctx.lib.gd_svd_debias_scaled_cells, p_cells)):
            rc, s, k, m = ctx.resident_scaled(fn, p, p_out, A.shape[0], A.shape[1], c["pct"], 3)
            assert rc == E_RANGE and np.isnan(s).all() and k == -1 and np.isnan(m).all()
            assert np.isnan(ctx.read(p_out, A.shape, np.float32)).all()
    finally:
        ctx.free(p_f, p_out, p_cells)
    good(ctx)


def test_sizes_and_shares_out_of_range(ctx):
    A = LS.case("n64_cs")["A"]
    for rows, n in ((64, 1), (1, 1025), (0, 5)):
        rc, out, s, k, m = ctx.scaled(A, 1.0, LOG2, rows=rows, n=n)
        assert rc == E_RANGE and ctx.err() and untouched(out, s, k, m), (rows, n)
        good(ctx)
    for pct in (float("nan"), -1.0, float("inf"), -float("inf")):
        rc, out, s, k, m = ctx.scaled(A, pct, LOG2)
        assert rc == E_RANGE and "share" in ctx.err() and untouched(out, s, k, m), pct
        good(ctx)


@pytest.mark.parametrize("bad", [np.nan, -1.0, np.inf, -np.inf])
def test_a_cell_that_is_no_depth_is_named(ctx, bad):
    A = LS.case("n65_cs+1")["A"].copy()
    A[37, 64] = bad
    rc, out, s, k, m = ctx.scaled(A, 1.0, LOG2)
    assert rc == E_INVALID and "row 37, sample 64" in ctx.err() and untouched(out, s, k, m), ctx.err()
    good(ctx)
    p_f, p_out = ctx.upload(A), ctx.upload(A)
    try:
        rc, s, k, m = ctx.resident_scaled(ctx.lib.gd_svd_debias_scaled_device, p_f, p_out, A.shape[0], A.shape[1], 1.0, LOG2)
        assert rc == E_INVALID and "row 37, sample 64" in ctx.err(), ctx.err()
        assert np.isnan(s).all() and k == -1 and np.isnan(m).all()
        assert ctx.read(p_out, A.shape, np.float32).tobytes() == A.tobytes()         # nothing written
    finally:
        ctx.free(p_f, p_out)
    good(ctx)


def test_a_negative_cell_of_the_int64_form_is_named(ctx):
    A = LS.case("n65_cs+1")["A"].astype(np.int64)
    A[3, 1] = -2
    p_cells, p_out = ctx.upload(A), ctx.upload(np.zeros(A.shape, np.float32))
    try:
        rc, s, k, m = ctx.resident_scaled(ctx.lib.gd_svd_debias_scaled_cells, p_cells, p_out, A.shape[0], A.shape[1], 1.0, LOG2)
        assert rc == E_INVALID and "row 3, sample 1" in ctx.err(), ctx.err()
        assert np.isnan(s).all() and k == -1 and np.isnan(m).all()
    finally:
        ctx.free(p_cells, p_out)
    good(ctx)


def test_null_outputs_are_accepted(ctx):
    c = LS.case("n63_slab-1")
    rc, out, _, _, _ = ctx.scaled(c["A"], c["pct"], LOG2)
    rc2, out2, s2, k2, m2 = ctx.scaled(c["A"], c["pct"], LOG2, want=False)
    assert rc == 0 and rc2 == 0 and out2.tobytes() == out.tobytes()
    assert np.isnan(s2).all() and k2 == -1 and np.isnan(m2).all()


def test_the_timing_is_positive_and_the_medians_keep_theirs(ctx):
    A = LS.case("n64_cs")["A"]
    med = np.empty(A.shape[1], np.float32)
    assert ctx.lib.gd_sample_medians(ctx.h, A.ctypes.data, A.shape[0], A.shape[1], med.ctypes.data, None) == 0
    before = (C.c_double * 4)()
    assert ctx.lib.gd_sample_medians_timing(ctx.h, before, 4) == 0
    good(ctx)
    t = (C.c_double * 5)()
    assert ctx.lib.gd_svd_debias_timing(ctx.h, t, 5) == 0
    assert all(v > 0 for v in t), list(t)
    after = (C.c_double * 4)()
    assert ctx.lib.gd_sample_medians_timing(ctx.h, after, 4) == 0
    assert list(after) == list(before)
