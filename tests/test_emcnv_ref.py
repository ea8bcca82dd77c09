"""CPU: the restatement of emdepth.Cache (tests/emcnv_ref.py) against the reference's own unit test, its quirks on
hand-made inputs, the parallel form against the sequential walk, and the conditions every case of
tests/emcnv_shapes.py must meet for the device comparison to be exact (asserted from the restatement alone)."""
import math

import numpy as np
import pytest

from tests import emcnv_ref as C
from tests import emcnv_shapes as S
from tests import emdepth_ref as R

INF = math.inf


def emd_of(depths):
    row = R.em_row(depths)
    return C.EMD(0, np.asarray(depths, np.float32), 123, 456, cn=row.cn, lam2=row.lam[2])


def test_reference_unit_test_same():
    """emdepth_test.go:38-49 (TestBig): em2.Same(cns)"""
    cns = emd_of([296.6, 16.7, 17.0, 3019.2, 14.4, 16.5, 14.2, 26, 7])
    em2 = emd_of([96.6, 16.7, 17.0, 319.2, 14.4, 16.5, 14.2, 7, 16])
    non2, changed, pct = C.same(em2, cns)
    assert non2 == [0, 3]
    assert changed == [7, 8]
    assert pct == 7.0 / 9.0


def fake(fc_rows, starts, ends):
    """EMDs with given fold changes (the depth of a cell is its row number, its cn 7: they only travel)"""
    n = len(fc_rows[0])
    return [C.EMD(r, [float(r)] * n, starts[r], ends[r], fc=list(fc), cn=[7] * n) for r, fc in enumerate(fc_rows)]


def keys(cnvs):
    return [(c.sample, c.psize, c.emit_row, tuple(c.rows)) for c in cnvs]


def tiled(rows, width=10000):
    return [1000000 + r * width for r in range(rows)], [1000000 + (r + 1) * width for r in range(rows)]


def test_row_zero_is_compared_with_itself():
    st, en = tiled(1)
    assert keys(C.run_cache(fake([[0.0, 1.0, -INF, math.nan]], st, en))) == [(1, 2, 1, (0,)), (2, 2, 1, (0,))]


def test_up_then_down_is_a_change_and_nan_never_a_member():
    st, en = tiled(4)
    fc = [[0, 1.0, math.nan], [0, 1.0, math.nan], [0, -1.0, math.nan], [0, -1.0, 0]]
    # row 0 (itself) and row 1 are U members, row 2 changed, row 3 is a D member: one list, nothing between them gapped
    assert keys(C.run_cache(fake(fc, st, en))) == [(1, 1, 4, (0, 1, 3))]


def test_thresholds_are_inclusive():
    st, en = tiled(2)
    fc = [[0, 0.40, -0.80, 0.39999, -0.79999]] * 2
    assert [k[0] for k in keys(C.run_cache(fake(fc, st, en)))] == [1, 2]


def test_sample_zero_loses_its_list_in_every_clear_that_finds_one():
    st, en = tiled(12, width=1000)
    for r in range(8, 12):
        st[r] += 50000
        en[r] += 50000
    fc = [[1.0, 0.0]] * 12
    # sample 0 is a member of every row; each Clear drops its one-site list, emitted only where the next row is a gap
    # (row 8) and at the end
    assert keys(C.run_cache(fake(fc, st, en))) == [(0, 1, 8, (7,)), (0, 1, 12, (11,))]
    # beside another sample's list it is the same, and PSize counts both
    fc = [[1.0, -1.0]] * 12
    assert keys(C.run_cache(fake(fc, st, en))) == [(0, 2, 8, (7,)), (1, 2, 8, tuple(range(8))), (0, 2, 12, (11,)),
                                                   (1, 2, 12, (8, 9, 10, 11))]


def test_a_start_before_the_end_wraps_into_a_gap():
    st = [1000000, 1010000, 500, 10500]
    en = [1010000, 1020000, 10500, 20500]
    fc = [[0.0, 1.0]] * 4
    assert keys(C.run_cache(fake(fc, st, en))) == [(1, 1, 2, (0, 1)), (1, 1, 4, (2, 3))]


def test_gap_of_exactly_30000():
    for g, want in ((29999, [(1, 1, 3, (0, 1, 2))]), (30000, [(1, 1, 2, (0, 1)), (1, 1, 3, (2,))])):
        st = [0, 1000, 2000 + g]
        en = [1000, 2000, 2000 + g]
        assert keys(C.run_cache(fake([[0.0, 1.0]] * 3, st, en))) == want, g


def test_final_test_is_against_start_plus_100000():
    for width, want in ((70000, [(1, 1, 2, (0, 1))]), (70001, [])):
        st, en = [0, 1000], [1000, 1000 + width]
        assert keys(C.run_cache(fake([[0.0, 1.0]] * 2, st, en))) == want, width
    # near 2^32 the sum wraps: start + 100000 comes out below the end, and the difference wraps again
    st, en = [2 ** 32 - 100500, 2 ** 32 - 100000], [2 ** 32 - 100000, 2 ** 32 - 99500]
    assert keys(C.run_cache(fake([[0.0, 1.0]] * 2, st, en))) == [(1, 1, 2, (0, 1))]


def test_repeated_positions_never_gap_before_the_end():
    fc = [[0.0, 1.0, -1.0]] * 6
    assert keys(C.run_cache(fake(fc, [5000] * 6, [5000] * 6))) == [(1, 2, 6, tuple(range(6))), (2, 2, 6, tuple(range(6)))]


def test_the_filter_of_makecnvs_never_meets_a_member():
    """-0.5 < fc < 0.3 lies inside (-0.80, 0.40): a member's fc is outside it.  The filter is kept in the restatement;
    on a list that does hold such a value (which Add cannot build) it works as written."""
    st, en = tiled(3)
    es = fake([[0.0, 1.0], [0.0, 0.1], [0.0, 1.0]], st, en)
    assert C.makecnvs(es, 1).rows == [0, 2]
    assert C.makecnvs(es[1:2], 1) is None
    for name in S.cases():
        ref = S.reference(name)
        for c in ref.cnvs:
            assert all(not (-0.5 < ref.fc[r][c.sample] < 0.3) for r in c.rows)


@pytest.mark.parametrize("seed", range(8))
def test_parallel_form_equals_the_walk(seed):
    rng = np.random.default_rng(seed)
    values = np.array([0.0, 0.0, 0.0, 1.0, 1.0, -1.0, -1.0, 0.40, -0.80, 0.39, -0.79, INF, -INF, math.nan])
    for _ in range(150):
        rows, n = int(rng.integers(0, 26)), int(rng.integers(1, 8))
        if rows == 0:
            assert C.parallel_form([], [], []) == [] and C.run_cache([]) == []
            continue
        fc = rng.choice(values, size=(rows, n))
        persist = rng.random((rows, n)) < 0.6            # runs: a cell often repeats the one above
        for r in range(1, rows):
            fc[r] = np.where(persist[r], fc[r - 1], fc[r])
        kind = int(rng.integers(0, 4))
        if kind == 0:                                    # tiled, with jumps and restarts
            width = int(rng.choice([1000, 10000, 29999, 30000]))
            st = np.cumsum(rng.choice([width, width, width + 30000, width + 29999], size=rows)).astype(np.int64)
            if rows > 3:
                st[rows // 2:] -= st[rows // 2]
            en = st + width
        elif kind == 1:                                  # repeated
            st = np.full(rows, 7000, np.int64)
            en = st + int(rng.choice([0, 10]))
        elif kind == 2:                                  # anything
            st = rng.integers(0, 2 ** 32, size=rows)
            en = rng.integers(0, 2 ** 32, size=rows)
        else:                                            # around 2^32
            st = (2 ** 32 - 130000 + np.cumsum(rng.integers(0, 40000, size=rows))) % 2 ** 32
            en = (st + rng.integers(0, 80000, size=rows)) % 2 ** 32
        st, en = [int(v) for v in st], [int(v) for v in en]
        fcl = [[float(v) for v in row] for row in fc]
        assert C.parallel_form(fcl, st, en) == keys(C.run_cache(fake(fcl, st, en))), (seed, rows, n, kind)


@pytest.mark.parametrize("name", sorted(S.cases()))
def test_case_conditions(name):
    case, ref = S.cases()[name], S.reference(name)
    left_out, members, excluded = S.plan(name)
    print("%s: %d rows x %d, %d CNVs, %d member cells, %d near a threshold, %d rows left out, %d member cells excluded" % (
        name, case.depths.shape[0], case.depths.shape[1], len(ref.cnvs), len(members), len(ref.near), left_out, len(excluded)))
    assert ref.near == []
    assert left_out == 0
    assert len(excluded) <= S.CAP * len(members)
    if case.want is True:
        assert len(ref.cnvs) >= 1
    if case.want is False:
        assert ref.cnvs == []
    if case.depths.shape[0] <= 600:
        assert C.parallel_form(ref.fc, [int(v) for v in case.starts], [int(v) for v in case.ends]) == keys(ref.cnvs)


def test_shapes_meant_to_differ_do():
    n = {k: len(S.reference(k).cnvs) for k in ("gap_29999", "gap_30000", "final_70000", "final_70001")}
    assert n == {"gap_29999": 1, "gap_30000": 2, "final_70000": 1, "final_70001": 0}
    s0 = [c for c in S.reference("sample0").cnvs if c.sample == 0]
    assert s0 and all(len(c.rows) == 1 for c in s0)
    sizes = {c.psize for c in S.reference("psize").cnvs}
    assert min(sizes) == 1 and max(sizes) == 4 and len(sizes) >= 3         # one, several, four of nine at once
    assert max(len(c.rows) for c in S.reference("long_cnv").cnvs) > S.CHUNK
    assert max(np.bincount([c.emit_row for c in S.reference("many_at_one_row").cnvs])) == 30
    case = S.cases()["dense"]
    assert 0.4 <= len(S.plan("dense")[1]) / case.depths.size <= 0.6
    assert any(R.em_row(r).lam[2] != np.median(r) and 0 in r for r in S.cases()["fallback"].depths[3:4])
    # ... and the moved lambda[2] decides: a member of those rows would be in another state against the row's median
    fb, ref = S.cases()["fallback"], S.reference("fallback")
    moved = [(r, c.sample) for c in ref.cnvs for r in c.rows if 3 <= r < 8 and
             C.state_of(ref.fc[r][c.sample]) != C.state_of(C.log2_quotient(float(fb.depths[r][c.sample]), R.median32(fb.depths[r])))]
    assert moved
    assert len(S.reference("sparse_long").cnvs) == 1 and len(S.reference("sparse_long").cnvs[0].rows) == 41     # (40 pairs; row 0 is a member too, against itself)
    assert max(c.rows[-1] - c.rows[0] for c in S.reference("repeated_long").cnvs) > S.SPAN2    # one list from end to end
