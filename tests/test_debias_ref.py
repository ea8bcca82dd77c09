"""CPU: tests/debias_ref.py, the restatement of dcnv's ChunkDebiaser (dcnv/debiaser/debiaser.go:125-171), pinned on
hand-made columns: the index (n - k) / 2 from the start of the chunk, the strict float64 comparison at a chunk boundary,
and the two properties the device form rests on -- the order among tied vals changes no bit, and permuting the rows
permutes the result."""
import numpy as np
import pytest

from tests import debias_ref as R

F = np.float32


@pytest.mark.parametrize("cells,want", [
    ([5], 5),                                    # n, k = 1, 0: sorted[0]
    ([7, 3], 7),                                 # 2, 0: sorted[1], the upper of the two
    ([7, 0], 0),                                 # 2, 1: sorted[0] is the zero (n < 3k)
    ([9, 0, 4], 4),                              # 3, 1: sorted[1]
    ([3, 0, 1, 0, 2], 0),                        # 5, 2: sorted[1] is still a zero (5 < 6)
    ([4, 0, 1, 3, 0, 2], 1),                     # 6, 2: sorted[2], the first non-zero (n = 3k)
    ([0, 0, 0], 0),                              # all zero: sorted[0]
    ([0, -0.0, 1, 2, 3, 4], 1),                  # -0.0 counts as a zero
    ([0, 0, 1, 2, 3, 4, 5], 1),                  # 7, 2: n = 3k + 1 -> sorted[2]
])
def test_chunk_median(cells, want):
    got = R.chunk_median(np.array(cells, F))
    assert got.dtype == F and got == F(want) and not np.signbit(got)


def test_zero_median_leaves_the_chunk():
    m = np.array([[7, 2], [0, 4], [1, 6]], F)
    o64, o, cor, C, med = R.debias(m, [0.5, 0.5, 0.5], 0.01)
    assert C == 1 and cor.tolist() == [0, 0, 0]
    assert med.tolist() == [[1, 4]]
    assert o64[:, 0].tolist() == [7, 0, 1] and o64[:, 1].tolist() == [0.5, 1.0, 1.5]
    m[:, 0] = [7, 0, 0]                          # n = 3, k = 2: median 0, the column stays
    o64, o, _, _, med = R.debias(m, [0.5, 0.5, 0.5], 0.01)
    assert med[0, 0] == 0 and o64[:, 0].tolist() == [7, 0, 0] and o[:, 0].tolist() == [7, 0, 0]


def test_division_is_one_float64_division_then_narrowed():
    m = np.array([[1], [3], [3]], F)
    o64, o, _, _, _ = R.debias(m, [0, 0, 0], 1.0)
    assert o64[0, 0] == 1.0 / 3.0 and o[0, 0] == F(1.0 / 3.0) and o64.dtype == np.float64 and o.dtype == F
    big = np.array([[np.finfo(F).max], [1e-45], [1e-45]], F)           # FLT_MAX over a denormal: inf as float32 only
    o64, o, _, _, med = R.debias(big, [0, 0, 0], 1.0)
    assert med[0, 0] == F(1e-45) and np.isfinite(o64[0, 0]) and np.isinf(o[0, 0])


def test_boundary_is_strictly_greater_in_float64():
    W = 0.25
    v0 = 0.5
    at = v0 + W                                  # exact in float64
    above = np.nextafter(at, np.inf)
    _, sl, cor = R.chunks([v0, at], W)
    assert sl.tolist() == [0, 2] and cor.tolist() == [0, 0]
    _, sl, cor = R.chunks([v0, above], W)
    assert sl.tolist() == [0, 1, 2] and cor.tolist() == [0, 1]
    # v0 is the value that opened the chunk, not the one before (0.5 - 0.25 is not above W; 0.5 - 0.0 is)
    _, sl, cor = R.chunks([0.0, 0.125, 0.25, 0.5, 0.75], W)
    assert sl.tolist() == [0, 3, 5] and cor.tolist() == [0, 0, 0, 1, 1]


def test_a_tenth_and_two_tenths():
    # 0.1 + 0.2 is 0.30000000000000004: one ulp above 0.3.  From v0 = 0.1 the differences are 0.2 and
    # 0.20000000000000004 (both exact), the window 0.2
    assert 0.1 + 0.2 > 0.3
    _, sl, _ = R.chunks([0.1, 0.3], 0.2)
    assert (0.3 - 0.1 > 0.2) == (len(sl) == 3)
    _, sl2, _ = R.chunks([0.1, 0.1 + 0.2], 0.2)
    assert ((0.1 + 0.2) - 0.1 > 0.2) == (len(sl2) == 3)
    assert len(sl) == 2 and len(sl2) == 3        # 0.3 - 0.1 = 0.19999999999999998; (0.1 + 0.2) - 0.1 = 0.20000000000000004


def test_all_vals_tie_and_window_below_the_smallest_gap():
    rng = np.random.default_rng(5)
    m = rng.integers(0, 50, (7, 3)).astype(F)
    _, sl, cor = R.chunks([0.4] * 7, 1e-300)
    assert sl.tolist() == [0, 7] and not cor.any()
    vals = np.array([0.7, 0.1, 0.4, 0.2, 0.6, 0.3, 0.5])
    order, sl, cor = R.chunks(vals, 0.05)
    assert sl.tolist() == list(range(8)) and cor.tolist() == [6, 0, 3, 1, 5, 2, 4]
    o64, o, _, C, med = R.debias(m, vals, 0.05)
    assert C == 7
    for r in range(7):                           # a chunk of one row: the cell over itself, or left when it is 0
        assert np.array_equal(med[cor[r]], m[r])
        assert np.array_equal(o64[r], np.where(m[r] > 0, 1.0, 0.0))


def _same(a, b):
    return all(np.array_equal(x.view(np.uint8) if isinstance(x, np.ndarray) else x, y.view(np.uint8) if isinstance(y, np.ndarray) else y)
               for x, y in zip(a, b))


def test_order_among_ties_changes_no_bit():
    rng = np.random.default_rng(11)
    R_, N = 60, 4
    vals = rng.integers(0, 6, R_) * 0.125        # many ties, gaps of 0.125
    m = (rng.integers(0, 9, (R_, N)) * rng.random((R_, N))).astype(F)
    base = R.debias(m, vals, 0.2)
    assert 1 < base[3] < R_
    stable = np.argsort(vals, kind="stable")
    for seed in range(5):
        # shuffle inside every run of equal vals
        jitter = np.random.default_rng(seed).random(R_)
        order = np.lexsort((jitter, vals))
        assert np.array_equal(vals[order], vals[stable])
        assert seed == 0 or not np.array_equal(order, stable)
        assert _same(base, R.debias(m, vals, 0.2, order=order))


def test_permuting_rows_with_their_vals_permutes_the_output():
    rng = np.random.default_rng(12)
    R_, N = 50, 3
    vals = np.round(rng.normal(0.41, 0.05, R_), 2)
    m = (rng.integers(0, 5, (R_, N)) * rng.random((R_, N)) * 30).astype(F)
    o64, o, cor, C, med = R.debias(m, vals, 0.03)
    p = rng.permutation(R_)
    p64, po, pcor, pC, pmed = R.debias(m[p], vals[p], 0.03)
    assert pC == C and _same((o64[p], o[p], cor[p], med), (p64, po, pcor, pmed))


def test_matrix_text():
    assert R.matrix_text("#chrom\tstart\tend\ta\tb", ["1\t0\t10", "1\t10\t20"], np.array([[1 / 3, 0], [2, 1e-45]], F)) == \
        "#chrom\tstart\tend\ta\tb\n1\t0\t10\t0.333333343\t0\n1\t10\t20\t2\t1.40129846e-45\n"
