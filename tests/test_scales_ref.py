"""CPU: the restatement of dcnv's SampleMedians and of the scale factors (tests/scales_ref.py) on hand-made columns,
each worked out by hand from dcnv/dcnv.go:108-125 as DESIGN.md section 3.12 describes it."""
import numpy as np
import pytest

from tests import scales_ref as SR


def med(col, dtype=np.float32):
    m, n = SR.column_median(np.array(col, dtype))
    return m, n


@pytest.mark.parametrize("n, want", [(1, 0), (2, 1), (3, 1), (20, 13), (40, 26), (65537, 42599)])
def test_rank_is_the_truncated_float64_product(n, want):
    assert SR.rank(0, n) == want
    assert SR.rank(7, n) == 7 + want


def test_all_zero_column_gives_zero_and_no_count():
    assert med([0, 0, 0, 0]) == (0, 0)
    assert med([0, 0], np.int64) == (0, 0)


def test_one_non_zero_among_zeros():
    # k = 4, n = 1: sorted[4 + 0]
    assert med([0, 0, 9, 0, 0]) == (9, 1)


def test_all_equal():
    assert med([7] * 11) == (7, 11)


def test_negative_zero_counts_as_a_zero():
    # sorted: three zeros (one of them -0.0), then 2, 5: k = 3, n = 2, sorted[3 + 1]
    m, n = med([5, -0.0, 0, 2, 0])
    assert (m, n) == (5, 2)
    m, n = med([-0.0, -0.0])
    assert n == 0 and m == 0 and not np.signbit(m)


def test_duplicates_straddling_the_rank():
    # n = 20: rank 13; sorted[12] = sorted[13] = sorted[14] = 4
    col = [1] * 12 + [4] * 3 + [9] * 5
    assert med(col) == (4, 20)
    assert med(col[::-1] + [0, 0]) == (4, 20)


@pytest.mark.parametrize("n", [1, 2, 3, 20, 40])
def test_the_rank_picks_that_value_of_a_ramp(n):
    want = {1: 0, 2: 1, 3: 1, 20: 13, 40: 26}[n]
    col = np.arange(1, n + 1)[::-1]                                 # 1 .. n: sorted[i] = i + 1
    assert med(col, np.int64) == (want + 1, n)
    assert med(list(col) + [0] * 5, np.float32) == (want + 1, n)    # leading zeros move the index, not the value


def test_int64_values_stay_exact():
    a, b = 2 ** 53, 2 ** 53 + 1
    assert med([a, b], np.int64) == (b, 2)                          # n = 2: sorted[1]
    assert med([b, a, a], np.int64) == (a, 3)                       # n = 3: sorted[1]


def test_matrix_form():
    m = np.array([[0, 3, 5], [0, 1, 5], [0, 2, 0]], np.float32)
    got, nz = SR.sample_medians(m)
    assert got.tolist() == [0, 2, 5] and nz.tolist() == [0, 3, 2] and got.dtype == np.float32 and nz.dtype == np.uint64


def test_level_is_the_upper_middle_median():
    assert SR.level_of([5, 1, 3]) == 3                              # odd N: sorted[1]
    assert SR.level_of([5, 1, 3, 7]) == 5                           # even N: sorted[2], the upper of the middle two
    assert SR.level_of([4]) == 4


def test_factors():
    s = SR.scales(np.array([51, 22, 112], np.float32))
    assert s.dtype == np.float32
    assert s.tolist() == [np.float32(1.0), np.float32(51.0 / 22.0), np.float32(51.0 / 112.0)]
    one = SR.scales(np.array([51, 22, 112], np.float32), level=1)
    assert one.tolist() == [np.float32(1.0 / 51.0), np.float32(1.0 / 22.0), np.float32(1.0 / 112.0)]
    # %.9g of a float32 reads back as that float32
    for line, v in zip(SR.scale_lines(s).split("\n"), s):
        assert np.float32(float(line)) == v
