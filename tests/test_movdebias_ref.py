"""CPU: the restatement of dcnv's GeneralDebiaser (tests/movdebias_ref.py) pinned on hand-made columns.  The closed form
(`debias_column`: every row's window is a range of the pushed sequence) is held, bit for bit, to `literal_column`, a
transcription of the Go loop (dcnv/debiaser/debiaser.go:104-120) that feeds a ring push by push and takes the median of
whatever it holds.  Then the skipped rows, and four mutants of the closed form, each killed by a named case."""
import numpy as np
import pytest

from tests import movdebias_ref as MR

WINDOWS = (1, 3, 9)


def row_counts(W):
    mid = MR.mid_of(W)
    return sorted({r for r in (mid, 2 * mid - 1, 2 * mid, 2 * mid + 1, W - 1, W, W + 1, 40) if r >= mid})


def column(seed, rows):
    """depths as a sample has them: integers with duplicates, some zero, one -0.0"""
    rng = np.random.default_rng(seed)
    c = rng.poisson(30.0, rows).astype(np.float32)
    c[rng.random(rows) < 0.2] = 0.0
    if rows > 3:
        c[3] = -0.0
    return c


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same(a, b):
    return np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1]))


@pytest.mark.parametrize("W", WINDOWS)
def test_the_closed_form_is_the_go_loop(W):
    for rows in row_counts(W):
        for seed in range(3):
            c = column(100 * W + seed, rows)
            assert same(MR.debias_column(c, W), MR.literal_column(c, W)), (W, rows, seed)


def test_hand_made_columns():
    # W = 1: mid = 1; row 0 is divided by itself, every later row by the NEXT row's value, the last by its own
    out, med = MR.debias_column(np.array([4, 8, 2, 16, 5], np.float32), 1)
    assert med.tolist() == [4, 2, 16, 5, 5] and np.array_equal(out, np.array([1, 4, 0.125, 3.2, 1], np.float32))
    # W = 3: mid = 2, P = c[0], c[1], c[4], c[5], c[6]; the values of rows 2 and 3 are in no window
    c = np.array([10, 20, 1000, 2000, 30, 60, 40], np.float32)
    out, med = MR.debias_column(c, 3)
    #              {10,20} twice  {10,20,30}  {20,30,60}  {30,40,60} for the last three rows
    assert med.tolist() == [15, 15, 20, 30, 40, 40, 40]
    assert np.array_equal(out, (c.astype(np.float64) / med).astype(np.float32))
    # rows = mid: one partial window for every row
    out, med = MR.debias_column(np.array([6, 2], np.float32), 3)
    assert med.tolist() == [4, 4] and out.tolist() == [1.5, 0.5]


@pytest.mark.parametrize("W", WINDOWS)
def test_a_median_below_one_divides_by_one(W):
    c = np.full(40, 0.25, np.float32)
    c[::7] = 0.5
    out, med = MR.debias_column(c, W)
    assert np.all(med < 1) and np.all(med > 0) and np.array_equal(bits(out), bits(c))
    assert same((out, med), MR.literal_column(c, W))


@pytest.mark.parametrize("W", WINDOWS)
def test_an_all_zero_column(W):
    c = np.zeros(40, np.float32)
    c[5] = -0.0
    out, med = MR.debias_column(c, W)
    assert not bits(med).any()                   # +0.0 everywhere: -0.0 is the key 0
    assert np.array_equal(bits(out), bits(c))    # the dividend keeps its sign
    assert same((out, med), MR.literal_column(c, W))


def test_tied_covariates_go_by_row():
    vals = np.array([0.5, 0.25, 0.5, 0.25, 0.5, 0.75, 0.25])
    assert MR.order_of(vals).tolist() == [1, 3, 6, 0, 2, 4, 5]
    m = np.arange(1, 15, dtype=np.float32).reshape(7, 2) * 3
    out, med = MR.debias(m, vals, 3)
    order = MR.order_of(vals)
    for s in range(2):
        o, d = MR.literal_column(m[order, s], 3)
        assert np.array_equal(out[order, s], o) and np.array_equal(med[order, s], d)
    # the other order of the ties gives another answer: the rule matters
    other = np.array([3, 1, 6, 0, 2, 4, 5])
    assert not np.array_equal(MR.literal_column(m[other, 0], 3)[0], out[other, 0])


@pytest.mark.parametrize("W", WINDOWS)
def test_the_skipped_rows_touch_only_themselves(W):
    mid = MR.mid_of(W)
    for rows in (2 * mid, 2 * mid + 1, 40):
        c = column(7 * W + rows, rows) + 1
        d = c.copy()
        d[mid:2 * mid] = d[mid:2 * mid] * 3 + 5
        (o1, m1), (o2, m2) = MR.debias_column(c, W), MR.debias_column(d, W)
        assert np.array_equal(bits(m1), bits(m2))
        keep = np.ones(rows, bool)
        keep[mid:2 * mid] = False
        assert np.array_equal(bits(o1[keep]), bits(o2[keep])) and np.all(o1[~keep] != o2[~keep])
        assert same((o2, m2), MR.literal_column(d, W))


# ---- mutants of the closed form: each differs from the Go loop on the case named ----
def mutant(c, W, pushed=None, window_of=None, median_of=None):
    c = np.asarray(c, np.float32)
    rows = len(c)
    P = np.abs((pushed or MR.pushed)(c, W)).astype(np.float64)
    med = np.empty(rows)
    for i in range(rows):
        lo, hi = (window_of or MR.window_of)(i, rows, W)
        med[i] = (median_of or MR.median_of)(P[lo:hi], W)
    return (c.astype(np.float64) / np.maximum(med, 1.0)).astype(np.float32), med


RAMP = (np.arange(40, dtype=np.float32) * 3 + 2)     # strictly increasing: every window has its own median


def test_the_harness_of_the_mutants_is_the_closed_form():
    for W in WINDOWS:
        assert same(mutant(RAMP, W), MR.literal_column(RAMP, W))


def test_mutant_pushed_without_the_skip():
    no_skip = lambda c, W: c[:len(c) - MR.mid_of(W)]             # P[t] = c[t]
    for W in WINDOWS:
        assert not same(mutant(RAMP, W, pushed=no_skip), MR.literal_column(RAMP, W)), W


def test_mutant_the_tail_keeps_sliding():
    def slides(i, rows, W):                                       # hi = i + 1 for every row from mid on
        mid = MR.mid_of(W)
        hi = mid if i < mid else i + 1
        return max(0, hi - W), hi
    # named case: W = 9, 40 rows -- 35 values are pushed and rows 34 .. 39 share the window that ends with the last of
    # them; sliding on loses a value of it per row from row 35 on
    got, want = mutant(RAMP, 9, window_of=slides), MR.literal_column(RAMP, 9)
    assert np.array_equal(got[1][:35], want[1][:35]) and np.all(got[1][35:] != want[1][35:])
    assert not same(mutant(RAMP, 3, window_of=slides), MR.literal_column(RAMP, 3))


def test_mutant_a_centred_window():
    def centred(i, rows, W):                                      # W rows of the column around row i, as a pushed range
        h = (W - 1) // 2
        pushes = rows - MR.mid_of(W)
        return min(max(0, i - h), pushes - 1), min(pushes, i + h + 1)
    for W in (3, 9):
        assert not same(mutant(RAMP, W, window_of=centred), MR.literal_column(RAMP, W)), W


def test_mutant_the_lower_median_of_a_partial_window():
    def lower(w, W):
        return np.sort(w)[(len(w) - 1) // 2]
    # named case: W = 3, rows 0 and 1 of the ramp share the partial window {2, 5}: 3.5, not 2
    got, want = mutant(RAMP, 3, median_of=lower), MR.literal_column(RAMP, 3)
    assert want[1][0] == 3.5 and got[1][0] == 2.0
    assert np.array_equal(got[1][2:], want[1][2:])               # full windows: one middle value either way
    # and a matrix shorter than its window: every row's window is partial
    c = RAMP[:12]                                # (W = 9: seven values are pushed; the windows hold 5, 6 and 7)
    assert not same(mutant(c, 9, median_of=lower), MR.literal_column(c, 9))


def test_refusals():
    m, v = np.ones((6, 3), np.float32), np.arange(6.0)
    MR.debias(m, v, 9)                           # mid = 5 <= 6 rows
    for W, rows, code in ((9, 4, MR.E_RANGE), (2, 6, MR.E_RANGE), (0, 6, MR.E_RANGE), (257, 200, MR.E_RANGE), (-1, 6, MR.E_RANGE)):
        with pytest.raises(MR.Refused) as e:
            MR.debias(np.ones((rows, 3), np.float32), np.arange(float(rows)), W)
        assert e.value.code == code, (W, rows)
    for bad in (np.nan, np.inf, -1.0):
        b = m.copy()
        b[2, 1] = bad
        with pytest.raises(MR.Refused) as e:
            MR.debias(b, v, 3)
        assert e.value.code == MR.E_INVALID
    w = v.copy()
    w[3] = np.nan
    with pytest.raises(MR.Refused) as e:
        MR.debias(m, w, 3)
    assert e.value.code == MR.E_INVALID
