"""CPU: the restatement of emdepth.EMDepth (tests/emdepth_ref.py) against the reference's own unit-test vectors, its
quirks each pinned on a hand-made row, and the exclusion caps of every seeded matrix the GPU tests run: at most 1 % of
rows and 1 % of adjusted cells may be left out of a comparison, and that is decided here, by the restatement alone."""
import json
import math
import os

import numpy as np
import pytest

from tests import emdepth_ref as R
from tests import emdepth_shapes as S
from tests.helpers import GOLDEN


def hand(name):
    (row,) = S.reference("hand_" + name)
    return row


def test_golden_vectors():
    with open(os.path.join(GOLDEN, "emdepth_vectors.json")) as f:
        vec = {v["name"]: v for v in json.load(f)["vectors"]}
    for name in ("TestDepth_1", "TestDepth_2"):
        assert R.em_row(vec[name]["depths"]).cn == vec[name]["go_expected"], name
    big = vec["TestBig"]
    got = R.em_row(big["depths"]).cn
    # Type (:278-279) answers len(Lambda) = 9 above lambda[8]; the Go test lists 8 in those two cells.  The code as
    # written is followed (no Go toolchain to run the reference's test): they are 9 here.
    differ = [i for i, (a, b) in enumerate(zip(got, big["go_expected"])) if a != b]
    assert differ == [0, 3] and [got[i] for i in differ] == [9, 9] and [big["go_expected"][i] for i in differ] == [8, 8]
    assert got == big["code_gives"] == [9, 2, 2, 9, 2, 2, 2, 3, 1]


def test_even_median_is_one_place_to_the_right():
    assert R.median32([5, 5, 5, 5, 9, 9]) == 7.0                 # (b[3] + b[4]) / 2, not the middle pair's 5
    assert R.median32([3, 3, 7, 7, 7, 7, 9, 9]) == 7.0
    assert R.median32([1, 2, 3, 4]) == 3.5
    assert R.median32([4, 6, 6, 6, 8]) == 6.0


def test_two_samples_are_refused():
    with pytest.raises(ValueError):
        R.em_row([1.0, 2.0])
    with pytest.raises(ValueError):
        R.em_row([])
    with pytest.raises(IndexError):
        R.median32([1.0, 2.0])                                   # what Go panics on


def test_non_ascending_lambda_and_the_binary_search():
    r = hand("fallback_non_ascending")
    assert r.lam[1] < r.lam[0] and r.lam[2] == R.EPS             # bin 2 stayed empty: lambda[2] is the clamp alone
    # the binary search and a scan differ on such centres: 2.5 lies under lambda[0] = 5.005 and over every other centre; the
    # search never looks at lambda[0] and answers 9, a first-not-below scan answers 0
    scan = lambda lam, d: next((i for i in range(9) if lam[i] >= d), 9)
    d = (r.lam[1] + r.lam[0]) / 2
    assert R.search(r.lam, d, R.Gap()) == 9 and scan(r.lam, d) == 0
    # 1 and 1000 are both "above lambda[8]"; the zeros are CN 0 by the search and CN 2 by adjustCN (lambda[0] = 5.005)
    assert r.cn == [2, 2, 9, 9] and sorted(r.pairs) == [0, 1]
    rows = S.reference("non_ascending")
    assert len(rows) >= 20
    for row in rows:
        assert any(row.lam[k] > row.lam[k + 1] for k in range(8))


def test_fallback_clamps_in_order():
    # all zero: bin 2 is empty, lambda[2] = 0 -> eps (the clamp at i = 2 comes before anything is added to it)
    r = hand("all_zero")
    assert r.iters == 1 and r.lam[0] == 0.0 and r.lam[2] == R.EPS and r.lam[4] == 2 * R.EPS
    assert r.lam[1] == R.EPS / 2 - (R.EPS - R.EPS / 2) / 1.5
    # [0, 0, 1, 1000]: the median is 500.5; pass 1 finds bin 2 empty and adds 1000 * (2 / 4) * (1 / 4) to the clamp, pass 2
    # then has 1000 above lambda[8] (the top bin is not counted): lambda[2] is the clamp alone from there on
    assert R.median32([0.0, 0.0, 1.0, 1000.0]) == 500.5
    lam, it = R.em_lambda([0.0, 0.0, 1.0, 1000.0], R.Gap())
    assert it == 3 and lam[0] == R.EPS * 500.5 and lam[2] == R.EPS and lam[8] == 4 * R.EPS


def test_nine_above_lambda8():
    r = hand("above_lambda8")
    assert r.cn == [0, 0, 0, 9, 0, 0, 0]
    assert hand("go_test_big").cn[0] == 9


def test_all_zero_row():
    r = hand("all_zero")
    assert r.cn == [0] * 9
    a, b = r.pairs[0]
    assert math.isnan(a) and not math.isnan(b)                   # pmf(0, 0) = exp(0 * log 0): NaN, both comparisons false
    assert np.all(np.isneginf(r.log2fc))


def test_hand_rows_do_what_their_names_say():
    assert hand("all_zero").iters == 1                            # a row stopping after one pass
    assert hand("ten_passes").iters == R.MAXITER
    r = hand("on_a_centre")
    assert r.lam[2] == 30.0 and r.lam[4] == 60.0 and r.gap == 0.0
    r = hand("underflow_kept")
    assert r.pairs[8] == (0.0, 0.0) and r.cn[8] == 8
    assert hand("all_equal").cn == [2] * 9
    assert hand("single_sample").cn == [2] and hand("single_sample").lam[2] == 12.5
    for name in ("deep_int", "deep_float"):                       # (the 1e-9 margin of adjustCN is derived for depths <= 4096)
        deep = S.cases()[name].depths
        assert (deep >= 1000).sum() >= 20 and deep.max() <= 4096, name


@pytest.mark.parametrize("name", sorted(S.cases()))
def test_exclusion_caps(name):
    case = S.cases()[name]
    rows = S.reference(name)
    keep, out, adjusted = S.plan(case, rows)
    assert S.within_caps(keep, out, adjusted), (name, int((~keep).sum()), len(keep), len(out), adjusted)
    if case.exact:
        # integers times one power of two a row (or a single value): every bin sum is exact in float64 in any order
        d = case.depths.astype(np.float64)
        for row in d:
            nz = row[row > 0]
            if len(nz) > 1:
                q = 2.0 ** np.floor(np.log2(nz)).min()
                while not np.all(nz / q == np.floor(nz / q)):
                    q /= 2
                assert nz.sum() / q < 2.0 ** 53, name


def test_cli_matrix_has_no_excluded_cell():
    for scale in (None, S.CLI_SCALES):
        rows = R.em_matrix(R.cells_to_depths(S.cli_cells(), scale))
        assert all(not R.pair_excluded(a, b) for r in rows for a, b in r.pairs.values())
        assert len({c for r in rows for c in r.cn}) >= 4          # (the text to compare is not all 2s)
