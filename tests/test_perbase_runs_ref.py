"""CPU: the numpy restatement of gd_perbase_runs (tests/perbase_runs_ref.py) on hand-written vectors.  The DepthEngine
method it restates must exist: the restatement alone pins nothing."""
import numpy as np

from tests import perbase_runs_ref as R


def _runs(d, s, e, cuts=None):
    st, v = R.runs(np.asarray(d, np.int32), s, e, cuts)
    assert st.dtype == np.uint32 and v.dtype == np.int32
    return st.tolist(), v.tolist()


def test_the_engine_has_the_method_restated_here():
    from goleft_amd.engine import DepthEngine
    assert callable(DepthEngine.perbase_runs) and callable(DepthEngine.perbase_runs_timing)


def test_empty_region_and_length_one():
    d = [3, 3, 4]
    for p in (0, 1, 3):
        assert _runs(d, p, p) == ([], [])
    assert _runs(d, 0, 1) == ([0], [3])
    assert _runs(d, 2, 3) == ([2], [4])
    assert _runs([0], 0, 1) == ([0], [0])


def test_constant_and_alternating():
    assert _runs([7] * 9, 0, 9) == ([0], [7])
    assert _runs([0] * 9, 0, 9) == ([0], [0])                       # a run of depth 0 is a run like any other
    assert _runs([0, 1] * 4, 0, 8) == (list(range(8)), [0, 1] * 4)
    assert _runs([0, 1] * 4, 3, 6) == ([3, 4, 5], [1, 0, 1])


def test_a_region_start_inside_a_run_starts_a_run():
    d = [5, 5, 5, 5, 2, 2, 9]
    assert _runs(d, 0, 7) == ([0, 4, 6], [5, 2, 9])
    assert _runs(d, 2, 7) == ([2, 4, 6], [5, 2, 9])                 # d[2] == d[1], still a start
    assert _runs(d, 2, 4) == ([2], [5])
    assert _runs(d, 5, 6) == ([5], [2])


def test_depths_at_a_cut_one_below_and_one_above():
    d = [3, 4, 5, 4, 3, 0]
    assert R.values(d, [4]).tolist() == [0, 1, 1, 1, 0, 0]          # the bin of a depth equal to a cut is the upper one
    assert _runs(d, 0, 6, [4]) == ([0, 1, 4], [0, 1, 0])
    assert _runs(d, 0, 6, [4, 5]) == ([0, 1, 2, 3, 4], [0, 1, 2, 1, 0])
    assert R.values([0, 1, 2 ** 31 - 1], [1, 2 ** 31 - 1]).tolist() == [0, 1, 2]


def test_two_depths_in_one_bin_start_no_run():
    d = [1, 2, 3, 4, 99, 100, 101, 0]
    assert _runs(d, 0, 8, [1, 4, 100]) == ([0, 3, 5, 7], [1, 2, 3, 0])
    assert _runs(d, 1, 3, [1, 4, 100]) == ([1], [1])
    assert _runs(d, 0, 8) == (list(range(8)), d)


def test_labels_and_lines():
    assert R.labels([1, 4, 100]) == ["0:1", "1:4", "4:100", "100:inf"]
    d = np.array([0, 0, 2, 2, 2, 7], np.int32)
    assert R.lines("chrM", d, 0, 6) == "chrM\t0\t2\t0\nchrM\t2\t5\t2\nchrM\t5\t6\t7\n"
    assert R.lines("chrM", d, 1, 6, [1, 4]) == "chrM\t1\t2\t0:1\nchrM\t2\t5\t1:4\nchrM\t5\t6\t4:inf\n"
    assert R.lines("chrM", d, 3, 3) == ""
