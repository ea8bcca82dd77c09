"""CPU: the numpy restatement of gd_depth_hist, gd_region_bins and the dist files (tests/depth_hist_ref.py) on vectors small
enough to work out by hand -- the yardstick of the GPU tests has to be right on its own."""
import numpy as np

from tests import depth_hist_ref as D

A = np.array([0, 0, 1, 3, 3, 7, 2, 0], np.int32)
B = np.array([5, 5, 5], np.int32)


def test_hist_clamps_the_bins_and_not_the_scalars():
    b, s, lo, hi = D.hist([A], [(0, 0, 8)], 8)
    assert b.dtype == np.uint64 and b.tolist() == [3, 1, 1, 2, 0, 0, 0, 1] and (s, lo, hi) == (16, 0, 7)
    b, s, lo, hi = D.hist([A], [(0, 0, 8)], 3)
    assert b.tolist() == [3, 1, 4] and (s, lo, hi) == (16, 0, 7)
    b, s, lo, hi = D.hist([A], [(0, 0, 8)], 1)
    assert b.tolist() == [8] and (s, lo, hi) == (16, 0, 7)


def test_hist_counts_a_position_once_per_region_that_holds_it():
    b, s, lo, hi = D.hist([A, B], [(0, 2, 6), (0, 3, 5), (1, 0, 3), (0, 4, 4), (1, 1, 1)], 6)
    # [1 3 3 7] + [3 3] + [5 5 5]
    assert b.tolist() == [0, 1, 0, 4, 0, 4] and (s, lo, hi) == (14 + 6 + 15, 1, 7)


def test_hist_of_no_position_is_all_zero():
    for regions in ([], [(0, 3, 3)], [(0, 8, 8), (1, 0, 0)]):
        b, s, lo, hi = D.hist([A, B], regions, 4)
        assert b.tolist() == [0, 0, 0, 0] and (s, lo, hi) == (0, 0, 0)


def test_a_region_outside_the_region_is_not_depth_zero():
    b, s, lo, hi = D.hist([A], [(0, 3, 6)], 8)
    assert b[0] == 0 and lo == 3 and int(b.sum()) == 3


def test_bins_are_the_number_of_cuts_at_or_below_the_depth():
    assert D.bins(A, 0, 8).tolist() == [8]
    assert D.bins(A, 2, 2, [1, 3]).tolist() == [0, 0, 0]
    assert D.bins(A, 0, 8, [1]).tolist() == [3, 5]
    assert D.bins(A, 0, 8, [1, 3, 8]).tolist() == [3, 2, 3, 0]
    assert D.bins(A, 0, 8, [3, 7]).tolist() == [5, 2, 1]
    row = D.bins(A, 1, 7, [2, 3])
    assert row.dtype == np.uint64 and row.tolist() == [2, 1, 3] and int(row.sum()) == 6
    assert int(row[1:].sum()) == 4 and int(row[2:].sum()) == 3          # at or above 2; at or above 3


def test_the_files():
    contigs = [("a", 8), ("z", 0), ("b", 3)]
    depth = [A, np.zeros(0, np.int32), B]
    f = D.files(contigs, depth)
    assert f[".dist.txt"] == ("a\t7\t0.125000\na\t6\t0.125000\na\t5\t0.125000\na\t4\t0.125000\na\t3\t0.375000\na\t2\t0.500000\n"
                              "a\t1\t0.625000\na\t0\t1.000000\n"
                              "b\t5\t1.000000\nb\t4\t1.000000\nb\t3\t1.000000\nb\t2\t1.000000\nb\t1\t1.000000\nb\t0\t1.000000\n"
                              "total\t7\t0.090909\ntotal\t6\t0.090909\ntotal\t5\t0.363636\ntotal\t4\t0.363636\ntotal\t3\t0.545455\n"
                              "total\t2\t0.636364\ntotal\t1\t0.727273\ntotal\t0\t1.000000\n")
    assert f[".summary.txt"] == ("chrom\tlength\tbases\tmean\tmin\tmax\na\t8\t16\t2.00\t0\t7\nz\t0\t0\t0.00\t0\t0\nb\t3\t15\t5.00\t5\t5\n"
                                 "total\t11\t31\t2.82\t0\t7\n")
    assert set(f) == {".dist.txt", ".summary.txt"}
    f = D.files(contigs, depth, max_depth=2, only="a")
    assert f[".dist.txt"] == "a\t2\t0.500000\na\t1\t0.625000\na\t0\t1.000000\ntotal\t2\t0.500000\ntotal\t1\t0.625000\ntotal\t0\t1.000000\n"
    assert f[".summary.txt"] == "chrom\tlength\tbases\tmean\tmin\tmax\na\t8\t16\t2.00\t0\t7\ntotal\t8\t16\t2.00\t0\t7\n"


def test_the_files_over_bed_lines():
    contigs = [("a", 8), ("b", 3)]
    depth = [A, B]
    bed = [(0, 3, 6, "x"), (0, 4, 5, "unknown"), (0, 8, 8, "e")]
    f = D.files(contigs, depth, bed=bed, thresholds=[1, 3, 100])
    assert f[".region.dist.txt"] == ("".join("a\t%d\t%s\n" % (d, v) for d, v in zip(range(7, -1, -1), ["0.250000"] * 4 + ["1.000000"] * 4))
                                     + "".join("total\t%d\t%s\n" % (d, v) for d, v in zip(range(7, -1, -1), ["0.250000"] * 4 + ["1.000000"] * 4)))
    assert f[".summary.txt"] == ("chrom\tlength\tbases\tmean\tmin\tmax\na\t8\t16\t2.00\t0\t7\na_region\t4\t16\t4.00\t3\t7\nb\t3\t15\t5.00\t5\t5\n"
                                 "total\t11\t31\t2.82\t0\t7\ntotal_region\t4\t16\t4.00\t3\t7\n")
    assert f[".thresholds.bed"] == "#chrom\tstart\tend\tregion\t1X\t3X\t100X\na\t3\t6\tx\t3\t3\t0\na\t4\t5\tunknown\t1\t1\t0\na\t8\t8\te\t0\t0\t0\n"
    g = D.files(contigs, depth, bed=[(1, 1, 1, "n")])
    assert g[".region.dist.txt"] == "" and g[".summary.txt"].endswith("b_region\t0\t0\t0.00\t0\t0\ntotal\t11\t31\t2.82\t0\t7\ntotal_region\t0\t0\t0.00\t0\t0\n")
