"""CPU: `indexsplit` without a device -- the restatement (tests/indexsplit_ref.py) against rows worked out by hand on
tiny cohorts, the no-gap / no-overlap check of the reference's functional-tests.sh on the restatement's rows for a
synthetic cohort and for the reference's own .bai fixtures, and the new ABI and host symbols."""
import os

import numpy as np
import pytest

from goleft_amd import _hostlib, _lib
from tests import indexcov_ref as IR
from tests import indexsplit_ref as R
from tests.helpers import ROOT

GOLD = os.path.join(ROOT, "tests", "golden", "ref")
G = 10 ** 9                                                  # a tile of k * G bytes is a cell of exactly k


def intervals(cells, start=1 << 20):
    """The stored linear index of one reference whose tile sizes are cells (in units of 1e9)."""
    if len(cells) == 0:
        return np.zeros(0, np.uint64)
    s = [int(round(c * G)) for c in cells]
    return np.concatenate([[start], start + np.cumsum(s)]).astype(np.uint64)


def cohort(tmp_path, samples, refs):
    """samples: per sample a list (one per reference it has) of cell lists; refs: [(name, length)] -> (paths, fai)."""
    paths = []
    for k, per_ref in enumerate(samples):
        p = str(tmp_path / ("s%d.bai" % k))
        IR.write_bai(p, [(intervals(c), None) for c in per_ref])
        paths.append(p)
    fai = tmp_path / "ref.fai"
    fai.write_text("".join("%s\t%d\t%d\t60\t61\n" % (n, l, 100 + 10 * i) for i, (n, l) in enumerate(refs)))
    return paths, str(fai)


def rows(*r):
    return "".join("%s\t%d\t%d\t%s\t%d\n" % x for x in r)


def test_tiles_above_chunk_split_2_5_and_8_ways(tmp_path):
    # cells 8 18 34 4 4 9 2 2 2 2 3 8: sum 96, N = 12 -> chunk 8; mean 8, sd 9.43: nothing is above 36.3, nothing chopped
    a = [4, 9, 17, 2, 2, 5, 1, 1, 1, 1, 2, 4]
    b = [4, 9, 17, 2, 2, 4, 1, 1, 1, 1, 1, 4]
    paths, fai = cohort(tmp_path, [[a], [b]], [("c1", 190000)])
    want = rows(
        ("c1", 0, 16384, "8.00", 1),
        # 18: int(0.5 + 18 / 4) = 5 pieces of int(16384 / 5 + 1) = 3277, the last cut at the tile's end
        ("c1", 16384, 19661, "3.60", 5), ("c1", 19661, 22938, "3.60", 5), ("c1", 22938, 26215, "3.60", 5),
        ("c1", 26215, 29492, "3.60", 5), ("c1", 29492, 32768, "3.60", 5),
        # 34: int(0.5 + 8.5) = 9, capped at 8 pieces of 2049
        ("c1", 32768, 34817, "4.25", 8), ("c1", 34817, 36866, "4.25", 8), ("c1", 36866, 38915, "4.25", 8),
        ("c1", 38915, 40964, "4.25", 8), ("c1", 40964, 43013, "4.25", 8), ("c1", 43013, 45062, "4.25", 8),
        ("c1", 45062, 47111, "4.25", 8), ("c1", 47111, 49152, "4.25", 8),
        ("c1", 49152, 81920, "8.00", 1),
        # 9: int(0.5 + 2.25) = 2 pieces of 8193
        ("c1", 81920, 90113, "4.50", 2), ("c1", 90113, 98304, "4.50", 2),
        ("c1", 98304, 163840, "8.00", 1),
        ("c1", 163840, 190000, "11.00", 1))                  # the last tile ends at the reference's length
    assert R.indexsplit(paths, 12, fai=fai) == want
    assert R.partition_gaps(want, [("c1", 190000)]) == []


def test_the_comparison_with_len_plus_one_as_it_stands(tmp_path):
    # 4 tiles, chunk 4: tile 1 (5 pieces) meets i + k == len(size) + 1 at k = 4, tile 2 (8 pieces) at k = 3: those
    # pieces end at the reference's length, in the middle of the reference
    paths, fai = cohort(tmp_path, [[[4, 9, 17, 2]]], [("c1", 60000)])
    got = R.indexsplit(paths, 8, fai=fai).splitlines()
    assert got[5] == "c1\t29492\t60000\t1.80\t5" and got[4] == "c1\t26215\t29492\t1.80\t5"
    assert got[9] == "c1\t38915\t60000\t2.12\t8" and got[10] == "c1\t40964\t43013\t2.12\t8"   # 2.125 prints as 2.12
    assert got[-1] == "c1\t49152\t60000\t2.00\t1" and len(got) == 15
    assert R.partition_gaps("\n".join(got) + "\n", [("c1", 60000)]) != []


def test_problematic_regions(tmp_path):
    # cells 20 20 4 1 9 29 1 40 36 40: sum 200, N = 5 -> chunk 40; 0.05 chunk = 2, 0.2 chunk = 8; nothing chopped (max 67.3)
    paths, fai = cohort(tmp_path, [[[20, 20, 4, 1, 9, 29, 1, 40, 36, 40]]], [("c1", 163000)])
    bed = tmp_path / "p.bed"
    # tiles 2, 3, 4; tile 6; an empty row (it would touch tile 0); another chromosome; a last line without its newline
    # (it would touch tile 9, whose 40 is above 0.05 chunk)
    bed.write_text("c1\t40000\t70000\nc1\t100000\t100001\nc1\t100\t100\nc9\t0\t999999\nc1\t150000\t160000")
    want = rows(
        ("c1", 0, 32768, "40.00", 1),
        # tile 2: 4 >= 2 under a region: int(0.5 + 4 / 20) = 0 -> 3 pieces of 5462
        ("c1", 32768, 38230, "1.33", 3), ("c1", 38230, 43692, "1.33", 3), ("c1", 43692, 49152, "1.33", 3),
        # tile 3: 1 < 2 and 1 < 8: carried; tile 4: 9 >= 2 writes what was carried, then 3 pieces
        ("c1", 49152, 65536, "1.00", 1),
        ("c1", 65536, 70998, "3.00", 3), ("c1", 70998, 76460, "3.00", 3), ("c1", 76460, 81920, "3.00", 3),
        # tile 5: 29 carried; tile 6: 1 < 2 under a region, 30 >= 8: written
        ("c1", 81920, 114688, "30.00", 1),
        ("c1", 114688, 131072, "40.00", 1),
        ("c1", 131072, 163000, "76.00", 1))
    assert R.indexsplit(paths, 5, fai=fai, problematic=str(bed)) == want
    # a tile at 0.05 chunk or above that is not above chunk / 4: one piece (nsplits 1), not three
    paths, fai = cohort(tmp_path, [[[2] * 10]], [("c1", 163000)])
    bed.write_text("c1:40001-50000\n")                       # chrom:start-end is 1-based: [40000, 50000), tiles 2 and 3
    want = rows(("c1", 0, 32768, "4.00", 1), ("c1", 32768, 49152, "2.00", 1), ("c1", 49152, 65536, "2.00", 1),
                ("c1", 65536, 98304, "4.00", 1), ("c1", 98304, 131072, "4.00", 1), ("c1", 131072, 163000, "4.00", 1))
    assert R.indexsplit(paths, 5, fai=fai, problematic=str(bed)) == want
    without = R.indexsplit(paths, 5, fai=fai)
    assert without == rows(*[("c1", 32768 * k, min(32768 * (k + 1), 163000), "4.00", 1) for k in range(5)])


def test_a_chopped_outlier(tmp_path):
    # 19 cells of 1 and one of 81: mean 5, variance 6080 / 19 = 320, 5 + 3 * 17.89 = 58.7 < 81: the cell becomes 40
    cells = [1] * 20
    cells[5] = 81
    paths, fai = cohort(tmp_path, [[cells]], [("c1", 327000)])
    assert R.indexsplit(paths, 1, fai=fai) == rows(("c1", 0, 327000, "59.00", 1))
    # N = 2: chunk 29.5; 40 is above it: int(0.5 + 40 / 14.75) = 3 pieces of 5462
    assert R.indexsplit(paths, 2, fai=fai) == rows(
        ("c1", 0, 81920, "5.00", 1),
        ("c1", 81920, 87382, "13.33", 3), ("c1", 87382, 92844, "13.33", 3), ("c1", 92844, 98304, "13.33", 3),
        ("c1", 98304, 327000, "14.00", 1))


def test_missing_and_empty_references_and_a_share_below_one_region(tmp_path):
    refs = [("c1", 80000), ("c2", 30000), ("c3", 5000), ("c4", 32000)]
    a = [[10, 10, 10, 10], [1, 1], [], [0, 0]]
    b = [[10, 10, 10, 10, 20]]                               # an index with one reference, and one tile more on it
    paths, fai = cohort(tmp_path, [a, b], refs)
    assert [len(s) for s in IR.read_bai(paths[0])[0]] == [4, 2, 0, 2] and len(IR.read_bai(paths[1])[0]) == 1
    # sums 100, 2, -, 0 of 102; N = 3: c1 int(2.94) = 2 -> chunk 50; c2 int(0.06) = 0 with data -> 1; c4 has no data
    want = rows(("c1", 0, 49152, "60.00", 1), ("c1", 49152, 80000, "40.00", 1),
                ("c2", 0, 30000, "2.00", 1),
                ("c3", 0, 5000, "0.00", 0),
                ("c4", 0, 32000, "0.00", 0))
    assert R.indexsplit(paths, 3, fai=fai) == want
    # the order of the arguments does not matter to these cells (every sum is exact), the row format does not change
    assert R.indexsplit(paths[::-1], 3, fai=fai) == want
    # a cohort without data has no defined split
    z, zf = cohort(tmp_path, [[[0, 0, 0]]], [("c1", 40000)])
    with pytest.raises(R.Fatal):
        R.indexsplit(z, 3, fai=zf)
    with pytest.raises(R.Fatal) as e:
        R.indexsplit(paths + [str(tmp_path / "x.crai")], 3, fai=fai)
    assert "x.crai" in str(e.value)


def test_float64_cells_follow_the_argument_order(tmp_path):
    # 2^53 + 1 bytes is not a double: the cell rounds the size first, then the quotient, then every sum
    big = 2 ** 53 + 1
    sizes = [[np.array([big, 3, 7], np.int64)], [np.array([1, 10 ** 9, 5], np.int64)], [np.array([12345678901], np.int64)]]
    got = R.cohort_sizes(sizes, 1)[0]
    want0 = float(big) / 1e9
    want0 = want0 + 1 / 1e9
    want0 = want0 + 12345678901 / 1e9
    assert float(big) == 2.0 ** 53 and got[0] == want0 and got[1] == 3 / 1e9 + 1.0 and got[2] == 7 / 1e9 + 5 / 1e9


# ---- the rows partition every reference ---------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 10, 100])
def test_rows_partition_a_synthetic_cohort(tmp_path, N):
    from tests.test_gpu_indexcov import CHROMS, synth_cohort
    paths, fai = synth_cohort(tmp_path / "cohort", 12, 77)
    refs = IR.read_fai(fai)
    assert [n for n, _ in refs] == CHROMS
    text = R.indexsplit(paths, N, fai=fai)
    assert R.partition_gaps(text, refs) == []
    assert len(text.splitlines()) >= len(CHROMS)
    with_p = tmp_path / "p.bed"
    with_p.write_text("1\t100000\t400000\nX\t0\t50000\n")
    text_p = R.indexsplit(paths, N, fai=fai, problematic=str(with_p))
    assert R.partition_gaps(text_p, refs) == [] and len(text_p.splitlines()) > len(text.splitlines())


@pytest.mark.parametrize("names", [["t.bam"], ["sample_issue_27_0001.bam"], ["t.bam", "sample_issue_27_0001.bam"]])
def test_rows_partition_the_reference_fixtures(names):
    # (hla.bam and t-empty.bam have no tile at all: the reference stops at "no usable chromsomes")
    for empty in ("hla.bam", "t-empty.bam"):
        with pytest.raises(R.Fatal):
            R.indexsplit([os.path.join(GOLD, empty)], 1)
    paths = [os.path.join(GOLD, n) for n in names]
    refs = IR.bam_header(paths[0])[1]
    # (N = 1: these references have a tile or two, and a split tile next to a reference's end meets the comparison with
    # len(size) + 1 -- test_the_comparison_with_len_plus_one_as_it_stands; such rows belong to the byte-equality tests)
    text = R.indexsplit(paths, 1)
    assert R.partition_gaps(text, refs) == [], text


# ---- the libraries ------------------------------------------------------------------------------------------------------
def test_abi_and_host_symbols_resolve():
    lib = _lib.load()
    names = [n for n in _lib.SYMBOLS if n.startswith("gd_indexsplit_")]
    assert sorted(names) == ["gd_indexsplit_add", "gd_indexsplit_begin", "gd_indexsplit_sums", "gd_indexsplit_timing"]
    for n in names:
        assert getattr(lib, n)
    import re
    hdr = open(os.path.join(ROOT, "include", "goleft_depth.h")).read()
    for n in names:
        assert re.search(r"\bint %s\(" % n, hdr), n
    assert lib.gd_abi_revision() == int(re.search(r"#define\s+GD_ABI_REVISION\s+(\d+)", hdr).group(1)) >= 2
    host = _hostlib.load()
    for n in ("gdh_indexsplit_main", "gdh_indexsplit_run", "gdh_samplename_main", "gdh_intervals_read_lines"):
        assert getattr(host, n)
    assert os.path.exists(os.path.join(ROOT, "goleft_amd", "indexsplit.py"))


def test_problematic_reader_drops_a_last_line_without_newline(tmp_path):
    import ctypes as C
    host = _hostlib.load()
    bed = tmp_path / "p.bed"
    bed.write_text("c1\t10\t20\nc1\t5\t5\nc1\t100\t200")
    h = C.c_void_p()
    assert host.gdh_intervals_read_lines(str(bed).encode(), C.byref(h)) == 0
    try:
        assert host.gdh_intervals_count(h, b"c1") == 1
        assert host.gdh_intervals_overlaps(h, b"c1", 19, 30) == 1 and host.gdh_intervals_overlaps(h, b"c1", 20, 30) == 0
        assert host.gdh_intervals_overlaps(h, b"c1", 100, 200) == 0
    finally:
        host.gdh_intervals_free(h)
    assert R.read_tree(str(bed)) == {"c1": [(10, 20)]}
    assert _hostlib.Intervals(str(bed)).count("c1") == 2     # ReadTree as `depth` has it is unchanged
