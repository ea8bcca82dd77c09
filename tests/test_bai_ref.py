"""CPU: the .bai model (tests/bai_ref.py) against the indexes htslib wrote, and the host's index arithmetic
(gdh_bai_assemble, goleft_amd/csrc/host/index_host.cpp: bin compression, chunk merge, linear fill, layout) against the
model on runs that sit on the edges of those rules.  No device: the runs, windows and counts are given."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import bai_ref
from tests import helpers as H

REF = os.path.join(H.GOLDEN, "ref")
UNSET = bai_ref.UNSET


@pytest.mark.parametrize("name", ["t", "hla", "t-empty"])
def test_the_model_reproduces_htslibs_indexes(name):
    bam = os.path.join(REF, name + ".bam")
    assert bai_ref.build(bam) == open(bam + ".bai", "rb").read()


def test_the_fixtures_pin_what_the_issue_says_they_pin():
    lens, recs, size = bai_ref.read(os.path.join(REF, "t.bam"))
    runs, lin, meta, n_no_coor = bai_ref.scan(len(lens), recs)
    assert len(recs) == 80330 and len(lens) == 2 and n_no_coor == 64
    assert sum(m[3] for m in meta if m) > 0                  # reads with flag 4 that are filed under a reference
    assert recs[-1][5] == size << 16                         # the last record ends at the file's size
    # reference 1 of t.bam: a level-5 bin that moved into its level-4 parent
    before = {b for r, b, _, _ in runs if r == 1}
    d = open(os.path.join(REF, "t.bam.bai"), "rb").read()
    assert {bai_ref.bin_level(b) for b in before} >= {4, 5}
    assert bai_ref.assemble(len(lens), runs, lin, meta, n_no_coor) == d


def assemble(n_ref, runs, lin, meta, n_no_coor, windows=12):
    """gdh_bai_assemble on the model's inputs: `windows` windows per reference, untouched ones all ones."""
    from goleft_amd import _hostlib, _lib
    lib = _hostlib.load()
    r = (_lib.GdIndexRun * max(1, len(runs)))()
    for k, (ref, b, vb, ve) in enumerate(runs):
        r[k] = _lib.GdIndexRun(ref, b, vb, ve)
    lin_off = np.arange(n_ref + 1, dtype=np.uint64) * np.uint64(windows)
    flat = np.full(n_ref * windows + 1, UNSET, np.uint64)
    for t in range(n_ref):
        for w, v in lin[t].items():
            flat[t * windows + w] = v
    refs = (_lib.GdIndexRef * max(1, n_ref))()
    for t in range(n_ref):
        if meta[t] is not None:
            refs[t] = _lib.GdIndexRef(*meta[t])
    args = (n_ref, C.addressof(r), len(runs), lin_off.ctypes.data, flat.ctypes.data, C.addressof(refs), n_no_coor)
    need = lib.gdh_bai_assemble(*args, None, 0)
    assert need > 0
    out = np.zeros(need, np.uint8)
    assert lib.gdh_bai_assemble(*args, out.ctypes.data, need) == need
    return out.tobytes()


def V(coff, uoff=0):
    return (coff << 16) | uoff


def _meta(runs, n_ref):
    meta = [None] * n_ref
    for ref, _b, vb, ve in runs:
        if meta[ref] is None:
            meta[ref] = [vb, ve, 3, 1]
        meta[ref][1] = ve
    return meta


L5, L4, L3 = 4681, 585, 73                                    # the first bin of levels 5, 4 and 3: each the first child of the next

CASES = {
    # a level-5 bin spanning 65535 compressed bytes, its parent present: it moves up (and meets nothing there)
    "parent-below": [(0, L4, V(10), V(20)), (0, L5, V(1000), V(1000 + 65535, 7))],
    # ... spanning exactly 65536: it stays
    "parent-at": [(0, L4, V(10), V(20)), (0, L5, V(1000), V(1000 + 65536))],
    # the same two without the parent: both stay, whatever they span
    "orphan-below": [(0, L5 + 9, V(10), V(20)), (0, L5, V(1000), V(1000 + 65535, 7))],
    "orphan-at": [(0, L5 + 9, V(10), V(20)), (0, L5, V(1000), V(1000 + 65536))],
    # 5 -> 4 -> 3: the level-4 bin, grown by its child, is still small and moves on
    "chain": [(0, L3, V(5), V(6)), (0, L4, V(10), V(20)), (0, L5, V(30), V(40)), (0, L5 + 1, V(50), V(60))],
    # ... but not once the child has made it span 65536
    "chain-stops": [(0, L3, V(5), V(6)), (0, L4, V(10), V(20)), (0, L5, V(30), V(10 + 65536))],
    # two chunks of one bin that meet inside one member (>=: merged) and in neighbouring members (<: kept apart)
    "merge-ge": [(0, L5, V(100), V(200, 5)), (0, L5 + 1, V(200, 5), V(200, 9)), (0, L5, V(200, 9), V(300))],
    "merge-lt": [(0, L5, V(100), V(199, 5)), (0, L5 + 1, V(199, 5), V(200, 9)), (0, L5, V(200, 9), V(300))],
    # a merge that keeps the LARGER end (chunks out of order after a child joined its parent)
    "merge-larger-end": [(0, L4, V(10), V(500)), (0, L5, V(20), V(30)), (0, L4, V(500), V(600))],
    # a reference without records between two that have some
    "gap": [(0, L5, V(10), V(20)), (2, L5 + 3, V(20), V(30))],
    # level 1 into bin 0, where the three chunks then meet end to begin
    "bin0": [(0, 0, V(10), V(20)), (0, 1, V(20), V(30)), (0, 0, V(30), V(40))],
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_assemble_matches_the_model(name):
    runs = CASES[name]
    n_ref = 3
    meta = _meta(runs, n_ref)
    lin = [dict() for _ in range(n_ref)]
    for ref, _b, vb, _ve in runs:
        lin[ref].setdefault(0, vb)
    want = bai_ref.assemble(n_ref, runs, lin, meta, 7)
    assert assemble(n_ref, runs, lin, meta, 7) == want
    # and the case is the case: what the rule under test must have done to the bins of reference 0
    bins = _bins(want)[0]
    expect = {"parent-below": {L4: 2}, "parent-at": {L4: 1, L5: 1}, "orphan-below": {L5: 1, L5 + 9: 1}, "orphan-at": {L5: 1, L5 + 9: 1},
              "chain": {L3: 4}, "chain-stops": {L3: 1, L4: 2}, "merge-ge": {L5: 1, L5 + 1: 1}, "merge-lt": {L5: 2, L5 + 1: 1},
              "merge-larger-end": {L4: 1}, "gap": {L5: 1}, "bin0": {0: 1}}[name]
    assert {b: n for b, n in bins.items() if b != bai_ref.PSEUDO_BIN} == expect


def _bins(bai):
    """[{bin: chunk count}] per reference of a .bai."""
    import struct
    n_ref, = struct.unpack_from("<i", bai, 4)
    p, out = 8, []
    for _ in range(n_ref):
        n_bin, = struct.unpack_from("<i", bai, p)
        p += 4
        d = {}
        for _ in range(n_bin):
            b, n = struct.unpack_from("<Ii", bai, p)
            d[b] = n
            p += 8 + 16 * n
        n_intv, = struct.unpack_from("<i", bai, p)
        p += 4 + 8 * n_intv
        out.append(d)
    return out


@pytest.mark.parametrize("touched", [{0: 5}, {3: 5}, {0: 5, 3: 9}, {1: 5, 2: 6, 7: 9, 11: 12}, {11: 4}, {}])
def test_linear_index_trailing_and_interior_unset_windows(touched):
    runs = [(1, L5, V(4), V(13))] if touched else []
    meta = _meta(runs, 2)
    lin = [dict(), {w: V(v) for w, v in touched.items()}]
    want = bai_ref.assemble(2, runs, lin, meta, 0)
    assert assemble(2, runs, lin, meta, 0) == want


def test_bins_come_out_ascending_with_the_pseudo_bin_last():
    runs = [(0, b, V(10 + 200000 * k), V(10 + 200000 * k + 70000)) for k, b in enumerate((4700, 1, 600, 0, 80, 4690, 9))]   # (too wide to move)
    meta = _meta(runs, 1)
    want = bai_ref.assemble(1, runs, [{}], meta, 0)
    assert assemble(1, runs, [{}], meta, 0) == want
    assert list(_bins(want)[0]) == [0, 1, 9, 80, 600, 4690, 4700, bai_ref.PSEUDO_BIN]


def test_assemble_refuses_what_is_no_input():
    from goleft_amd import _hostlib, _lib
    lib = _hostlib.load()
    r = (_lib.GdIndexRun * 2)(_lib.GdIndexRun(1, L5, 1, 2), _lib.GdIndexRun(0, L5, 2, 3))      # references out of order
    lin_off = np.zeros(3, np.uint64)
    refs = (_lib.GdIndexRef * 2)()
    assert lib.gdh_bai_assemble(2, C.addressof(r), 2, lin_off.ctypes.data, None, C.addressof(refs), 0, None, 0) == -1
    r[0].ref, r[1].ref = 0, 5                                                                    # a reference that does not exist
    assert lib.gdh_bai_assemble(2, C.addressof(r), 2, lin_off.ctypes.data, None, C.addressof(refs), 0, None, 0) == -1
