"""CPU: the .crai reader.  The restatement of the reference's ReadIndex / makeSizes (tests/crai_ref.py) against rows worked
out by hand and against the counts of the reference's own long-read fixture; the C++ reader (host/crai_reader.hpp, through
gdh_crai_read) slice for slice against the restatement, on the fixture and on small written files; and the device entry
that tiles the slices declared, bound and exported at ABI revision 3."""
import gzip
import os
import re

import pytest

from tests import crai_cases as CC
from tests import crai_ref as CR
from tests.helpers import ROOT

T = CR.T

HAND = [
    ([(10000, 20000, 100), (40000, 10000, 50)], [500, 500]),
    ([(1, 16384, 16384), (100000, 40000, 7)], [100000, 100000, 0, 0, 0, 0, 17, 17]),
    ([(1, 100000, 1000), (20000, 30000, 999), (120000, 20000, 40)], [1000] * 7 + [200]),      # four shifts, then skipped
    ([(1, 100000, 1000), (50000, 100000, 3000)], [1000] * 6 + [4462] * 4),                   # two shifts
    ([(5, 100, 9), (70000, 16384, 3)], [9000, 0, 0, 0, 18]),
    ([(16384, 16384, 1), (49152, 16383, 5), (65536, 16384, 2)], [6, 6, 30, 12]),
    ([(1, 0, 5), (20000, 16384, 8)], [0, 48]),
]


@pytest.mark.parametrize("k", range(len(HAND)))
def test_restatement_reproduces_the_hand_rows(k):
    slices, want = HAND[k]
    assert CR.make_sizes(slices) == (want, 0)


def test_restatement_counts_shifts_and_skips_of_the_hand_rows():
    st = {}
    CR.make_sizes(HAND[2][0], st)
    assert st == {"shifts": 4, "skipped": 1}
    st = {}
    CR.make_sizes(HAND[3][0], st)
    assert st == {"shifts": 2}


@pytest.fixture(scope="module")
def viral():
    return CR.read_index(CC.VIRAL)


def test_restatement_on_the_long_read_fixture(viral):
    text = gzip.open(CC.VIRAL, "rb").read()
    rows = text.split(b"\n")
    assert rows[-1] == b"" and len(rows) - 1 == 4374
    assert sum(r.split(b"\t")[0] == b"-1" for r in rows[:-1]) == 53
    assert len(viral) - 1 == 3421 and sum(1 for r in viral if r) == 98
    assert sum(len(r) for r in viral) == 4321 and max(len(r) for r in viral) == 335
    st = {}
    tiles = total = 0
    for r in viral:
        sizes, status = CR.make_sizes(r, st)
        assert status == 0
        tiles += len(sizes)
        total += sum(sizes)
    assert tiles == 191442
    assert st == {"shifts": 2640, "skipped": 27, "small": 107}
    assert 8.35e10 < total < 8.45e10


def test_host_reader_reads_the_fixture_as_the_restatement_does(viral):
    assert CC.host_read(CC.VIRAL) == viral


GOOD = CC.line(0, 1, 20000, 100) + CC.line(-1, 0, 0, 55) + CC.line(2, 5, 70000, 9) + CC.line(0, 20001, 30000, 7)


def both(path):
    """(what the host reader returns or its refusal's line, the same of the restatement)"""
    def run(f):
        try:
            return f(path)
        except CR.CraiError as e:
            return ("refused", e.line)
    return run(CC.host_read), run(CR.read_index)


def agree(tmp_path, text, members=1):
    p = CC.write_crai(tmp_path / ("c%d.crai" % len(os.listdir(str(tmp_path)))), text, members)
    got, want = both(p)
    assert got == want, (text[-200:], got, want)
    return want


def test_host_reader_on_small_files(tmp_path):
    assert agree(tmp_path, GOOD) == [[(1, 20000, 100), (20001, 30000, 7)], [], [(5, 70000, 9)]]
    assert agree(tmp_path, GOOD * 40, members=5) == agree(tmp_path, GOOD * 40)          # several gzip members
    assert len(agree(tmp_path, GOOD + b"0\t90000\t100\t0\t0\t8")[0]) == 2               # a last line without its newline
    assert agree(tmp_path, b"  " + GOOD[:-1] + b" \t \r\n")[0][1] == (20001, 30000, 7)  # white space around a line
    assert agree(tmp_path, b"-1\t5\t6\t7\t8\t9\n" + GOOD)[2] == [(5, 70000, 9)]                  # an unmapped line first
    # a negative span in the middle ends the reading: what came before is kept, and that reference is already listed
    want = agree(tmp_path, GOOD + CC.line(4, 7, -1, 3) + CC.line(0, 99999, 5, 5))
    assert want == [[(1, 20000, 100), (20001, 30000, 7)], [], [(5, 70000, 9)], [], []]
    assert agree(tmp_path, b"") == []
    assert agree(tmp_path, b"\n") == ("refused", 1)                                     # an empty line is one field
    assert agree(tmp_path, GOOD + b"0\t1\t2\t3\t4\n") == ("refused", 5)                 # five fields
    assert agree(tmp_path, GOOD + b"0\t1\t2\t3\t4\t5\t6\n") == ("refused", 5)
    assert agree(tmp_path, GOOD + b"0\t1\t2\t3\t4\t\n") == ("refused", 5)               # (the trailing tab is trimmed)
    for k in range(6):
        t = [b"0", b"1", b"2", b"3", b"4", b"5"]
        t[k] = b"1x"
        assert agree(tmp_path, GOOD[:len(CC.line(0, 1, 20000, 100))] + b"\t".join(t) + b"\n") == ("refused", 2)
    assert agree(tmp_path, b"0\t\t2\t3\t4\t5\n") == ("refused", 1)
    assert agree(tmp_path, b"0\t1.5\t2\t3\t4\t5\n") == ("refused", 1)
    assert agree(tmp_path, b"0\t0x10\t2\t3\t4\t5\n") == ("refused", 1)
    assert agree(tmp_path, b"0\t+7\t2\t3\t4\t-0\n") == [[(7, 2, 0)]]                    # (Atoi takes a sign)
    assert agree(tmp_path, b"0\t1\t2\t99999999999999999999\t4\t5\n") == ("refused", 1)  # beyond int64
    assert agree(tmp_path, b"-1\tnot\tlooked\tat\n") == ("refused", 1)                  # (the field count comes first)
    assert agree(tmp_path, b"-1\tnot\tlooked\tat\tat\tall\n" + GOOD)[0][0] == (1, 20000, 100)


@pytest.mark.parametrize("text,line", [
    (GOOD + CC.line(-2, 1, 2, 3), 5),                        # htslib's multi-reference slices
    (CC.line(1 << 20, 1, 2, 3), 1),
    (GOOD + GOOD + CC.line(0, 1 << 31, 2, 3), 9),
    (CC.line(0, -(1 << 31), 2, 3), 1),
    (CC.line(0, 1, 1 << 31, 3), 1),
    (CC.line(0, 1, 2, 1 << 31), 1),
    (CC.line(0, 1, 2, -(1 << 31) - 1), 1),
])
def test_host_reader_refuses_what_is_outside_the_bounds(tmp_path, text, line):
    assert agree(tmp_path, text) == ("refused", line)


def test_host_reader_takes_the_bounds_themselves(tmp_path):
    text = CC.line((1 << 20) - 1, (1 << 31) - 1, (1 << 31) - 1, (1 << 31) - 1) + CC.line(0, -(1 << 31) + 1, 0, -(1 << 31))
    want = agree(tmp_path, text)
    assert want[0] == [(-(1 << 31) + 1, 0, -(1 << 31))] and want[-1] == [((1 << 31) - 1,) * 3] and len(want) == 1 << 20


def test_host_reader_refuses_what_is_not_gzip(tmp_path):
    p = tmp_path / "plain.crai"
    p.write_bytes(GOOD)
    assert both(str(p)) == (("refused", 0), ("refused", 0))
    assert both(str(tmp_path / "missing.crai")) == (("refused", 0), ("refused", 0))
    cut = tmp_path / "cut.crai"
    cut.write_bytes(gzip.compress(GOOD * 200, mtime=0)[:-20])
    assert both(str(cut)) == (("refused", 0), ("refused", 0))


def test_device_entry_is_declared_bound_and_exported_at_revision_3():
    from goleft_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "goleft_depth.h")).read()
    assert "gd_crai_sizes" in _lib.SYMBOLS and re.search(r"\bint gd_crai_sizes\(", hdr)
    assert int(re.search(r"#define\s+GD_ABI_REVISION\s+(\d+)", hdr).group(1)) == 3 == lib.gd_abi_revision()
    assert int(re.search(r"#define\s+GD_ABI_VERSION\s+(\d+)", hdr).group(1)) == 15 == lib.gd_abi_version()
    assert lib.gd_crai_sizes is not None
    from goleft_amd import _hostlib
    assert "gdh_crai_read" in _hostlib.SYMBOLS and _hostlib.load().gdh_crai_read is not None
