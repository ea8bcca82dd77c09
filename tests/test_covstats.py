"""CPU: `covstats` -- the Python restatement of covstats.go on hand-worked record lists, the host's row
(gdh_covstats_finish) byte for byte against it on random sampled arrays, and the .bai pseudo-bin reader."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

from tests import covstats_ref as R
from tests.helpers import ROOT

GOLD = os.path.join(ROOT, "tests", "golden", "ref")
M, I, D, S = 0, 1, 2, 4


@pytest.fixture(scope="module")
def hostlib():
    from goleft_amd import _hostlib
    return _hostlib.load()


def rec(flag=0x3, pos=100, next_pos=300, tlen=350, cigar=((M, 100),)):
    return R.Rec(0, pos, flag, next_pos, tlen, cigar)


# ---- the restatement, worked by hand ---------------------------------------------------------------------------------
def test_skip_boundary():
    recs = [rec(flag=0x4)] * 3 + [rec(next_pos=300 + i) for i in range(5)]
    s = R.bam_stats(recs, n=5, skip=3)
    assert s["counts"] == (0, 5, 0, 0, 5) and s["ins"] == [100, 101, 102, 103, 104]
    s = R.bam_stats(recs, n=5, skip=4)                      # one good record skipped as well
    assert s["counts"] == (0, 4, 0, 0, 4) and len(s["ins"]) == 4
    assert R.bam_stats(recs, n=5, skip=9)["skip_short"] and not R.bam_stats(recs, n=5, skip=8)["skip_short"]


def test_unmapped_not_counted_in_k_and_dup_vs_qcfail():
    recs = [rec(flag=0x4), rec(flag=0x4 | 0x400), rec(flag=0x400 | 0x1), rec(flag=0x200), rec(flag=0x600), rec()]
    s = R.bam_stats(recs, n=10, skip=0)
    assert s["counts"] == (2, 4, 3, 2, 1)                   # nU, k, nBad, nDup, nProper
    assert s["unmapped"] == 2 / 6 and s["bad"] == 3 / 6 and s["dup"] == 2 / 6 and s["proper"] == 1 / 6


def test_proper_counted_on_the_breaking_record_and_the_single_end_break():
    # n = 1: two sizes, then the third good record breaks (no insert yet) -- counted in k and nProper
    recs = [rec(flag=0x2, next_pos=0), rec(flag=0x0), rec(flag=0x2, next_pos=0), rec(flag=0x2, next_pos=0)]
    s = R.bam_stats(recs, n=1, skip=0)
    assert s["counts"] == (0, 3, 0, 0, 2) and s["sizes"] == [100, 100] and s["ins"] == []


def test_stored_cigar_and_query_length():
    recs = [rec(cigar=((S, 5), (M, 90), (I, 3), (D, 7), (7, 2))), rec(cigar=()), rec(cigar=((M, 50), (M, 50)))]
    s = R.bam_stats(recs, n=10, skip=0)
    assert s["sizes"] == [100, 0, 100] and s["ins"] == []    # none is a single M


def test_mad_filter_drops_the_largest_element_and_the_percentiles():
    assert R.mad_filter([1, 2, 3, 4, 5]) == [1, 2, 3, 4]     # nothing above the bound: the last index is cut
    assert R.mad_filter([10, 10, 10, 11, 1000]) == [10, 10, 10, 11]
    with pytest.raises(R.MadFilterPanic):
        R.mad_filter([5])
    with pytest.raises(R.MadFilterPanic):
        R.mad_filter([5, 6])
    recs = [rec(next_pos=100 + 100 + v) for v in range(21)]
    s = R.bam_stats(recs, n=21, skip=0)
    assert (s["pct5"], s["pct95"]) == (1, 19)               # int(0.05 * 20 + 0.5) = 1, int(0.95 * 20 + 0.5) = 19


def test_raw_counts_when_no_size_was_sampled():
    recs = [rec(flag=0x400 | 0x2), rec(flag=0x400), rec(flag=0x4)]
    s = R.bam_stats(recs, n=10, skip=0)
    row = R.format_row(s, 10, 100, "x.bam", "S")
    assert row.split("\t")[7:11] == ["0.00", "0.0", "200.0", "0.0"]


def test_regions_with_and_without_a_final_newline(tmp_path):
    p = tmp_path / "a.bed"
    p.write_text("c\t0\t100\nc\t200\t250\n")
    assert R.read_coverage(str(p)) == 150
    p.write_text("c\t0\t100\nc\t200\t250")
    assert R.read_coverage(str(p)) == 100


# ---- gdh_covstats_finish against the restatement -------------------------------------------------------------------------
class Values(C.Structure):
    _fields_ = [("lo", C.c_int64), ("n_bins", C.c_uint64), ("bins", C.c_void_p), ("n_overflow", C.c_uint64),
                ("overflow", C.c_void_p)]


def pack(arr, lo, n_bins, keep):
    a = np.asarray(arr, np.int64)
    win = (a >= lo) & (a < lo + n_bins)
    bins = np.bincount((a[win] - lo).astype(np.int64), minlength=n_bins).astype(np.uint64)
    ovf = a[~win].copy()
    np.random.default_rng(len(a)).shuffle(ovf)
    keep += [bins, ovf]
    return Values(lo, n_bins, bins.ctypes.data, len(ovf), ovf.ctypes.data)


def finish(hostlib, s, mapped, genome, lo=(0, -64, -64), nb=(256, 128, 128)):
    keep = []
    v = [pack(s["sizes"], lo[0], nb[0], keep), pack(s["ins"], lo[1], nb[1], keep), pack(s["tl"], lo[2], nb[2], keep)]
    cnt = (C.c_int64 * 5)(*s["counts"])
    buf = C.create_string_buffer(4096)
    n = hostlib.gdh_covstats_finish(cnt, C.byref(v[0]), C.byref(v[1]), C.byref(v[2]), mapped, genome, b"x.bam", b"S1,S2",
                                    buf, 4096)
    return n, buf.raw[:max(n, 0)].decode()


def random_records(rng, n):
    out = []
    rl = rng.choice([100, 150, 151])
    ins_mu = rng.choice([50, 300, 5000])
    for _ in range(n):
        f = int(rng.choice([0x3, 0x3, 0x3, 0x1, 0x4, 0x403, 0x203, 0x3 | 0x100, 0x3 | 0x800, 0x13]))
        pos = int(rng.integers(0, 1 << 20))
        kind = rng.random()
        if kind < 0.05:
            np_ = pos + int(rng.integers(-500, 500))         # overlapping mates: negative inserts
        elif kind < 0.08:
            np_ = pos + int(rng.integers(1, 1 << 28))        # gigabase outliers
        else:
            np_ = pos + rl + max(1, int(rng.normal(ins_mu, ins_mu / 8)))
        tl = int(rng.integers(-(1 << 30), 1 << 30)) if rng.random() < 0.03 else np_ - pos + rl
        cig = ((M, rl),) if rng.random() < 0.9 else ((S, 5), (M, rl - 5))
        out.append(rec(flag=f, pos=pos, next_pos=np_, tlen=tl, cigar=cig))
    return out


@pytest.mark.parametrize("seed", range(40))
def test_finish_is_byte_identical_to_the_restatement(hostlib, seed):
    rng = np.random.default_rng(seed)
    recs = random_records(rng, int(rng.integers(3, 3000)))
    n = int(rng.integers(3, 1500))
    s = R.bam_stats(recs, n=n, skip=int(rng.integers(0, 3)))
    mapped, genome = int(rng.integers(0, 1 << 40)), int(rng.integers(1, 1 << 33))
    got_n, got = finish(hostlib, s, mapped, genome)
    if len(s["ins"]) in (1, 2):
        assert got_n == -2
        return
    assert got == R.format_row(s, mapped, genome, "x.bam", "S1,S2")


def test_finish_at_rounding_ties_and_degenerate_rows(hostlib):
    # sizes whose mean lands on a %.2f tie: 0.125 * 100 = 12.5 -> "12.50"; inserts 1, 2, 3, 4 (mean of {1,2,3} = 2)
    for sizes, ins in (([1, 1, 1, 2] * 2, [1, 2, 3, 4]), ([0], []), ([], []), ([7] * 9, [0, 0, 0, 5, -5, 1 << 40])):
        s = R.bam_stats([], n=1, skip=0)
        s.update(sizes=sizes, ins=ins, tl=list(ins), counts=(3, len(sizes), 1, 1, 2))
        s.update(dup=1.0, proper=2.0)                       # the raw counts, unless sizes were sampled
        ss = sorted(sizes)
        if ss:
            tot = float(3 + len(sizes))
            s.update(bad=1 / tot, dup=1 / tot, proper=2 / tot, unmapped=3 / tot, rl_mean=R.mean_std(ss)[0], max_rl=ss[-1])
        if ins:
            si = sorted(ins)
            l = float(len(si) - 1)
            s.update(pct5=si[int(0.05 * l + 0.5)], pct95=si[int(0.95 * l + 0.5)])
            s["insert_mean"], s["insert_sd"] = R.mean_std(R.mad_filter(si))
            s["template_mean"], s["template_sd"] = R.mean_std(R.mad_filter(si))
        for genome in (1000, 0):
            n, got = finish(hostlib, s, 12345, genome)
            assert got == R.format_row(s, 12345, genome, "x.bam", "S1,S2"), (sizes, ins, genome)


@pytest.mark.parametrize("k", [1, 2])
def test_finish_refuses_one_or_two_inserts(hostlib, k):
    s = R.bam_stats([rec(next_pos=300 + i) for i in range(k)], n=10, skip=0)
    assert len(s["ins"]) == k
    assert finish(hostlib, s, 1, 1)[0] == -2


# ---- the .bai pseudo-bins ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,want", [("t.bam", [79980, 262]), ("hla.bam", [482, -1]), ("t-empty.bam", [-1, -1]),
                                       ("sample_issue_27_0001.bam", None)])
def test_bai_pseudo_bins(hostlib, name, want):
    path = os.path.join(GOLD, name)
    if want is None:
        want = [-1 if m is None else m for m in R.bai_mapped(path + ".bai")]
        assert len(want) == 180 and sum(want) == 6517502
    out = (C.c_int64 * 256)()
    n = C.c_size_t()
    assert hostlib.gdh_bai_mapped(path.encode(), out, 256, C.byref(n)) == 0
    assert list(out[:n.value]) == want


def test_bai_without_index_and_the_x_bai_name(hostlib, tmp_path):
    R.write_bam(str(tmp_path / "a.bam"), [("c", 1000)], [rec()])
    out = (C.c_int64 * 4)()
    n = C.c_size_t()
    assert hostlib.gdh_bai_mapped(str(tmp_path / "a.bam").encode(), out, 4, C.byref(n)) == 0 and list(out[:1]) == [1]
    os.rename(tmp_path / "a.bam.bai", tmp_path / "a.bai")
    assert hostlib.gdh_bai_mapped(str(tmp_path / "a.bam").encode(), out, 4, C.byref(n)) == 0 and list(out[:1]) == [1]
    os.remove(tmp_path / "a.bai")
    assert hostlib.gdh_bai_mapped(str(tmp_path / "a.bam").encode(), out, 4, C.byref(n)) == -1


def test_cli_prints_the_header_first_and_refuses_cram(tmp_path):
    exe = os.path.join(ROOT, "goleft_amd", "goleft-depth")
    r = subprocess.run([exe, "covstats", str(tmp_path / "x.cram")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and r.stdout == R.HEADER and "CRAM" in r.stderr
    r = subprocess.run([exe, "covstats"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and r.stdout == R.HEADER


def test_python_entry_refuses_cram(tmp_path):
    from goleft_amd import covstats
    out = tmp_path / "out.txt"
    assert covstats.Main([str(tmp_path / "x.cram")], out_path=str(out)) == 1
    assert out.read_text() == R.HEADER
