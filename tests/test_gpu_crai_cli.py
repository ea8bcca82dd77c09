"""GPU: `goleft-depth indexcov` and `indexsplit` on .crai indexes, end to end against their twins.  The twin of a .crai is
a .bai whose linear index holds the running sums of the tile sizes the restatement (tests/crai_ref.py) makes of the
.crai: both tools take the differences of consecutive entries, so the twin carries exactly those sizes, has the same
short name, and the tools must write the same bytes for both -- which the twin run is in turn held to the restatements
of the tools (tests/indexcov_ref.py, tests/indexsplit_ref.py) for.  Every CLI call runs under its own timeout."""
import gzip
import json
import os
import subprocess

import numpy as np
import pytest

from tests import covstats_ref as BR
from tests import crai_cases as CC
from tests import crai_ref as CR
from tests import indexcov_ref as IR
from tests import indexsplit_ref as SR
from tests.helpers import ROOT

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "goleft_amd", "goleft-depth")


def cli(word, args, timeout=300, env=None):
    r = subprocess.run([EXE, word] + [str(a) for a in args], capture_output=True, text=True, timeout=timeout,
                       env=dict(os.environ, **(env or {})))
    return r.returncode, r.stdout, r.stderr


def outputs(d):
    base = os.path.join(str(d), os.path.basename(str(d)) + "-indexcov")
    return gzip.decompress(open(base + ".bed.gz", "rb").read()).decode(), open(base + ".roc").read(), open(base + ".ped").read()


@pytest.fixture(scope="module")
def cohort(tmp_path_factory):
    d = tmp_path_factory.mktemp("crai")
    crais = CC.viral_variants(d)
    twins = [os.path.join(str(d), "twin", os.path.basename(p)[:-5] + ".bai") for p in crais]
    return crais, twins


@pytest.fixture(scope="module")
def indexcov_runs(cohort, tmp_path_factory):
    crais, twins = cohort
    d = tmp_path_factory.mktemp("cov")
    out = []
    for name, paths in (("a", crais), ("b", twins)):
        rc, _, err = cli("indexcov", ["-d", d / name / "out", "-f", CC.VIRAL_FAI] + paths)
        assert rc == 0, err
        out.append(outputs(d / name / "out"))
    return out


def test_indexcov_writes_the_same_bytes_for_crais_and_twins(indexcov_runs):
    (bed, roc, ped), (tbed, troc, tped) = indexcov_runs
    assert bed == tbed and roc == troc and ped == tped
    assert bed.splitlines()[0] == "#chrom\tstart\tend\tviral\tv1\tv2\tv3"
    assert bed.count("\n") > 150000 and ped.splitlines()[0].endswith("\tPC4") and "mapped" not in ped.splitlines()[0]
    rows = [ln.split("\t") for ln in bed.splitlines() if ln.startswith("21\t")]      # (reference 20 of the index)
    assert rows and all(r[5] == "0" for r in rows) and any(r[3] != "0" for r in rows)  # v2 has no slice there


def test_indexcov_twins_against_the_restatement(cohort, indexcov_runs, tmp_path):
    _, twins = cohort
    want = IR.indexcov(twins, str(tmp_path / "out"), fai=CC.VIRAL_FAI)
    bed, roc, ped = indexcov_runs[1]
    assert bed == want.bed and roc == want.roc
    got_rows, got_pcs = IR.strip_pcs(ped, want.n_front, want.n_pc)
    want_rows, want_pcs = IR.strip_pcs(want.ped, want.n_front, want.n_pc)
    assert got_rows == want_rows and want.n_pc == 4
    # (four samples: the fourth singular value of the centred matrix is 0 up to rounding and prints 0.00 on both sides)
    sign = np.sign((got_pcs * want_pcs).sum(axis=0))
    sign[sign == 0] = 1
    assert np.abs(got_pcs * sign - want_pcs).max() <= 0.01 + 1e-12


def test_indexsplit_prints_the_same_rows_for_crais_twins_and_the_restatement(cohort):
    crais, twins = cohort
    rc, out, err = cli("indexsplit", ["-n", 50, "--fai", CC.VIRAL_FAI] + crais)
    assert rc == 0, err
    rc, tout, err = cli("indexsplit", ["-n", 50, "--fai", CC.VIRAL_FAI] + twins)
    assert rc == 0, err
    assert out == tout and out.count("\n") > 50
    assert out == SR.indexsplit(twins, 50, fai=CC.VIRAL_FAI)


def test_python_entries_write_the_same_files(cohort, indexcov_runs, tmp_path):
    from goleft_amd import indexcov, indexsplit
    crais, _ = cohort
    assert indexcov.Main(["-d", str(tmp_path / "out"), "-f", CC.VIRAL_FAI] + crais) == 0
    assert outputs(tmp_path / "out") == indexcov_runs[0]
    assert indexsplit.Main(["-n", "50", "--fai", CC.VIRAL_FAI] + crais, out_path=str(tmp_path / "rows")) == 0
    rc, out, err = cli("indexsplit", ["-n", 50, "--fai", CC.VIRAL_FAI] + crais)
    assert rc == 0 and open(str(tmp_path / "rows")).read() == out


def test_a_cohort_may_mix_bam_bai_and_crai(tmp_path):
    refs = [("1", 400000), ("2", 300000)]
    recs = [BR.Rec(r, 150 * i, 0x3, 150 * i + 300, 500, ((0, 100),)) for r, n in ((0, 2500), (1, 1800)) for i in range(n)]
    bam = str(tmp_path / "first.bam")
    BR.write_bam(bam, refs, recs, block=4096)
    other = str(tmp_path / "second.bam")
    BR.write_bam(other, refs, recs[::2], block=4096)
    bai = str(tmp_path / "second.bai")
    os.rename(other + ".bai", bai)
    crai = CC.write_crai(tmp_path / "third.x.crai", b"".join(CC.line(s, 1 + 50000 * i, 50000, 40000 + 1000 * i) for s in (0, 1) for i in range(6)))
    d = tmp_path / "out"
    rc, _, err = cli("indexcov", ["-d", d, bam, bai, crai])
    assert rc == 0, err
    bed, roc, ped = outputs(d)
    assert bed.splitlines()[0].split("\t")[3:] == ["first", "second", "third-x"]           # argument order
    assert [ln.split("\t")[1] for ln in ped.splitlines()[1:]] == ["first", "second", "third-x"]
    third = [ln.split("\t")[5] for ln in bed.splitlines()[1:]]
    tiles = [v for s in CR.index_sizes(crai) for v in s]                                   # the .crai's tiles, on both references
    assert len(third) > 30 and sum(v != "0" for v in third) == sum(v > 0 for v in tiles) > 30
    rc, out, err = cli("indexsplit", ["-n", 10, bam, bai, crai])
    assert rc == 0 and out.count("\n") >= 2 and {ln.split("\t")[0] for ln in out.splitlines()} == {"1", "2"}, err


def test_timing_lines_split_the_index_reading(cohort, tmp_path):
    crais, _ = cohort
    rc, _, err = cli("indexcov", ["-d", tmp_path / "out", "-f", CC.VIRAL_FAI] + crais, env={"GOLEFT_INDEXCOV_TIMING": "1"})
    assert rc == 0, err
    t = json.loads([ln for ln in err.splitlines() if ln.startswith("{")][-1])
    print(t)
    assert t["samples"] == 4 and t["crai_read_s"] > 0 and t["crai_tile_s"] > 0 and t["index_read_s"] > 0
    rc, _, err = cli("indexsplit", ["-n", 50, "--fai", CC.VIRAL_FAI] + crais, env={"GOLEFT_INDEXSPLIT_TIMING": "1"})
    assert rc == 0, err
    t = json.loads(err.strip().splitlines()[-1])
    print(t)
    assert t["samples"] == 4 and t["crai_read_s"] > 0 and t["crai_tile_s"] > 0


def test_errors_name_the_argument_and_leave_nothing_behind(cohort, tmp_path):
    crais, _ = cohort
    plain = tmp_path / "plain.crai"
    plain.write_bytes(b"0\t1\t20000\t0\t0\t100\n")
    five = CC.write_crai(tmp_path / "five.crai", CC.line(0, 1, 20000, 9) * 2 + b"0\t1\t2\t3\t4\n" + CC.line(0, 50000, 20000, 9))
    unmapped = CC.write_crai(tmp_path / "unmapped.crai", CC.line(-1, 0, 0, 9) * 3)
    multi = CC.write_crai(tmp_path / "multi.crai", CC.line(0, 1, 20000, 9) + CC.line(-2, 1, 20000, 9))
    cases = [
        ([crais[0]], "viral.crai", None),                    # a .crai first without a .fai
        (["F", crais[0], str(plain)], "plain.crai", "gzip"),
        (["F", crais[0], five], "five.crai", "line 3"),
        (["F", unmapped, crais[0]], "unmapped.crai", "bad index"),
        (["F", crais[0], multi], "multi.crai", "line 2"),
        (["F", crais[0], str(tmp_path / "x.cram")], "x.cram", ".crai"),
    ]
    for k, (args, named, word) in enumerate(cases):
        d = tmp_path / ("o%d" % k)
        cov = ["-d", d] + [a for x in args for a in (["-f", CC.VIRAL_FAI] if x == "F" else [x])]
        rc, _, err = cli("indexcov", cov)
        assert rc == 1 and named in err and (word is None or word in err), (k, rc, err)
        assert not os.path.exists(os.path.join(str(d), "o%d-indexcov.ped" % k))
        split = ["-n", 50] + [a for x in args for a in (["--fai", CC.VIRAL_FAI] if x == "F" else [x])]
        rc, out, err = cli("indexsplit", split)
        assert rc == 1 and named in err and (word is None or word in err) and out == "", (k, rc, out, err)
