"""GPU: `goleft-depth scales` and `goleft-depth emdepth --normalize` on a 9-sample, 40-row integer matrix whose samples
sit at nine different levels -- text for text against the restatements (tests/scales_ref.py for the factors,
tests/emdepth_ref.py for the copy numbers).  Before anything is compared the matrix is held, on the CPU, to what makes
the text comparable: no cell on an adjustCN margin, every row's comparisons wider than 1e-9 relative, and copy numbers
that differ from the unnormalised run's.  Every call runs under its own timeout; nothing is retried."""
import functools
import gzip
import os
import subprocess

import numpy as np
import pytest

from tests import emdepth_ref as R
from tests import emdepth_shapes as ES
from tests import scales_ref as SR
from tests.helpers import ROOT

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "goleft_amd", "goleft-depth")
NAMES = ["s%d" % i for i in range(9)]
HEADER = "#chrom\tstart\tend\t" + "\t".join(NAMES)
LEVELS = (1.0, 0.5, 2.0, 1.25, 0.8, 1.0, 1.5, 3.0, 0.9)
MEDIANS = [51, 22, 112, 61, 59, 43, 84, 138, 43]
NONZERO = [36, 39, 35, 35, 37, 33, 36, 36, 36]


def cli_cells():
    # (seeds 500 and 501 hold an exact tie)
    return np.floor(ES.integer_rows(502, 40, 9) * np.array(LEVELS)).astype(np.int64)


def matrix_text(cells, header=HEADER):
    rows = ["chr%d\t%d\t%d\t%s" % (1 + i // 25, (i % 25) * 1000, (i % 25 + 1) * 1000, "\t".join(str(v) for v in row))
            for i, row in enumerate(np.asarray(cells).tolist())]
    return header + "\n" + "\n".join(rows) + "\n"


@functools.lru_cache(maxsize=None)
def factors(level=None):
    """(factors, their lines) of the restatement"""
    med, nz = SR.sample_medians(cli_cells().astype(np.float32))
    assert med.tolist() == MEDIANS and nz.tolist() == NONZERO
    assert SR.level_of(med) == 59
    scale = SR.scales(med, level)
    return scale, SR.scale_lines(scale)


@functools.lru_cache(maxsize=None)
def copy_numbers(level=None):
    """the copy-number text of the restatement for the normalised matrix, held to the three conditions first"""
    cells = cli_cells()
    ref = R.em_matrix(R.cells_to_depths(cells, factors(level)[0]))
    assert all(not R.pair_excluded(a, b) for r in ref for a, b in r.pairs.values())
    assert min(r.gap for r in ref) > 1e-9
    text = matrix_text(np.array([r.cn for r in ref]))
    assert text != matrix_text(np.array([r.cn for r in R.em_matrix(R.cells_to_depths(cells))]))
    return text


def run(cmd, args, env=None):
    return subprocess.run([EXE, cmd] + args, capture_output=True, text=True, timeout=120, env=dict(os.environ, **(env or {})))


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("scales")
    cells = cli_cells()
    plain, gz = d / "m.bed", d / "m.bed.gz"
    plain.write_text(matrix_text(cells))
    with gzip.open(gz, "wt") as f:
        f.write(matrix_text(cells))
    return d, cells, str(plain), str(gz)


def test_scales_writes_the_restatements_factors(files):
    d, cells, plain, gz = files
    scale, lines = factors()
    for path in (plain, gz):
        p = run("scales", [path], {"GOLEFT_EMDEPTH_TIMING": "1"})
        assert p.returncode == 0, p.stderr
        assert p.stdout == lines
        err = p.stderr.split("\n")
        assert err[:9] == ["%s\t%d\t%d" % (NAMES[s], MEDIANS[s], NONZERO[s]) for s in range(9)]
        assert '"medians_kernels_s"' in p.stderr and '"medians_passes": 4' in p.stderr
    # what --scales reads back is the float32, bit for bit
    back = np.array([np.float32(float(v)) for v in lines.split()], np.float32)
    assert np.array_equal(back.view(np.uint32), scale.view(np.uint32))


def test_level_one_gives_the_reciprocals(files):
    d, cells, plain, gz = files
    p = run("scales", ["--level", "1", plain])
    assert p.returncode == 0, p.stderr
    assert p.stdout == "".join("%.9g\n" % float(np.float32(1.0 / m)) for m in MEDIANS)
    assert p.stdout == factors(1.0)[1]
    p = run("scales", ["--level=59", gz])
    assert p.returncode == 0 and p.stdout == factors()[1], p.stderr


def test_normalize_is_scales_then_emdepth(files):
    d, cells, plain, gz = files
    lines, want = factors()[1], copy_numbers()
    f = d / "f.txt"
    p = run("scales", [plain])
    assert p.returncode == 0, p.stderr
    f.write_text(p.stdout)
    two = run("emdepth", ["--scales", str(f), plain])
    assert two.returncode == 0, two.stderr
    one = run("emdepth", ["--normalize", plain])
    assert one.returncode == 0, one.stderr
    assert one.stdout == two.stdout
    assert one.stdout == want
    p = run("emdepth", ["--normalize", gz], {"GOLEFT_EMDEPTH_ROWS": "7", "GOLEFT_EMDEPTH_TIMING": "1"})
    assert p.returncode == 0 and p.stdout == want, p.stderr
    assert '"medians_kernels_s"' in p.stderr and '"block_rows": 7' in p.stderr
    # a level of its own: the same factors as `scales --level`
    p = run("emdepth", ["--normalize", "--level", "30", plain])
    assert p.returncode == 0 and p.stdout == copy_numbers(30.0), p.stderr


def test_normalize_with_cnvs_and_the_python_entries(files):
    d, cells, plain, gz = files
    lines, want = factors()[1], copy_numbers()
    f, c1, c2, c3 = d / "f2.txt", str(d / "c1.tsv"), str(d / "c2.tsv"), str(d / "c3.tsv")
    from goleft_amd import emdepth
    assert emdepth.Scales([plain], out_path=str(f)) == 0
    assert f.read_text() == lines
    one = run("emdepth", ["--normalize", "--cnvs", c1, plain])
    assert one.returncode == 0 and one.stdout == want, one.stderr
    two = run("emdepth", ["--scales", str(f), "--cnvs", c2, gz], {"GOLEFT_EMDEPTH_ROWS": "7"})
    assert two.returncode == 0 and two.stdout == want, two.stderr
    with open(c1) as a, open(c2) as b:
        calls = a.read()
        assert calls == b.read() and calls.startswith("#sample\t")
    out = str(d / "out.bed")
    assert emdepth.Main(["--normalize", "--cnvs=" + c3, plain], out_path=out) == 0
    with open(out) as a, open(c3) as b:
        assert a.read() == want and b.read() == calls


def test_error_exits(files):
    d, cells, plain, gz = files
    zero = cells.copy()
    zero[:, 4] = 0
    zpath = d / "zero.bed"
    zpath.write_text(matrix_text(zero))
    for p in (run("scales", [str(zpath)]), run("emdepth", ["--normalize", str(zpath)])):
        assert p.returncode == 1 and p.stdout == "" and "sample s4" in p.stderr, p.stderr
    assert run("emdepth", [str(zpath)]).returncode == 0                       # without the flag nothing changed
    f = d / "f3.txt"
    f.write_text(factors()[1])
    p = run("emdepth", ["--normalize", "--scales", str(f), plain])
    assert p.returncode == 255 and p.stdout == "" and "--normalize" in p.stderr
    for level in ("0", "-1", "nan", "inf", "x", ""):
        assert run("scales", ["--level=" + level, plain]).returncode == 255, level
        assert run("emdepth", ["--normalize", "--level=" + level, plain]).returncode == 255, level
    p = run("emdepth", ["--level", "2", plain])
    assert p.returncode == 255 and p.stdout == "" and "--normalize" in p.stderr
    assert run("scales", []).returncode == 255
    assert run("scales", ["--normalize", plain]).returncode == 255            # emdepth's flags are not scales'
    assert run("scales", ["--cnvs", "x", plain]).returncode == 255
    p = run("scales", [str(d / "missing.bed")])
    assert p.returncode == 1 and "cannot open" in p.stderr
    # the same reader, the same whole-file check, the same refusals as emdepth's
    two = d / "two.bed"
    two.write_text("#chrom\tstart\tend\ta\tb\nchr1\t0\t10\t1\t2\n")
    assert run("emdepth", [str(two)]).returncode == 1
    p = run("scales", [str(two)])
    assert p.returncode == 1 and p.stdout == "" and "2 samples" in p.stderr
    bad = d / "bad.bed"
    bad.write_text(matrix_text(cells[:2]).rsplit("\t", 1)[0] + "\t-1\n")       # the last cell of line 3
    p = run("scales", [str(bad)])
    assert p.returncode == 1 and p.stdout == "" and "line 3: column 12" in p.stderr
    empty = d / "empty.bed"
    empty.write_text(HEADER + "\n")
    p = run("scales", [str(empty)])
    assert p.returncode == 1 and p.stdout == "" and "no rows" in p.stderr
