"""GPU: `goleft-depth emdepth` on a 9-sample, 40-row integer matrix -- plain, gzipped, with --scales, in blocks of 7
rows, and through goleft_amd.emdepth.Main -- text for text against the copy numbers of the restatement
(tests/emdepth_ref.py); tests/test_emdepth_ref.py asserts on the CPU that no cell of this matrix sits on an adjustCN
margin, so every cell is compared.  Then the error exits.  Every call runs under its own timeout; nothing is retried."""
import gzip
import os
import subprocess

import numpy as np
import pytest

from tests import emdepth_ref as R
from tests import emdepth_shapes as S
from tests.helpers import ROOT

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "goleft_amd", "goleft-depth")
HEADER = "#chrom\tstart\tend\t" + "\t".join("s%d" % i for i in range(9))


def matrix_text(cells, header=HEADER):
    rows = ["chr%d\t%d\t%d\t%s" % (1 + i // 25, (i % 25) * 1000, (i % 25 + 1) * 1000, "\t".join(str(v) for v in row))
            for i, row in enumerate(cells.tolist())]
    return header + "\n" + "\n".join(rows) + "\n"


def expected_text(cells, scale=None):
    ref = R.em_matrix(R.cells_to_depths(cells, scale))
    assert all(not R.pair_excluded(a, b) for r in ref for a, b in r.pairs.values())
    return matrix_text(np.array([r.cn for r in ref]))


def run(args, env=None):
    return subprocess.run([EXE, "emdepth"] + args, capture_output=True, text=True, timeout=120,
                          env=dict(os.environ, **(env or {})))


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("emdepth")
    cells = S.cli_cells()
    plain, gz, scales = d / "m.bed", d / "m.bed.gz", d / "scales.txt"
    plain.write_text(matrix_text(cells))
    with gzip.open(gz, "wt") as f:
        f.write(matrix_text(cells))
    scales.write_text("".join("%r\n" % v for v in S.CLI_SCALES))
    return d, cells, str(plain), str(gz), str(scales)


def test_plain_gz_and_blocks(files):
    d, cells, plain, gz, _ = files
    want = expected_text(cells)
    p = run([plain])
    assert p.returncode == 0, p.stderr
    assert p.stdout == want
    p = run([gz])
    assert p.returncode == 0 and p.stdout == want, p.stderr
    p = run([plain], {"GOLEFT_EMDEPTH_ROWS": "7", "GOLEFT_EMDEPTH_TIMING": "1"})
    assert p.returncode == 0 and p.stdout == want, p.stderr
    assert '"kernel_s"' in p.stderr and '"block_rows": 7' in p.stderr


def test_scales_and_python_entry(files):
    d, cells, plain, gz, scales = files
    want = expected_text(cells, np.array(S.CLI_SCALES, np.float32))
    assert want != expected_text(cells)
    p = run(["--scales", scales, gz])
    assert p.returncode == 0 and p.stdout == want, p.stderr
    from goleft_amd import emdepth
    out = str(d / "out.bed")
    assert emdepth.Main(["--scales=" + scales, plain], out_path=out) == 0
    with open(out) as f:
        assert f.read() == want


def test_error_exits(files):
    d, cells, plain, gz, scales = files
    assert run([]).returncode == 255
    assert run(["--nope", plain]).returncode == 255
    p = run([str(d / "missing.bed")])
    assert p.returncode == 1 and "cannot open" in p.stderr
    two = d / "two.bed"
    two.write_text("#chrom\tstart\tend\ta\tb\nchr1\t0\t10\t1\t2\n")
    p = run([str(two)])
    assert p.returncode == 1 and p.stdout == "" and "2 samples" in p.stderr and "median" in p.stderr
    short = d / "short.bed"
    short.write_text(matrix_text(cells[:3]).rsplit("\t", 1)[0] + "\n")           # the last row loses a column
    p = run([str(short)])
    assert p.returncode == 1 and p.stdout == "" and "line 4 has 11 columns, the header has 12" in p.stderr
    for cell in ("x", "-1", "nan", "1e50", ""):
        bad = d / "bad.bed"
        bad.write_text(matrix_text(cells[:2]).rsplit("\t", 1)[0] + "\t" + cell + "\n")      # the last cell of line 3
        p = run([str(bad)])
        assert p.returncode == 1 and p.stdout == "" and "line 3: column 12" in p.stderr, (cell, p.stderr)
    few = d / "few.txt"
    few.write_text("1\n2\n")
    p = run(["--scales", str(few), plain])
    assert p.returncode == 1 and "2 factors" in p.stderr
    nohdr = d / "nohdr.bed"
    nohdr.write_text("chr1\t0\t10\t1\t2\t3\n".replace("chr1", "1"))
    assert run([str(nohdr)]).returncode == 1
