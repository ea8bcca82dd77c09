"""`goleft-depth emdepth --cnvs` on a 9-sample, 40-row integer matrix over two chromosomes -- plain, gzipped, with
--scales, in blocks of 7 rows -- text for text against the restatement of emdepth.Cache (tests/emcnv_ref.py).  The
first test runs on the CPU and holds the matrix to what makes the text comparable: no cell near a state threshold, no
adjustCN margin, every row's comparisons wide, and no log2fc within 1e-5 of a tie of %.2f.  Every call runs under its
own timeout; nothing is retried."""
import gzip
import os
import subprocess

import numpy as np
import pytest

from tests import emcnv_shapes as S
from tests import emdepth_ref as R
from tests import emdepth_shapes as ES
from tests.helpers import ROOT

EXE = os.path.join(ROOT, "goleft_amd", "goleft-depth")
HEADER = "#chrom\tstart\tend\t" + "\t".join(S.CLI_NAMES)


def matrix_text(cells, where=None):
    where = where or S.cli_where()
    return HEADER + "\n" + "".join("%s\t%d\t%d\t%s\n" % (where[i] + ("\t".join(str(v) for v in row),))
                                    for i, row in enumerate(np.asarray(cells).tolist()))


def stdout_text(res):
    return matrix_text(np.array([r.cn for r in res.rows]))


@pytest.mark.parametrize("scaled", (False, True))
def test_the_matrix_can_be_compared_as_text(scaled):
    res = S.cli_reference(scaled)
    assert res.near == []
    # (unscaled, the depths are integers: lambda is bit for bit whatever ties a row holds, as emdepth_shapes.plan has it)
    assert not scaled or all(r.gap > ES.GAP for r in res.rows)
    assert all(not R.pair_excluded(a, b) for r in res.rows for a, b in r.pairs.values())
    assert len(res.cnvs) >= 4 and any(c.sample == 0 for c in res.cnvs)
    fc = np.array([v for c in res.cnvs for v in c.log2fc], np.float64)
    assert np.isneginf(fc).any()
    fin = fc[np.isfinite(fc)] * 100.0
    assert np.all(np.abs(fin - np.floor(fin) - 0.5) > 1e-3)             # 1e-5 in log2fc
    text = S.cli_text(res)
    assert "-Inf" in text and "chr1:24000-25000,chr2:0-1000" not in text    # the boundary is a gap for this matrix


def run(args, env=None):
    return subprocess.run([EXE, "emdepth"] + args, capture_output=True, text=True, timeout=120,
                          env=dict(os.environ, **(env or {})))


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("emcnv")
    cells = S.cli_cells()
    plain, gz, scales = d / "m.bed", d / "m.bed.gz", d / "scales.txt"
    plain.write_text(matrix_text(cells))
    with gzip.open(gz, "wt") as f:
        f.write(matrix_text(cells))
    scales.write_text("".join("%r\n" % v for v in S.CLI_SCALES))
    return d, cells, str(plain), str(gz), str(scales)


@pytest.mark.gpu
def test_plain_gz_and_blocks(files):
    d, cells, plain, gz, _ = files
    res = S.cli_reference(False)
    want, out = S.cli_text(res), str(d / "cnvs.tsv")
    base = run([plain])
    assert base.returncode == 0 and base.stdout == stdout_text(res), base.stderr
    for args, env in (([plain], None), ([gz], None), ([plain], {"GOLEFT_EMDEPTH_ROWS": "7", "GOLEFT_EMDEPTH_TIMING": "1"})):
        if os.path.exists(out):
            os.remove(out)
        p = run(["--cnvs", out] + args, env)
        assert p.returncode == 0, p.stderr
        assert p.stdout == base.stdout                                   # stdout is what it is without --cnvs
        with open(out) as f:
            assert f.read() == want
        if env:
            assert '"cnv_kernels_s"' in p.stderr and '"block_rows": 7' in p.stderr


@pytest.mark.gpu
def test_scales_and_python_entry(files):
    d, cells, plain, gz, scales = files
    res = S.cli_reference(True)
    want, out = S.cli_text(res), str(d / "cnvs_scaled.tsv")
    assert want != S.cli_text(S.cli_reference(False))
    p = run(["--scales", scales, "--cnvs=" + out, gz], {"GOLEFT_EMDEPTH_ROWS": "7"})
    assert p.returncode == 0 and p.stdout == stdout_text(res), p.stderr
    with open(out) as f:
        assert f.read() == want
    from goleft_amd import emdepth
    out2, bed = str(d / "cnvs_py.tsv"), str(d / "out.bed")
    assert emdepth.Main(["--scales=" + scales, "--cnvs", out2, plain], out_path=bed) == 0
    with open(out2) as f:
        assert f.read() == want
    with open(bed) as f:
        assert f.read() == stdout_text(res)


@pytest.mark.gpu
def test_positions_that_do_not_fit_are_refused(files):
    d, cells, plain, gz, scales = files
    out = str(d / "never.tsv")
    for col, value in ((1, "4294967296"), (2, "4294967296"), (1, "-5"), (2, "1e3"), (1, "")):
        where = S.cli_where()
        w = list(where[2])
        w[col] = value
        bad = d / "bad_pos.bed"
        lines = matrix_text(cells).split("\n")
        f = lines[3].split("\t")                                          # row 2 is line 4
        f[col] = value
        lines[3] = "\t".join(f)
        bad.write_text("\n".join(lines))
        p = run(["--cnvs", out, str(bad)])
        assert p.returncode == 1 and p.stdout == "" and "line 4" in p.stderr and "2^32" in p.stderr, (value, p.stderr)
        assert not os.path.exists(out)
        assert run([str(bad)]).returncode == 0                           # without --cnvs the positions are only text
    p = run(["--cnvs", out, "--nope", plain])
    assert p.returncode == 255
    assert run(["--cnvs=", plain]).returncode == 255                     # an empty value is not "no --cnvs"
    assert run(["--cnvs", plain]).returncode == 255                      # ... nor is a value that eats the matrix
    # the largest position that fits
    lines = matrix_text(cells).split("\n")
    f = lines[40].split("\t")
    f[2] = "4294967295"
    lines[40] = "\t".join(f)
    top = d / "top.bed"
    top.write_text("\n".join(lines))
    p = run(["--cnvs", out, str(top)])
    assert p.returncode == 0 and os.path.exists(out), p.stderr
