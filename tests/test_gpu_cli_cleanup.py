"""GPU: the refusals of `goleft-depth` AFTER the device context exists -- the paths on which the context's owner
(host/cli.hpp, Device) destroys it on the way out.  Each is an ordinary refusal of a 3-sample, 4-row matrix with exit code 1:
the child ends by itself within its timeout (a negative code would be a signal), writes nothing to stdout and says exactly
the line the source prints.  Every child runs under its own timeout; nothing is retried."""
import os
import subprocess

import pytest

from tests.helpers import ROOT

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "goleft_amd", "goleft-depth")
HEADER = "#chrom\tstart\tend\ta\tb\tc\n"
ROWS = [("chr1", i * 1000, (i + 1) * 1000, 10 + i, 20 + i, 30 + i) for i in range(4)]


def matrix(zero_column=None, samples=3):
    head = "\t".join(HEADER.rstrip("\n").split("\t")[:3 + samples]) + "\n"
    body = ""
    for row in ROWS:
        cells = [0 if s == zero_column else row[3 + s] for s in range(samples)]
        body += "%s\t%d\t%d\t%s\n" % (row[0], row[1], row[2], "\t".join(str(c) for c in cells))
    return head + body


def make_work(d):
    """the inputs of every case, in the directory the children run in"""
    (d / "m").write_text(matrix())
    (d / "zero").write_text(matrix(zero_column=1))
    (d / "one").write_text(matrix(samples=1))
    (d / "short").write_text("0.4\n0.41\n0.42\n")
    (d / "long").write_text("0.4\n0.41\n0.42\n0.43\n0.44\n")
    (d / "ref.fa").write_text(">chr9\n" + "ACGT" * 15 + "\n")
    (d / "ref.fa.fai").write_text("chr9\t60\t6\t60\t61\n")
    return d


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    return make_work(tmp_path_factory.mktemp("cleanup"))


def refused(work, cmd, args, line):
    p = subprocess.run([EXE, cmd] + args, cwd=str(work), stdin=subprocess.DEVNULL, capture_output=True, text=True, timeout=120)
    assert p.returncode == 1, (p.returncode, p.stderr)
    assert p.stdout == ""
    assert line in p.stderr.split("\n"), p.stderr
    assert "no usable MI355X device" not in p.stderr


def test_scales_of_a_sample_without_depth(work):
    refused(work, "scales", ["zero"], "scales: sample b (column 5) has no depth above 0: it has no factor")


def test_debias_gc_values_one_line_short(work):
    refused(work, "debias", ["--gc-values", "short", "m"], "debias: short ends after line 3: the matrix has 4 rows")


def test_debias_gc_values_one_line_long(work):
    refused(work, "debias", ["--gc-values", "long", "m"], "debias: long: line 5: the matrix has only 4 rows")


def test_debias_fasta_without_the_chromosome(work):
    refused(work, "debias", ["--fasta", "ref.fa", "m"], "debias: chromosome chr1 is not in ref.fa.fai")


def test_debias_svd_of_one_sample(work):
    refused(work, "debias", ["--svd", "5", "one"],
            "debias: gd_svd_debias_scaled: tid or coordinate out of range (svd debias: 2 .. 1024 samples, not 1)")


def test_emdepth_normalize_cnvs_of_a_sample_without_depth(work):
    refused(work, "emdepth", ["--normalize", "--cnvs", "out", "zero"], "emdepth: sample b (column 5) has no depth above 0: it has no factor")
    assert not os.path.exists(str(work / "out"))
