"""GPU: `goleft-depth cnveval` -- the worked example byte for byte, plain and gzipped; -s against the restatement on the
filtered truths, with the two counts on stderr; the dropped last line; every refusal of the parser with file and line;
goleft_amd.cnveval.Main and evaluate against the binary.  Every call runs under its own timeout; nothing is retried."""
import gzip
import os
import subprocess

import numpy as np
import pytest

from tests import cnveval_ref as R
from tests import cnveval_shapes as S
from tests.helpers import ROOT

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "goleft_amd", "goleft-depth")


def run(args, env=None):
    return subprocess.run([EXE, "cnveval"] + args, capture_output=True, text=True, timeout=120, env=dict(os.environ, **(env or {})))


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("cnveval")
    (d / "truth.bed").write_text(S.WORKED_TRUTH)
    (d / "test.bed").write_text("#chrom\tstart\tend\tcn\tsample\n" + S.WORKED_TEST)
    for n in ("truth", "test"):
        with gzip.open(d / (n + ".bed.gz"), "wt") as f:
            f.write((d / (n + ".bed")).read_text())
    return d


def test_worked_example_plain_and_gz(files):
    p = run(["-m", "0.4", str(files / "truth.bed"), str(files / "test.bed")])
    assert p.returncode == 0, p.stderr
    assert p.stdout == S.WORKED_OUT
    assert p.stderr == "cnveval: cnvs in test-set (6)\ncnveval: 5 total cnvs in truth-set (4)\n"
    p = run([str(files / "truth.bed.gz"), str(files / "test.bed.gz")], {"GOLEFT_CNVEVAL_TIMING": "1"})
    assert p.returncode == 0 and p.stdout == S.WORKED_OUT, p.stderr
    assert "kernels" in p.stderr.splitlines()[2] and "read-back" in p.stderr.splitlines()[2]


def test_limit_samples(files):
    truths = S.parse_bed(S.WORKED_TRUTH, False) + [("1", 1000, 6000, 1, ["zz", "c"]), ("1", 50000, 90000, 3, ["c", "b"])]
    cnvs = S.parse_bed(S.WORKED_TEST, True)
    path = files / "truth_more.bed"
    path.write_text(S.bed_text(truths))
    have = {c[4] for c in cnvs}
    kept = [t for t in truths if have & set(t[4])]
    assert len(kept) == len(truths) - 2                          # `2 100 200 1 c` and the zz,c line name no test sample
    want = R.report(R.evaluate_literal(cnvs, kept, 0.4))
    assert want != R.report(R.evaluate_literal(cnvs, truths, 0.4))
    p = run(["-s", str(path), str(files / "test.bed")])
    assert p.returncode == 0 and p.stdout == want, p.stderr
    assert p.stderr == "cnveval: cnvs in test-set (6)\ncnveval: %d total cnvs in truth-set (%d)\n" % (sum(len(t[4]) for t in kept), len(kept))
    p = run(["--limitsamples", "--minoverlap=0.4", str(path), str(files / "test.bed")])
    assert p.returncode == 0 and p.stdout == want, p.stderr


def test_last_line_without_newline_is_dropped(files):
    path = files / "test_cut.bed"
    path.write_text(S.WORKED_TEST[:-1])
    cnvs = S.parse_bed(S.WORKED_TEST, True)[:-1]
    want = R.report(R.evaluate_literal(cnvs, S.parse_bed(S.WORKED_TRUTH, False), 0.4))
    assert want != S.WORKED_OUT
    p = run([str(files / "truth.bed"), str(path)])
    assert p.returncode == 0 and p.stdout == want, p.stderr
    err = p.stderr.splitlines()
    assert len(err) == 3 and "%s:6" % path in err[0] and "no newline" in err[0]
    assert err[1] == "cnveval: cnvs in test-set (5)"


@pytest.mark.parametrize("text, line, word", [
    ("1\t10\t20\t1\n", 1, "five fields"),
    ("1\t10\t20\t1\ta\n\n1\t10\t20\t1\ta\n", 2, "empty line"),
    ("#c\n1\t10\t2x\t1\ta\n", 2, "not an integer"),
    ("1\t10\t20\t1.0\ta\n", 1, "not an integer"),
    ("1\t10\t2147483648\t1\ta\n", 1, "2147483647"),
    ("1\t10\t99999999999999999999999\t1\ta\n", 1, "2147483647"),
    ("1\t-1\t20\t1\ta\n", 1, "outside 0"),
    ("1\t10\t20\t1\ta\n1\t30\t29\t1\ta\n", 2, "before the start"),
])
def test_parser_refusals(files, text, line, word):
    bad = files / "bad.bed"
    bad.write_text(text)
    for args in ([str(bad), str(files / "test.bed")], [str(files / "truth.bed"), str(bad)]):
        p = run(args)
        assert p.returncode == 1 and p.stdout == "", (p.returncode, p.stdout, p.stderr)
        assert "%s:%d:" % (bad, line) in p.stderr and word in p.stderr, p.stderr


def test_usage_errors_and_a_missing_file(files):
    truth, test = str(files / "truth.bed"), str(files / "test.bed")
    for args in (["-m", "0", truth, test], ["-m", "1.5", truth, test], ["-m", "x", truth, test], [truth], ["--nope", truth, test]):
        p = run(args)
        assert p.returncode == 255 and p.stdout == "" and "usage: cnveval" in p.stderr, (args, p.stderr)
    p = run([truth, str(files / "absent.bed")])
    assert p.returncode == 1 and "cannot open" in p.stderr


def test_python_entries_agree_with_the_binary(files):
    from goleft_amd import cnveval
    out = files / "report.txt"
    assert cnveval.Main(["-m", "0.4", str(files / "truth.bed.gz"), str(files / "test.bed")], out_path=str(out)) == 0
    assert out.read_text() == S.WORKED_OUT
    case = S.cases()["hand_worked"]
    names, stats = cnveval.evaluate(case.cnvs, case.truths, 0.4)
    want_names, want = S.reference("hand_worked")
    assert names == want_names and stats.dtype == np.int64 and (stats == want).all()
    tabs = stats.sum(axis=0)
    assert R.report({("all", k): tabs[k].tolist() for k in range(3)}) == S.WORKED_OUT
    names, stats = cnveval.evaluate([], [], 0.4)
    assert names == [] and stats.shape == (0, 3, 4)
