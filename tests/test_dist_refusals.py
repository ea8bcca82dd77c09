"""CPU: what `goleft-depth dist` refuses before it opens a device: exit code 1, a first stderr line
that names the cause, nothing on stdout and no file created.  GOLEFT_DEVICE names a device no box has: a command that went
on to open one would say so instead."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "goleft_amd", "goleft-depth")
BAM = os.path.join(ROOT, "tests", "golden", "ref", "t.bam")
BED = os.path.join(ROOT, "tests", "golden", "ref", "windows.bed")
T33 = ",".join(str(k) for k in range(1, 34))
PREFIX = "@PREFIX@"                                 # stands for tmp_path / "out" in the argument lists


def _dist(tmp_path, *args):
    args = [str(tmp_path / "out") if a == PREFIX else a for a in args]
    p = subprocess.run([EXE, "dist"] + args, env=dict(os.environ, GOLEFT_DEVICE="99"), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       cwd=str(tmp_path))
    err = p.stderr.decode().splitlines()
    made = sorted(f for f in os.listdir(str(tmp_path)) if f.startswith("out"))
    return p.returncode, p.stdout, err[0] if err else "", made


@pytest.mark.parametrize("args, line", [
    (["--prefix", PREFIX, "-c", "chrZ", BAM], "dist: chromosome chrZ is not in the BAM header"),
    ([BAM], "error: --prefix is required"),
    (["--prefix", "", BAM], "error: --prefix is required"),
    (["--prefix", PREFIX, "--max-depth", "0", BAM], "error: --max-depth 0: 1 .. 65535"),
    (["--prefix", PREFIX, "--max-depth", "65536", BAM], "error: --max-depth 65536: 1 .. 65535"),
    (["--prefix", PREFIX, "--max-depth", "-3", BAM], "error: --max-depth -3: 1 .. 65535"),
    (["--prefix", PREFIX, "--max-depth", "many", BAM], "error: --max-depth many: not an integer"),
    (["--prefix", PREFIX, "--max-depth", "1e3", BAM], "error: --max-depth 1e3: not an integer"),
    (["--prefix", PREFIX, "--thresholds", "1,10", BAM], "error: --thresholds needs -b"),
    (["--prefix", PREFIX, "-b", BED, "--thresholds", "1,,4", BAM], "error: --thresholds 1,,4: an empty field"),
    (["--prefix", PREFIX, "-b", BED, "--thresholds", "", BAM], "error: --thresholds : an empty field"),
    (["--prefix", PREFIX, "-b", BED, "--thresholds", "1,x", BAM], "error: --thresholds 1,x: 'x' is not an integer"),
    (["--prefix", PREFIX, "-b", BED, "--thresholds", "1.5", BAM], "error: --thresholds 1.5: '1.5' is not an integer"),
    (["--prefix", PREFIX, "-b", BED, "--thresholds", "4,4", BAM], "error: --thresholds 4,4: cut 4 is not above the cut before it"),
    (["--prefix", PREFIX, "-b", BED, "--thresholds", "4,3", BAM], "error: --thresholds 4,3: cut 3 is not above the cut before it"),
    (["--prefix", PREFIX, "-b", BED, "--thresholds", "0,4", BAM], "error: --thresholds 0,4: cut 0 is below 1"),
    (["--prefix", PREFIX, "-b", BED, "--thresholds", T33, BAM], "error: --thresholds %s: more than 32 cuts" % T33),
    (["--prefix", PREFIX, "--frobnicate", BAM], "error: unknown argument --frobnicate"),
    (["--prefix", PREFIX, "-o", "x", BAM], "error: unknown argument -o"),
    (["--prefix", PREFIX, "-Q", "high", BAM], "error: -Q high: not an integer"),
    (["--prefix", PREFIX, BAM, BAM], "error: too many positional arguments at '%s'" % BAM),
    (["--prefix", PREFIX], "error: bam is required"),
    (["--prefix"], "error: missing value for --prefix"),
])
def test_refused_from_the_command_line_alone(tmp_path, args, line):
    assert _dist(tmp_path, *args) == (1, b"", line, [])


def test_a_missing_and_a_cram_input(tmp_path):
    missing = str(tmp_path / "none.bam")
    assert _dist(tmp_path, "--prefix", PREFIX, missing) == (1, b"", "dist: cannot open %s: No such file or directory" % missing, [])
    cram = tmp_path / "x.cram"
    cram.write_bytes(b"CRAM")
    assert _dist(tmp_path, "--prefix", PREFIX, str(cram)) == (1, b"", "dist: %s: a CRAM is not served, only a BAM" % cram, [])


def test_a_prefix_whose_directory_is_missing(tmp_path):
    prefix = str(tmp_path / "no_such_dir" / "out")
    p = subprocess.run([EXE, "dist", "--prefix", prefix, BAM], env=dict(os.environ, GOLEFT_DEVICE="99"), stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE)
    assert (p.returncode, p.stdout) == (1, b"")
    assert p.stderr.decode().splitlines()[0] == "dist: cannot write to %s: No such file or directory" % (tmp_path / "no_such_dir")
    assert os.listdir(str(tmp_path)) == []


def test_bed_lines_the_header_lacks_or_that_hold_no_region(tmp_path):
    unknown = tmp_path / "unknown.bed"
    unknown.write_text("chrM\t1\t5\n\n# a comment\nchrZ\t1\t5\n")
    assert _dist(tmp_path, "--prefix", PREFIX, "-b", str(unknown), BAM) == \
        (1, b"", "dist: %s:4: chromosome chrZ is not in the BAM header" % unknown, [])
    bad = tmp_path / "bad.bed"
    bad.write_text("chrM\t1\t5\nnonsense here\nchrM\t2\t3\n")
    assert _dist(tmp_path, "--prefix", PREFIX, "-b", str(bad), "--thresholds", "1", BAM) == \
        (1, b"", "dist: %s:2: cannot get a region from this line" % bad, [])
    nofile = tmp_path / "nofile.bed"
    assert _dist(tmp_path, "--prefix", PREFIX, "-b", str(nofile), BAM) == (1, b"", "dist: cannot open %s" % nofile, [])


def test_a_valid_command_line_goes_on_to_the_device(tmp_path):
    """The counterpart: nothing above is refused for another reason than the one pinned."""
    rc, out, err, made = _dist(tmp_path, "--prefix", PREFIX, "-Q", "0", "-c", "chrM", "-b", BED, "--thresholds", "1,10,2000,3000",
                               "--max-depth", "100", BAM)
    assert (rc, out, made) == (1, b"", [])
    assert err in ("dist: no usable MI355X device (tid or coordinate out of range); this build has no CPU path",
                   "dist: no usable MI355X device (no usable HIP device); this build has no CPU path")
