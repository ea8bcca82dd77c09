"""CPU: what `goleft-depth perbase` refuses before it opens a device: exit code 1 and a first
stderr line that names the cause, nothing on stdout.  GOLEFT_DEVICE names a device no box has: a command that went on to
open one would say so instead."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "goleft_amd", "goleft-depth")
BAM = os.path.join(ROOT, "tests", "golden", "ref", "t.bam")
CUTS33 = ",".join(str(k) for k in range(1, 34))


def _perbase(*args):
    p = subprocess.run([EXE, "perbase"] + list(args), env=dict(os.environ, GOLEFT_DEVICE="99"), stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE)
    err = p.stderr.decode().splitlines()
    return p.returncode, p.stdout, err[0] if err else ""


@pytest.mark.parametrize("args, line", [
    (["-c", "chrZ", BAM], "perbase: chromosome chrZ is not in the BAM header"),
    (["--quantize", "1,,4", BAM], "error: --quantize 1,,4: an empty field"),
    (["--quantize", ",1", BAM], "error: --quantize ,1: an empty field"),
    (["--quantize", "", BAM], "error: --quantize : an empty field"),
    (["--quantize", "1,x", BAM], "error: --quantize 1,x: 'x' is not an integer"),
    (["--quantize", "1.5", BAM], "error: --quantize 1.5: '1.5' is not an integer"),
    (["--quantize", "4,4", BAM], "error: --quantize 4,4: cut 4 is not above the cut before it"),
    (["--quantize", "4,3", BAM], "error: --quantize 4,3: cut 3 is not above the cut before it"),
    (["--quantize", "0,4", BAM], "error: --quantize 0,4: cut 0 is below 1"),
    (["--quantize", "-2", BAM], "error: --quantize -2: cut -2 is below 1"),
    (["--quantize", CUTS33, BAM], "error: --quantize %s: more than 32 cuts" % CUTS33),
    (["--frobnicate", BAM], "error: unknown argument --frobnicate"),
    (["-z", BAM], "error: unknown argument -z"),
    (["-Q", "high", BAM], "error: -Q high: not an integer"),
    ([], "error: bam is required"),
])
def test_refused_from_the_command_line_alone(args, line):
    rc, out, err = _perbase(*args)
    assert (rc, out, err) == (1, b"", line)


def test_a_missing_and_a_cram_input(tmp_path):
    missing = str(tmp_path / "none.bam")
    assert _perbase(missing) == (1, b"", "perbase: cannot open %s: No such file or directory" % missing)
    cram = tmp_path / "x.cram"
    cram.write_bytes(b"CRAM")
    assert _perbase(str(cram)) == (1, b"", "perbase: %s: a CRAM is not served, only a BAM" % cram)


def test_bed_lines_the_header_lacks_or_that_hold_no_region(tmp_path):
    unknown = tmp_path / "unknown.bed"
    unknown.write_text("chrM\t1\t5\n\n# a comment\nchrZ\t1\t5\n")
    assert _perbase("-b", str(unknown), BAM) == (1, b"", "perbase: %s:4: chromosome chrZ is not in the BAM header" % unknown)
    bad = tmp_path / "bad.bed"
    bad.write_text("chrM\t1\t5\nnonsense here\nchrM\t2\t3\n")
    assert _perbase("-b", str(bad), BAM) == (1, b"", "perbase: %s:2: cannot get a region from this line" % bad)
    assert _perbase("-b", str(tmp_path / "nofile.bed"), BAM) == (1, b"", "perbase: cannot open %s" % (tmp_path / "nofile.bed"))


def test_a_valid_command_line_goes_on_to_the_device():
    """The counterpart: nothing above is refused for another reason than the one pinned."""
    rc, out, err = _perbase("-Q", "0", "-c", "chrM", "--quantize", "1,4,100", BAM)
    assert (rc, out, err) == (1, b"", "perbase: no usable MI355X device (tid or coordinate out of range); this build has no CPU path") or \
        (rc, out, err) == (1, b"", "perbase: no usable MI355X device (no usable HIP device); this build has no CPU path")
