"""-m gpu: `goleft-depth perbase` on the reference's fixture BAMs: stdout equals the lines of the
numpy restatement (tests/perbase_runs_ref.py) for the CPU oracle's per-base vector of the same records -- through the
device decoder and the host decoder, with -Q, -c, -b, --quantize and -o, whatever GOLEFT_PERBASE_SLICE is --, the default
output expanded position by position is what the `samtools depth -a` shim prints, and goleft_amd.perbase.Main gives the
command's bytes.  Every child process that uses the device runs under `timeout -k 10`."""
import functools
import os
import subprocess

import numpy as np
import pytest

from oracle import bamio, pyoracle as po
from tests import helpers as H
from tests import perbase_runs_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "goleft_amd", "goleft-depth")
SHIM = os.path.join(ROOT, "goleft_amd", "shim", "samtools")
REF = os.path.join(ROOT, "tests", "golden", "ref")
BED = os.path.join(REF, "windows.bed")


def perbase(*args, **env):
    p = subprocess.run(["timeout", "-k", "10", "60", EXE, "perbase"] + list(args), env=dict(os.environ, **env),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, (args, env, p.returncode, p.stderr.decode())
    return p.stdout.decode()


@functools.lru_cache(maxsize=None)
def fixture(name):
    """(contigs, reads) of a fixture BAM, read by the oracle's own reader."""
    if name == "t-empty":
        _, contigs, reads, _ = bamio.read_bam(os.path.join(REF, name + ".bam"))
        return contigs, reads
    contigs, reads, _ = H.load_golden_bam(name)
    return contigs, reads


@functools.lru_cache(maxsize=None)
def depth(name, tid, q):
    contigs, reads = fixture(name)
    L = contigs[tid][1]
    return po.perbase_c(reads[tid], q, 0, L) if tid in reads else np.zeros(L, np.int32)


def want(name, q=1, cuts=None, only=None):
    contigs, _ = fixture(name)
    return "".join(R.lines(c, depth(name, tid, q), 0, L, cuts) for tid, (c, L) in enumerate(contigs) if only in (None, c))


@pytest.mark.parametrize("name", ["t", "hla", "t-empty"])
def test_whole_files_through_both_decoders(name):
    bam = os.path.join(REF, name + ".bam")
    expect = want(name)
    assert expect.count("\n") >= len(fixture(name)[0])
    assert perbase(bam) == expect
    assert perbase(bam, GOLEFT_GPU_DECODE="0") == expect
    if name == "t-empty":                                                  # a contig without records is one run of 0
        assert expect == "".join("%s\t0\t%d\t0\n" % c for c in fixture(name)[0])


def test_flags():
    bam = os.path.join(REF, "t.bam")
    assert perbase("-Q", "0", bam) == want("t", q=0)
    assert perbase("-Q", "60", bam) == want("t", q=60)
    assert want("t", q=0) != want("t") != want("t", q=60)
    assert perbase("-c", "chr22", bam) == want("t", only="chr22")
    assert perbase("--chrom", "chrM", "--q", "0", bam) == want("t", q=0, only="chrM")


def test_quantize():
    bam = os.path.join(REF, "t.bam")
    assert perbase("--quantize", "1,4,100", bam) == want("t", cuts=[1, 4, 100])
    assert perbase("--quantize=1,4,100", "-c", "chrM", bam, GOLEFT_GPU_DECODE="0") == want("t", cuts=[1, 4, 100], only="chrM")
    hla = os.path.join(REF, "hla.bam")
    assert perbase("--quantize", "1,4,100", "-Q", "0", hla) == want("hla", q=0, cuts=[1, 4, 100])


def bed_lines(name, path, cuts=None):
    """The BED file's lines in file order, each clipped to its contig and emitted on its own."""
    contigs, _ = fixture(name)
    tid_of = {c: k for k, (c, _) in enumerate(contigs)}
    out = []
    for line in open(path, "rb"):
        if not line.strip() or line.startswith(b"#"):
            continue
        chrom, s, e = po.chrom_start_end_c(line if line.endswith(b"\n") else line + b"\n")
        tid = tid_of[chrom]
        L = contigs[tid][1]
        e = min(e, L)
        s = min(s, e)
        out.append(R.lines(chrom, depth(name, tid, 1), s, e, cuts))
    return "".join(out)


def test_bed_regions_clipped_and_in_file_order(tmp_path):
    bam = os.path.join(REF, "t.bam")
    expect = bed_lines("t", BED)
    assert expect
    assert perbase("-b", BED, bam) == expect
    assert perbase("-b", BED, "--quantize", "1,4,100", bam) == bed_lines("t", BED, [1, 4, 100])
    mine = tmp_path / "mine.bed"                                           # overlapping, out of order, beyond the end, empty
    mine.write_text("chr22\t100\t900\nchrM\t16000\t99999\nchr22\t500\t600\n\nchrM:5-5\nchrM\t0\t16571\nchr22\t30000\t30010")
    assert perbase("-b", str(mine), bam) == bed_lines("t", str(mine))
    assert perbase("-b", str(mine), "-c", "chrM", bam) == "".join(
        R.lines("chrM", depth("t", 0, 1), s, e) for s, e in ((16000, 16571), (4, 5), (0, 16571)))


@pytest.mark.parametrize("sl", ["7", "1000"])
def test_the_output_does_not_depend_on_the_slice(sl):
    bam = os.path.join(REF, "t.bam")
    for args, expect in (([], want("t")), (["--quantize", "1,4,100"], want("t", cuts=[1, 4, 100])), (["-b", BED], bed_lines("t", BED))):
        assert perbase(*args, bam, GOLEFT_PERBASE_SLICE=sl) == expect, (args, sl)


def test_a_slice_of_one_position(tmp_path):
    """Every run but the one-position ones is joined from its pieces on the host."""
    bam = os.path.join(REF, "t.bam")
    small = tmp_path / "small.bed"
    small.write_text("chrM\t3000\t4200\nchr22\t14990\t15400\n")
    assert perbase("-b", str(small), bam, GOLEFT_PERBASE_SLICE="1") == bed_lines("t", str(small)) != ""
    assert perbase("-b", str(small), "--quantize", "2,4,100", bam, GOLEFT_PERBASE_SLICE="1") == bed_lines("t", str(small), [2, 4, 100])
    assert perbase(os.path.join(REF, "t-empty.bam"), GOLEFT_PERBASE_SLICE="1000") == want("t-empty")


def test_output_file_and_python_entry_point(tmp_path):
    from goleft_amd import perbase as gp
    bam = os.path.join(REF, "t.bam")
    expect = want("t", only="chrM")
    out = tmp_path / "o.bed"
    assert perbase("-c", "chrM", "-o", str(out), bam) == ""
    assert out.read_text() == expect
    out2 = tmp_path / "p.bed"
    assert gp.Main(["-c", "chrM", bam], out_path=str(out2)) == 0
    assert out2.read_bytes() == out.read_bytes()
    out3 = tmp_path / "q.bed"
    assert gp.Main(["--quantize", "1,4,100", "-o", str(out3), bam]) == 0
    assert out3.read_text() == want("t", cuts=[1, 4, 100])
    assert gp.Main(["-c", "chrZ", bam], out_path=str(tmp_path / "r.bed")) == 1


def test_expanded_output_is_what_the_samtools_shim_prints():
    bam = os.path.join(REF, "t.bam")
    for chrom, L in fixture("t")[0]:
        shim = subprocess.run(["timeout", "-k", "10", "60", SHIM, "depth", "-a", "-Q", "1", "-r", chrom, bam], stdout=subprocess.PIPE,
                              stderr=subprocess.PIPE)
        assert shim.returncode == 0, shim.stderr.decode()
        expanded = []
        for line in perbase("-c", chrom, bam).splitlines():
            c, s, e, d = line.split("\t")
            expanded += ["%s\t%d\t%s\n" % (c, p + 1, d) for p in range(int(s), int(e))]
        assert len(expanded) == L
        assert "".join(expanded) == shim.stdout.decode()
