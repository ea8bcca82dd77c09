"""-m gpu: `goleft-depth dist` on the reference's fixture BAMs: the bytes of every file it writes
equal the text of the numpy restatement (tests/depth_hist_ref.py) for the CPU oracle's per-base vectors of the same
records -- through the device decoder and the host decoder, with -Q, -c, --max-depth, -b and --thresholds --, and
goleft_amd.dist.Main writes the command's bytes.  Every child process that uses the device runs under `timeout -k 10`."""
import functools
import os
import subprocess

import numpy as np
import pytest

from oracle import bamio, pyoracle as po
from tests import depth_hist_ref as D
from tests import helpers as H

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "goleft_amd", "goleft-depth")
REF = os.path.join(ROOT, "tests", "golden", "ref")
BED = os.path.join(REF, "windows.bed")
SUFFIXES = (".dist.txt", ".summary.txt", ".region.dist.txt", ".thresholds.bed")
MINE = ("chr22\t100\t900\texon1\nchrM\t16000\t99999\nchr22\t500\t600\texon1\textra\n\n# a comment\nchrM:5-5\nchrM\t0\t16571\tall of it\n"
        "chr22\t30000\t30010\t\nchrM\t3000\t3400\tplateau\t0\t+")               # overlapping, out of order, past the end, empty


def dist(tmp_path, *args, **env):
    """{suffix: text} of the files the command wrote under a fresh prefix."""
    prefix = str(tmp_path / ("run%d" % len(os.listdir(str(tmp_path)))) / "s")
    os.makedirs(os.path.dirname(prefix))
    p = subprocess.run(["timeout", "-k", "10", "60", EXE, "dist", "--prefix", prefix] + list(args), env=dict(os.environ, **env),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0 and p.stdout == b"", (args, env, p.returncode, p.stderr.decode())
    made = sorted(os.listdir(os.path.dirname(prefix)))
    assert all(f.startswith("s.") and f[1:] in SUFFIXES for f in made), made
    return {f[1:]: open(os.path.join(os.path.dirname(prefix), f)).read() for f in made}


@functools.lru_cache(maxsize=None)
def fixture(name):
    """(contigs, reads) of a fixture BAM, read by the oracle's own reader."""
    if name == "t-empty":
        _, contigs, reads, _ = bamio.read_bam(os.path.join(REF, name + ".bam"))
        return contigs, reads
    contigs, reads, _ = H.load_golden_bam(name)
    return contigs, reads


@functools.lru_cache(maxsize=None)
def depths(name, q):
    contigs, reads = fixture(name)
    return [po.perbase_c(reads[tid], q, 0, L) if tid in reads else np.zeros(L, np.int32) for tid, (_, L) in enumerate(contigs)]


def bed_lines(name, path):
    """The BED file's lines in file order as (tid, start, end, name), each clipped to its contig."""
    contigs, _ = fixture(name)
    tid_of = {c: k for k, (c, _) in enumerate(contigs)}
    out = []
    for line in open(path, "rb"):
        if not line.strip() or line.startswith(b"#"):
            continue
        chrom, s, e = po.chrom_start_end_c(line if line.endswith(b"\n") else line + b"\n")
        L = contigs[tid_of[chrom]][1]
        e = min(e, L)
        s = min(s, e)
        fields = line.decode().rstrip("\r\n").split("\t")
        out.append((tid_of[chrom], s, e, fields[3] if len(fields) > 3 and fields[3] else "unknown"))
    return out


def want(name, q=1, **kw):
    return D.files(fixture(name)[0], depths(name, q), **kw)


@pytest.mark.parametrize("name", ["t", "hla", "t-empty"])
def test_whole_files_through_both_decoders(tmp_path, name):
    bam = os.path.join(REF, name + ".bam")
    expect = want(name)
    assert set(expect) == {".dist.txt", ".summary.txt"}
    assert expect[".summary.txt"].count("\n") == len(fixture(name)[0]) + 2
    assert dist(tmp_path, bam) == expect
    assert dist(tmp_path, bam, GOLEFT_GPU_DECODE="0") == expect
    if name == "t-empty":
        contigs = [c for c in fixture(name)[0]]
        assert expect[".dist.txt"] == "".join("%s\t0\t1.000000\n" % c for c, L in contigs if L) + "total\t0\t1.000000\n"
        assert expect[".summary.txt"] == "chrom\tlength\tbases\tmean\tmin\tmax\n" + "".join("%s\t%d\t0\t0.00\t0\t0\n" % c for c in contigs) + \
            "total\t%d\t0\t0.00\t0\t0\n" % sum(L for _, L in contigs)


def test_flags(tmp_path):
    bam = os.path.join(REF, "t.bam")
    assert dist(tmp_path, "-Q", "0", bam) == want("t", q=0)
    assert dist(tmp_path, "-Q", "60", bam) == want("t", q=60)
    assert want("t", q=0) != want("t") != want("t", q=60)
    assert dist(tmp_path, "-c", "chr22", bam) == want("t", only="chr22")
    assert dist(tmp_path, "--chrom", "chrM", "--q", "0", bam, GOLEFT_GPU_DECODE="0") == want("t", q=0, only="chrM")


def test_max_depth_clamps_the_distribution_and_not_the_summary(tmp_path):
    bam = os.path.join(REF, "t.bam")
    assert int(depths("t", 1)[0].max()) == 2012                            # chrM: the default does not clamp, 100 does
    clamped, full = want("t", max_depth=100), want("t")
    assert dist(tmp_path, "--max-depth", "100", bam) == clamped
    assert dist(tmp_path, "--max-depth=100", "-Q", "0", bam, GOLEFT_GPU_DECODE="0") == want("t", q=0, max_depth=100)
    assert clamped[".dist.txt"].startswith("chrM\t100\t") and full[".dist.txt"].startswith("chrM\t2012\t")
    assert clamped[".summary.txt"] == full[".summary.txt"]
    assert dist(tmp_path, "--max-depth", "1", bam) == want("t", max_depth=1)
    assert dist(tmp_path, "--max-depth", "2012", bam)[".dist.txt"] == full[".dist.txt"]
    assert dist(tmp_path, "--max-depth", "2011", bam) == want("t", max_depth=2011)


@pytest.mark.parametrize("decode", ["1", "0"])
def test_bed_lines_and_thresholds(tmp_path, decode):
    bam = os.path.join(REF, "t.bam")
    mine = tmp_path / "mine.bed"
    mine.write_text(MINE)
    for path in (BED, str(mine)):
        lines = bed_lines("t", path)
        assert dist(tmp_path, "-b", path, bam, GOLEFT_GPU_DECODE=decode) == want("t", bed=lines)
        expect = want("t", bed=lines, thresholds=[1, 10, 2000, 3000])
        assert set(expect) == set(SUFFIXES)
        assert dist(tmp_path, "-b", path, "--thresholds", "1,10,2000,3000", bam, GOLEFT_GPU_DECODE=decode) == expect
    lines = bed_lines("t", str(mine))
    assert [b[3] for b in lines] == ["exon1", "unknown", "exon1", "unknown", "all of it", "unknown", "plateau"]
    assert [b[1:3] for b in lines][:4] == [(100, 900), (16000, 16571), (500, 600), (4, 5)]
    assert dist(tmp_path, "-b", str(mine), "-c", "chrM", "--thresholds", "1,10,2000,3000", "--max-depth", "100", bam, GOLEFT_GPU_DECODE=decode) == \
        want("t", bed=lines, thresholds=[1, 10, 2000, 3000], only="chrM", max_depth=100)
    assert dist(tmp_path, "-b", str(mine), "-c", "chr22", "--thresholds", "5", bam, GOLEFT_GPU_DECODE=decode) == \
        want("t", bed=lines, thresholds=[5], only="chr22")


def test_bed_lines_on_the_other_fixtures(tmp_path):
    bed = tmp_path / "hla.bed"                                             # (the HLA contig's name holds colons: no BED line can name it)
    bed.write_text("chr22\t6667\t20001\tr0\nchr22\t0\t10\n")
    lines = bed_lines("hla", str(bed))
    assert dist(tmp_path, "-b", str(bed), "--thresholds", "1,10,2000,3000", os.path.join(REF, "hla.bam")) == \
        want("hla", bed=lines, thresholds=[1, 10, 2000, 3000])
    contigs, _ = fixture("t-empty")
    bed.write_text("%s\t0\t100\n" % contigs[0][0])
    got = dist(tmp_path, "-b", str(bed), "--thresholds", "1", os.path.join(REF, "t-empty.bam"))
    assert got == want("t-empty", bed=bed_lines("t-empty", str(bed)), thresholds=[1])
    assert got[".thresholds.bed"].splitlines()[1].split("\t")[3:] == ["unknown", "0"]


def test_the_python_entry_point_writes_the_same_bytes(tmp_path):
    from goleft_amd import dist as gd
    bam = os.path.join(REF, "t.bam")
    prefix = str(tmp_path / "py")
    assert gd.Main(["-b", BED, "--thresholds", "1,10,2000,3000", "--prefix", prefix, bam]) == 0
    expect = want("t", bed=bed_lines("t", BED), thresholds=[1, 10, 2000, 3000])
    assert {s: open(prefix + s).read() for s in SUFFIXES} == expect
    assert gd.Main(["-c", "chrZ", "--prefix", str(tmp_path / "no"), bam]) == 1
    assert not [f for f in os.listdir(str(tmp_path)) if f.startswith("no")]


def test_the_timing_line(tmp_path):
    p = subprocess.run(["timeout", "-k", "10", "60", EXE, "dist", "--prefix", str(tmp_path / "t"), os.path.join(REF, "t.bam")],
                       env=dict(os.environ, GOLEFT_DIST_TIMING="1"), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0 and p.stdout == b""
    assert [ln for ln in p.stderr.decode().splitlines() if ln.startswith("dist: ") and "kernels" in ln and "device calls" in ln]
