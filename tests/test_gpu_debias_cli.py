"""GPU: `goleft-depth debias` and `goleft-depth emdepth --gc-values | --gc-fasta` on a 9-sample, 40-row integer matrix
whose depth is a per-sample level x a per-sample function of a per-row covariate x a few planted CNVs -- text for text
against the restatements (tests/debias_ref.py for the quotients, tests/scales_ref.py for the factors, tests/emdepth_ref.py
for the copy numbers).  The bias differs from sample to sample (a bias all samples share is taken up by EMDepth's own row
median): sample s sits at 1 + SLOPES[s] * t, t from -1 at the lowest covariate to +1 at the highest.

Before any device call the matrix is held, on the CPU, to what the comparison rests on: the restatement alone calls exactly
the planted CNVs after the debiasing and miscalls the stated rows at the covariate's extremes without it, no cell sits on an
adjustCN margin and every row's comparisons are wider than 1e-9 relative.  Every call runs under its own timeout; nothing
is retried."""
import functools
import os
import subprocess

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import debias_ref as DR
from tests import emdepth_ref as R
from tests import scales_ref as SR
from tests.helpers import ROOT

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "goleft_amd", "goleft-depth")
ROWS, N = 40, 9
NAMES = ["s%d" % i for i in range(N)]
HEADER = "#chrom\tstart\tend\t" + "\t".join(NAMES)
LEVELS = (1.0, 0.5, 2.0, 1.25, 0.8, 1.0, 1.5, 3.0, 0.9)
SLOPES = (-0.5, -0.3, -0.15, 0.0, 0.0, 0.1, 0.2, 0.35, 0.5)
GC_LEVELS = (0.30, 0.375, 0.45, 0.525, 0.60)     # five chunks of eight rows at the default window
WINDOW = 0.01
LEVEL = 60.0
# (row, sample, copy number); a lone copy number 1 is not planted: the reference's centres do not call it in a row of nine
PLANTED = ((7, 2, 3), (12, 5, 3), (20, 0, 3), (33, 8, 0), (4, 8, 0), (26, 3, 4), (39, 1, 3), (15, 7, 4))
MISCALLED_ROWS = 16      # rows of the two extreme chunks: the undebiased run calls a CNV no one planted in every one
DEFAULT_LEVEL = 73.0     # the middle sample median (dcnv's 0.65 quantile) of the matrix as read


def where(i):
    return "chr%d\t%d\t%d" % (1 + i // 25, (i % 25) * 1000, (i % 25 + 1) * 1000)


def vals():
    return np.array([GC_LEVELS[r % 5] + (r // 5) * 0.0005 for r in range(ROWS)])


def truth():
    cn = np.full((ROWS, N), 2, np.int64)
    for r, s, c in PLANTED:
        cn[r, s] = c
    return cn


def cli_cells():
    rng = np.random.default_rng(7)
    t = (np.array([GC_LEVELS[r % 5] for r in range(ROWS)]) - 0.45) / 0.15
    bias = 1.0 + np.outer(t, SLOPES)
    noise = 1.0 + rng.uniform(-0.03, 0.03, (ROWS, N))
    return np.floor(60.0 * np.array(LEVELS) * bias * noise * truth() / 2.0).astype(np.int64)


def matrix_text(cells, fmt=str, header=HEADER):
    rows = ["%s\t%s" % (where(i), "\t".join(fmt(v) for v in row)) for i, row in enumerate(np.asarray(cells).tolist())]
    return header + "\n" + "\n".join(rows) + "\n"


def held(ref):
    assert all(not R.pair_excluded(a, b) for r in ref for a, b in r.pairs.values())
    assert min(r.gap for r in ref) > 1e-9
    return np.array([r.cn for r in ref])


@functools.lru_cache(maxsize=None)
def expected(level=LEVEL):
    """(debiased text, copy-number text after the debiasing, copy-number text without it), all the restatements' and
    held to the conditions above -- on the CPU, before any device call"""
    m = cli_cells().astype(np.float32)
    med_read = SR.sample_medians(m)[0]
    assert SR.level_of(med_read) == DEFAULT_LEVEL
    T = SR.level_of(med_read) if level is None else level
    _, deb, cor, C_, _ = DR.debias(m, vals(), WINDOW)
    assert C_ == 5 and np.bincount(cor).tolist() == [8] * 5 and np.isfinite(deb).all()
    deb_text = DR.matrix_text(HEADER, [where(i) for i in range(ROWS)], deb)
    # what read_matrix makes of that text is the float32 itself
    back = np.array([[np.float32(float(v)) for v in line.split("\t")[3:]] for line in deb_text.split("\n")[1:-1]], np.float32)
    assert np.array_equal(back.view(np.uint32), deb.view(np.uint32))
    cn_deb = held(R.em_matrix((deb * SR.scales(SR.sample_medians(deb)[0], T)[None, :]).astype(np.float32)))
    cn_raw = held(R.em_matrix((m * SR.scales(med_read, T)[None, :]).astype(np.float32)))
    # the debiased run calls the planted CNVs and nothing else; the undebiased one follows the covariate
    assert np.array_equal(cn_deb, truth())
    wrong = np.flatnonzero((cn_raw != truth()).any(1))
    assert len(wrong) == MISCALLED_ROWS and all(r % 5 in (0, 4) for r in wrong)
    assert all(cn_raw[r, s] != c for r, s, c in PLANTED if r % 5 in (0, 4) and c)
    return deb_text, matrix_text(cn_deb), matrix_text(cn_raw)


def run(cmd, args, env=None):
    return subprocess.run([EXE, cmd] + args, capture_output=True, text=True, timeout=120, env=dict(os.environ, **(env or {})))


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    expected()
    d = tmp_path_factory.mktemp("debias")
    plain, gc = d / "m.bed", d / "gc.txt"
    plain.write_text(matrix_text(cli_cells()))
    gc.write_text("".join("%r\n" % float(v) for v in vals()))
    return d, str(plain), str(gc)


def test_debias_writes_the_restatements_text(files):
    d, plain, gc = files
    p = run("debias", ["--gc-values", gc, plain], {"GOLEFT_EMDEPTH_TIMING": "1"})
    assert p.returncode == 0, p.stderr
    assert p.stdout == expected()[0]
    assert '"debias_kernels_s"' in p.stderr and '"debias_chunks": 5' in p.stderr and '"debias_largest_chunk": 8' in p.stderr
    p = run("debias", ["--window=0.01", "--gc-values=" + gc, plain])
    assert p.returncode == 0 and p.stdout == expected()[0], p.stderr
    # another window: one chunk of all rows
    p = run("debias", ["--gc-values", gc, "--window", "1", plain])
    assert p.returncode == 0, p.stderr
    m = cli_cells().astype(np.float32)
    assert p.stdout == DR.matrix_text(HEADER, [where(i) for i in range(ROWS)], DR.debias(m, vals(), 1.0)[1])
    from goleft_amd import emdepth
    out = str(d / "deb.bed")
    assert emdepth.Debias(["--gc-values", gc, plain], out_path=out) == 0
    with open(out) as f:
        assert f.read() == expected()[0]


def test_emdepth_with_gc_values_is_debias_then_normalize(files):
    d, plain, gc = files
    deb_text, want, raw = expected()
    deb = d / "deb2.bed"
    p = run("debias", ["--gc-values", gc, plain])
    assert p.returncode == 0, p.stderr
    deb.write_text(p.stdout)
    two = run("emdepth", ["--normalize", "--level", "60", str(deb)])
    assert two.returncode == 0, two.stderr
    one = run("emdepth", ["--gc-values", gc, "--level", "60", plain], {"GOLEFT_EMDEPTH_TIMING": "1"})
    assert one.returncode == 0, one.stderr
    assert one.stdout == two.stdout
    assert one.stdout == want
    assert '"debias_chunks": 5' in one.stderr and '"medians_kernels_s"' in one.stderr
    # without the debiasing the copy numbers follow the covariate
    p = run("emdepth", ["--normalize", "--level", "60", plain])
    assert p.returncode == 0 and p.stdout == raw, p.stderr
    differ = [a != b for a, b in zip(one.stdout.split("\n"), p.stdout.split("\n"))]
    assert sum(differ) == MISCALLED_ROWS
    # --normalize beside the GC flags is allowed and changes nothing; so do blocks of rows and --cnvs
    c1, c2 = str(d / "c1.tsv"), str(d / "c2.tsv")
    p = run("emdepth", ["--normalize", "--gc-values", gc, "--gc-window", "0.01", "--level=60", "--cnvs", c1, plain],
            {"GOLEFT_EMDEPTH_ROWS": "7"})
    assert p.returncode == 0 and p.stdout == want, p.stderr
    p = run("emdepth", ["--normalize", "--level", "60", "--cnvs", c2, str(deb)])
    assert p.returncode == 0 and p.stdout == want, p.stderr
    with open(c1) as a, open(c2) as b:
        calls = a.read()
        assert calls == b.read() and calls.startswith("#sample\t")


def test_the_default_level_is_the_undebiased_middle_median(files):
    d, plain, gc = files
    want = expected(None)[1]
    p = run("emdepth", ["--gc-values", gc, plain])
    assert p.returncode == 0 and p.stdout == want, p.stderr
    p = run("emdepth", ["--gc-values", gc, "--level", "%g" % DEFAULT_LEVEL, plain])
    assert p.returncode == 0 and p.stdout == want, p.stderr
    # a level of its own
    p = run("emdepth", ["--gc-values", gc, "--level", "45", plain])
    assert p.returncode == 0 and p.stdout == expected(45.0)[1], p.stderr


CONTIGS = (("chr2", 15000), ("chrX", 700), ("chr1", 25000))     # the .fai's order is not the matrix's


def fasta_text():
    """(text, .fai text, {name: bases}): a GC gradient along each contig, a lower-case stretch, some N"""
    rng = np.random.default_rng(17)
    text, fai, seqs = "", "", {}
    for name, length in CONTIGS:
        p_gc = np.linspace(0.25, 0.65, length) if name == "chr1" else np.linspace(0.6, 0.3, length)
        gc = rng.random(length) < p_gc
        bases = np.where(gc, np.where(rng.random(length) < 0.5, ord("G"), ord("C")),
                         np.where(rng.random(length) < 0.5, ord("A"), ord("T"))).astype(np.uint8)
        seq = bytearray(bases.tobytes())
        seq[100:400] = bytes(seq[100:400]).lower()                    # soft-masked, inside the first row's interval
        seq[300:330] = b"N" * 30
        seq[length - 200:length - 150] = b"n" * 50
        seqs[name] = bytes(seq)
        text += ">%s some words\n" % name
        fai += "%s\t%d\t%d\t60\t61\n" % (name, length, len(text))
        text += "".join(seq[i:i + 60].decode() + "\n" for i in range(0, length, 60))
    return text, fai, seqs


@pytest.mark.parametrize("contract", ("faidx", "window"))
def test_fasta_gives_the_oracles_gc(files, contract):
    d, plain, gc = files
    text, fai, seqs = fasta_text()
    fa = d / "ref.fa"
    fa.write_text(text)
    (d / "ref.fa.fai").write_text(fai)
    want = []
    for i in range(ROWS):
        chrom, start, end = where(i).split("\t")
        s, e = max(int(start), 250) - 250, int(end)
        n_gc, _, _, n_acgt, _ = po.seq_counts(seqs[chrom], s, e)
        assert n_gc == po.seq_stats(seqs[chrom], s, e)[0]
        tot = float(n_acgt) if contract == "faidx" else float(e - s)
        want.append(n_gc / tot)
    assert where(0).split("\t")[1] == "0" and len(set(want)) > ROWS - 5      # (a gradient: next to no ties)
    env = {"GOLEFT_STATS_CONTRACT": contract}
    p = run("debias", ["--fasta", str(fa), plain], env)
    assert p.returncode == 0, p.stderr
    lines = [ln.split("\t") for ln in p.stderr.split("\n") if ln.startswith("chr")]
    assert ["\t".join(ln[:3]) for ln in lines] == [where(i) for i in range(ROWS)]
    assert [float(ln[3]) for ln in lines] == want
    vals_file = d / ("gc_%s.txt" % contract)
    vals_file.write_text("".join("%r\n" % v for v in want))
    q = run("debias", ["--gc-values", str(vals_file), plain])
    assert q.returncode == 0 and q.stdout == p.stdout, q.stderr
    m = cli_cells().astype(np.float32)
    assert p.stdout == DR.matrix_text(HEADER, [where(i) for i in range(ROWS)], DR.debias(m, want, WINDOW)[1])
    one = run("emdepth", ["--gc-fasta", str(fa), "--gc-window", "0.02", plain], env)
    two = run("emdepth", ["--gc-values", str(vals_file), "--gc-window", "0.02", plain])
    assert one.returncode == 0 and two.returncode == 0 and one.stdout == two.stdout, one.stderr + two.stderr


def test_error_exits(files):
    d, plain, gc = files
    text, fai, seqs = fasta_text()
    fa = d / "part.fa"
    fa.write_text(text)
    (d / "part.fa.fai").write_text("".join(ln + "\n" for ln in fai.split("\n") if ln and not ln.startswith("chr2\t")))
    for cmd, flag in (("debias", "--fasta"), ("emdepth", "--gc-fasta")):
        p = run(cmd, [flag, str(fa), plain])
        assert p.returncode == 1 and p.stdout == "" and "chromosome chr2" in p.stderr, p.stderr
    p = run("debias", ["--fasta", str(d / "none.fa"), plain])
    assert p.returncode == 1 and p.stdout == "" and "cannot open" in p.stderr
    short = d / "short.txt"
    short.write_text("".join("%r\n" % float(v) for v in vals()[:-1]))
    for cmd in ("debias", "emdepth"):
        p = run(cmd, ["--gc-values", str(short), plain])
        assert p.returncode == 1 and p.stdout == "" and "line 39" in p.stderr and "40 rows" in p.stderr, p.stderr
    long_ = d / "long.txt"
    long_.write_text("".join("%r\n" % float(v) for v in vals()) + "0.5\n")
    p = run("debias", ["--gc-values", str(long_), plain])
    assert p.returncode == 1 and p.stdout == "" and "line 41" in p.stderr
    for bad in ("x", "nan", "", "0.4 0.5"):
        f = d / "badval.txt"
        f.write_text("0.4\n0.41\n%s\n" % bad + "0.4\n" * 37)
        p = run("debias", ["--gc-values", str(f), plain])
        assert p.returncode == 1 and p.stdout == "" and "line 3" in p.stderr, (bad, p.stderr)
    # usage errors
    assert run("debias", [plain]).returncode == 255                           # no covariate
    assert run("debias", ["--gc-values", gc, "--fasta", "ref.fa", plain]).returncode == 255
    assert run("debias", ["--gc-values", gc]).returncode == 255
    assert run("debias", ["--gc-values", gc, "--level", "3", plain]).returncode == 255      # emdepth's flag
    assert run("debias", ["--gc-fasta", "ref.fa", plain]).returncode == 255
    for w in ("0", "-1", "nan", "inf", "x", ""):
        assert run("debias", ["--gc-values", gc, "--window=" + w, plain]).returncode == 255, w
        assert run("emdepth", ["--gc-values", gc, "--gc-window=" + w, plain]).returncode == 255, w
    f = d / "f.txt"
    f.write_text("1\n" * N)
    for flag, v in (("--gc-values", gc), ("--gc-fasta", "ref.fa")):
        p = run("emdepth", [flag, v, "--scales", str(f), plain])
        assert p.returncode == 255 and p.stdout == "" and "--scales" in p.stderr
    assert run("emdepth", ["--gc-values", gc, "--gc-fasta", "ref.fa", plain]).returncode == 255
    p = run("emdepth", ["--gc-window", "0.02", plain])
    assert p.returncode == 255 and "--gc-window" in p.stderr
    assert run("emdepth", ["--fasta", "ref.fa", plain]).returncode == 255      # debias's spelling
    # a quotient that overflows float32 has no text
    big = cli_cells().astype(np.float64)
    cells = [["%.9g" % v for v in row] for row in big]
    for r in range(0, ROWS, 5):
        cells[r][3] = "1e-45"
    cells[0][3] = "3e38"
    over = d / "over.bed"
    over.write_text(HEADER + "\n" + "".join("%s\t%s\n" % (where(i), "\t".join(row)) for i, row in enumerate(cells)))
    p = run("debias", ["--gc-values", gc, str(over)])
    assert p.returncode == 1 and p.stdout == "" and "row 1, sample 4" in p.stderr, p.stderr
    # without the new flags emdepth does what it did
    assert run("emdepth", [plain]).returncode == 0
