#!/usr/bin/env python3
"""Record what `goleft-depth` answers to argvs and inputs it refuses BEFORE it opens the device: exit code, stdout and
stderr of every case of CASES, written as tests/cli_refusals.json, which tests/test_cli_refusals.py replays.

    python tools/record_cli_cases.py --exe /path/to/a/build/of/the/PARENT/commit/goleft-depth [--out tests/cli_refusals.json]

The recorded values are a reference, so they come from a build of the commit BEFORE the change under test, never from
the change itself.  A case is (name, subcommand, argv, files, env): the files are written into a fresh directory that is
the working directory of the run, so every path in an argv is relative and every message is stable; a file whose name
ends in .gz is gzipped.  No case may reach gd_create: the recorder refuses a stderr that says the device was looked for
(on a machine with a device such a case would succeed)."""
import argparse
import gzip
import json
import os
import subprocess
import sys
import tempfile

HEADER = "#chrom\tstart\tend\ta\tb\tc\n"
ROWS = ("chr1\t0\t1000\t10\t20\t30\n", "chr1\t1000\t2000\t11\t21\t31\n", "chr2\t0\t1000\t12\t22\t32\n")
GOOD = HEADER + "".join(ROWS)


def with_cell(text):
    """GOOD with the second row's middle cell replaced"""
    return HEADER + ROWS[0] + "chr1\t1000\t2000\t11\t%s\t31\n" % text + ROWS[2]


SUBCOMMANDS = ("depth", "depthwed", "multidepth", "covstats", "indexcov", "indexsplit", "emdepth", "scales", "debias",
               "cnveval", "samplename")
M = {"m": GOOD}
BED_OK = "chr1\t1\t2\t3\ts\n"

CASES = []


def case(name, cmd, argv, files=None, env=None):
    assert cmd in SUBCOMMANDS and all(n != name for n, *_ in CASES), name
    CASES.append((name, cmd, list(argv), dict(files or {}), dict(env or {})))


for c in SUBCOMMANDS:
    case(c + " -h", c, ["-h"])
    case(c + " --help", c, ["--help"])
    case(c + " --help after a flag", c, ["--bogus", "--help"])
    case(c + " --bogus", c, ["--bogus", "x"])
    case(c + " --bogus=1", c, ["--bogus=1", "x"])
    case(c + " nothing", c, [])

# ---- depth (no `--`; the key is printed; --flag=true)
case("depth missing value", "depth", ["a.bam", "--prefix"])
case("depth no prefix", "depth", ["a.bam"])
case("depth no bam", "depth", ["--prefix", "p"])
case("depth two bams", "depth", ["--prefix", "p", "a.bam", "b.bam"])
case("depth --windowsize x", "depth", ["--windowsize", "x", "--prefix", "p", "a.bam"])
case("depth --windowsize 0", "depth", ["--windowsize", "0", "--prefix", "p", "a.bam"])
case("depth -w=0", "depth", ["-w=0", "--prefix=p", "a.bam"])
case("depth -Q 1x", "depth", ["-Q", "1x", "--prefix", "p", "a.bam"])
case("depth --mincov 3000000000", "depth", ["--mincov", "3000000000", "--prefix", "p", "a.bam"])
case("depth --", "depth", ["--prefix", "p", "--", "a.bam", "b.bam"])
case("depth --ordered=true --stats=false", "depth", ["--ordered=true", "--stats=false", "a.bam"])
case("depth -o takes no word", "depth", ["-o", "-s", "a.bam", "b.bam", "--prefix", "p"])
case("depth --bogus=1 --help", "depth", ["--bogus=1", "--help"])

# ---- depthwed
case("depthwed -s last", "depthwed", ["a.bed", "-s"])
case("depthwed --size=x", "depthwed", ["--size=x", "a.bed"])
case("depthwed -s 1x", "depthwed", ["-s", "1x", "a.bed"])
case("depthwed no size", "depthwed", ["a.bed"])
case("depthwed no beds", "depthwed", ["-s", "1000"])
case("depthwed -s 0", "depthwed", ["-s", "0", "a.bed"])

# ---- multidepth (no `--`; the key is printed)
case("multidepth missing value", "multidepth", ["a.bam", "-c"])
case("multidepth no chrom", "multidepth", ["a.bam"])
case("multidepth no bams", "multidepth", ["-c", "chr1"])
case("multidepth --q=x", "multidepth", ["--q=x", "-c", "chr1", "a.bam"])
case("multidepth --minsamples x", "multidepth", ["--minsamples", "x", "-c", "chr1", "a.bam"])
case("multidepth -w 1.5", "multidepth", ["-w", "1.5", "-c", "chr1", "a.bam"])
case("multidepth --", "multidepth", ["-c", "chr1", "--", "a.bam"])
case("multidepth a bam that is not there", "multidepth", ["-c", "chr1", "none.bam"])

# ---- covstats (the header goes out before the arguments are read)
case("covstats missing value", "covstats", ["a.bam", "-n"])
case("covstats -n 1x", "covstats", ["-n", "1x", "a.bam"])
case("covstats --n=", "covstats", ["--n=", "a.bam"])
case("covstats -n 9223372036854775808", "covstats", ["-n", "9223372036854775808", "a.bam"])
case("covstats -- and nothing", "covstats", ["-n", "5", "--"])
case("covstats -- -r", "covstats", ["--", "-r.cram"])
case("covstats a cram", "covstats", ["-r", "x.bed", "a.cram", "b.bam"])

# ---- indexcov
case("indexcov missing value", "indexcov", ["a.bam", "-d"])
case("indexcov no directory", "indexcov", ["a.bam"])
case("indexcov no bam", "indexcov", ["-d", "out"])
case("indexcov -c", "indexcov", ["-c", "chr1", "-d", "out", "a.bam"])
case("indexcov --chrom=chr1", "indexcov", ["--chrom=chr1"])
case("indexcov -c last", "indexcov", ["-c"])
case("indexcov -- and nothing", "indexcov", ["-d", "out", "-e", "-n", "--"])
case("indexcov -- -d", "indexcov", ["--", "-d", "out"])

# ---- indexsplit
case("indexsplit missing value", "indexsplit", ["a.bam", "--fai"])
case("indexsplit no n", "indexsplit", ["a.bam"])
case("indexsplit no indexes", "indexsplit", ["-n", "3"])
case("indexsplit -n 0", "indexsplit", ["-n", "0", "a.bam"])
case("indexsplit -n x", "indexsplit", ["-n", "x", "a.bam"])
case("indexsplit --n=", "indexsplit", ["--n=", "a.bam"])
case("indexsplit -n 2147483648", "indexsplit", ["-n", "2147483648", "a.bam"])
case("indexsplit -- and nothing", "indexsplit", ["-n", "3", "--"])
case("indexsplit -- -n", "indexsplit", ["--", "-n", "3"])
case("indexsplit a cram", "indexsplit", ["-n", "3", "a.bam", "b.cram"])
case("indexsplit a bai and no fai", "indexsplit", ["-n", "3", "a.bai"])
case("indexsplit a fai that is not there", "indexsplit", ["-n", "3", "--fai", "none.fai", "a.bai"])
case("indexsplit a problematic bed that is not there", "indexsplit", ["-n", "3", "-p", "none.bed", "a.bam"])

# ---- samplename
case("samplename two bams", "samplename", ["a.bam", "b.bam"])
case("samplename --", "samplename", ["--", "-e", "x"])
case("samplename -e=1", "samplename", ["-e=1", "a.bam"])
case("samplename a bam that is not there", "samplename", ["-e", "none.bam"])

# ---- cnveval: the flags, then the beds (the test set is read first, then the truth set)
case("cnveval missing value", "cnveval", ["a", "b", "-m"])
case("cnveval one bed", "cnveval", ["a"])
case("cnveval -m 0", "cnveval", ["-m", "0", "a", "b"])
case("cnveval -m 1.5", "cnveval", ["-m", "1.5", "a", "b"])
case("cnveval -m 2", "cnveval", ["-m", "2", "a", "b"])
case("cnveval -m x", "cnveval", ["--minoverlap=x", "a", "b"])
case("cnveval -m=", "cnveval", ["-m=", "a", "b"])
case("cnveval -s=1", "cnveval", ["-s=1", "a", "b"])
case("cnveval --limitsamples=true", "cnveval", ["--limitsamples=true", "a", "b"])
case("cnveval -- -s", "cnveval", ["--", "-s", "a", "b"])
case("cnveval -- in the middle", "cnveval", ["a", "--", "b", "-m"])
case("cnveval no test file", "cnveval", ["truth.bed", "none.bed"], {"truth.bed": BED_OK})
case("cnveval no truth file", "cnveval", ["none.bed", "test.bed"], {"test.bed": BED_OK})
case("cnveval four fields", "cnveval", ["truth.bed", "test.bed"], {"truth.bed": BED_OK, "test.bed": BED_OK + "chr1\t1\t2\t3\n"})
case("cnveval start not an integer", "cnveval", ["truth.bed", "test.bed"], {"truth.bed": BED_OK, "test.bed": "#c\n" + BED_OK + "chr1\tx\t2\t3\ts\n"})
case("cnveval end not an integer", "cnveval", ["truth.bed", "test.bed"], {"truth.bed": BED_OK, "test.bed": "chr1\t1\t2.5\t3\ts\n"})
case("cnveval copy number not an integer", "cnveval", ["truth.bed", "test.bed"], {"truth.bed": BED_OK, "test.bed": "chr1\t1\t2\t+\ts\n"})
case("cnveval end beyond int32", "cnveval", ["truth.bed", "test.bed"], {"truth.bed": BED_OK, "test.bed": "chr1\t1\t3000000000\t3\ts\n"})
case("cnveval a negative start", "cnveval", ["truth.bed", "test.bed"], {"truth.bed": BED_OK, "test.bed": "chr1\t-1\t2\t3\ts\n"})
case("cnveval end before start", "cnveval", ["truth.bed", "test.bed"], {"truth.bed": BED_OK, "test.bed": "chr1\t5\t2\t3\ts\n"})
case("cnveval an empty line", "cnveval", ["truth.bed", "test.bed"], {"truth.bed": BED_OK, "test.bed": BED_OK + "\n" + BED_OK})
case("cnveval an empty line with a carriage return", "cnveval", ["truth.bed", "test.bed"], {"truth.bed": BED_OK, "test.bed": "\r\n"})
case("cnveval a bad truth line after a good test set", "cnveval", ["truth.bed", "test.bed"],
     {"truth.bed": BED_OK + BED_OK + "chr1\t1\n", "test.bed": BED_OK + BED_OK})
case("cnveval a last line without a newline", "cnveval", ["truth.bed", "test.bed"], {"truth.bed": "chr1\t1\n", "test.bed": "chr1\t1\t2\t3\ts"})
case("cnveval a last line without a newline after two lines", "cnveval", ["truth.bed", "test.bed"],
     {"truth.bed": "chr1\tx\t2\t3\ts\n", "test.bed": "#c\n" + BED_OK + "chr1\t1\t2"})
case("cnveval gzipped", "cnveval", ["truth.bed.gz", "test.bed.gz"], {"truth.bed.gz": BED_OK, "test.bed.gz": BED_OK + BED_OK + "chr1\t7\t2\t3\ts\n"})

# ---- scales: its flags, then the matrix reader (the matrix is read before the device is opened)
case("scales missing value", "scales", ["m", "--level"], M)
case("scales --level 0", "scales", ["--level", "0", "m"], M)
case("scales --level inf", "scales", ["--level=inf", "m"], M)
case("scales --level=", "scales", ["--level=", "m"], M)
case("scales --normalize", "scales", ["--normalize", "m"], M)
case("scales --log2", "scales", ["--log2", "m"], M)
case("scales --scales", "scales", ["--scales", "s", "m"], M)
case("scales two matrices", "scales", ["m", "n"], M)
case("scales -- --level", "scales", ["--", "--level"], M)
case("scales -- in the middle", "scales", ["m", "--", "-h"], M)
case("matrix not there", "scales", ["none.bed"])
case("matrix empty", "scales", ["m"], {"m": ""})
case("matrix of one empty line", "scales", ["m"], {"m": "\n"})
case("matrix without a header", "scales", ["m"], {"m": "".join(ROWS)})
case("matrix header without samples", "scales", ["m"], {"m": "#chrom\tstart\tend\n" + "chr1\t0\t1000\n"})
case("matrix header chrom without samples", "scales", ["m"], {"m": "chrom\tstart\n"})
case("matrix of two samples", "scales", ["m"], {"m": "#chrom\tstart\tend\ta\tb\nchr1\t0\t1000\t10\t20\n"})
case("matrix short row", "scales", ["m"], {"m": HEADER + ROWS[0] + "chr1\t1000\t2000\t11\t21\n" + ROWS[2]})
case("matrix very short row", "scales", ["m"], {"m": HEADER + ROWS[0] + ROWS[1] + "chr2\n"})
case("matrix long row", "scales", ["m"], {"m": HEADER + ROWS[0] + "chr1\t1000\t2000\t11\t21\t31\t41\n" + ROWS[2]})
case("matrix long row with a bad extra cell", "scales", ["m"], {"m": HEADER + "chr1\t0\t1000\t10\t20\t30\tx\n"})
case("matrix cell not a number", "scales", ["m"], {"m": with_cell("x")})
case("matrix cell with a tail", "scales", ["m"], {"m": with_cell("21 ")})
case("matrix cell empty", "scales", ["m"], {"m": with_cell("")})
case("matrix cell nan", "scales", ["m"], {"m": with_cell("nan")})
case("matrix cell negative", "scales", ["m"], {"m": with_cell("-1")})
case("matrix cell beyond float32", "scales", ["m"], {"m": with_cell("1e39")})
case("matrix last cell bad", "scales", ["m"], {"m": HEADER + ROWS[0] + "chr1\t1000\t2000\t11\t21\t-0.5\n"})
case("matrix bad cell behind an empty line", "scales", ["m"], {"m": HEADER + ROWS[0] + "\n" + with_cell("x")[len(HEADER + ROWS[0]):]})
case("matrix bad cell with carriage returns", "scales", ["m"], {"m": with_cell("x").replace("\n", "\r\n")})
case("matrix bad cell in a last line without a newline", "scales", ["m"], {"m": HEADER + ROWS[0] + "chr1\t1000\t2000\t11\t21\tx"})
case("matrix gzipped with a bad cell", "scales", ["m.bed.gz"], {"m.bed.gz": with_cell("x")})
case("matrix gzipped with a long row", "scales", ["m.bed.gz"], {"m.bed.gz": GOOD + "chr2\t1000\t2000\t1\t2\t3\t4\n"})
case("matrix reader from debias", "debias", ["--gc-values", "g", "none.bed"])
case("matrix reader from emdepth", "emdepth", ["m"], {"m": with_cell("1e39")})

# ---- debias: its flags and every cross-flag check it can reach
G = ["--gc-values", "g"]
case("debias missing value", "debias", ["m", "--window"], M)
case("debias --window 0", "debias", G + ["--window", "0", "m"], M)
case("debias --window=", "debias", G + ["--window=", "m"], M)
case("debias --moving 4", "debias", G + ["--moving", "4", "m"], M)
case("debias --moving 257", "debias", G + ["--moving=257", "m"], M)
case("debias --moving x", "debias", G + ["--moving", "x", "m"], M)
case("debias --svd -1", "debias", ["--svd", "-1", "m"], M)
case("debias --svd x", "debias", ["--svd=x", "m"], M)
case("debias --level", "debias", G + ["--level", "3", "m"], M)
case("debias --gc-fasta", "debias", ["--gc-fasta", "f", "m"], M)
case("debias --gc-window", "debias", G + ["--gc-window", "0.1", "m"], M)
case("debias --normalize", "debias", G + ["--normalize", "m"], M)
case("debias --zscore=1", "debias", ["--svd", "5", "--zscore=1", "m"], M)
case("debias --log2=1", "debias", ["--svd", "5", "--log2=1", "m"], M)
case("debias no covariate", "debias", ["m"], M)
case("debias no matrix", "debias", G, M)
case("debias two matrices", "debias", G + ["m", "n"], M)
case("debias -- and nothing", "debias", G + ["--"], M)
case("debias -- --svd", "debias", G + ["--", "--svd", "5"], M)
case("debias --gc-values and --fasta", "debias", G + ["--fasta", "f", "m"], M)
case("debias --svd and --gc-values", "debias", ["--svd", "5"] + G + ["m"], M)
case("debias --svd and --fasta", "debias", ["--svd", "5", "--fasta", "f", "m"], M)
case("debias --svd and --window", "debias", ["--svd", "5", "--window", "0.1", "m"], M)
case("debias --svd and --moving", "debias", ["--svd", "5", "--moving", "9", "m"], M)
case("debias --zscore without --svd", "debias", G + ["--zscore", "m"], M)
case("debias --log2 without --svd", "debias", G + ["--log2", "m"], M)
case("debias --log2 and --zscore", "debias", ["--svd", "5", "--log2", "--zscore", "m"], M)
case("debias --window without a covariate", "debias", ["--window", "0.01", "m"], M)
case("debias --window and --moving", "debias", G + ["--window", "0.01", "--moving", "9", "m"], M)
case("debias pair: --svd --zscore --log2 --gc-values", "debias", ["--svd", "5", "--zscore", "--log2", "--gc-values", "g", "m"], M)
case("debias pair: --window --moving without a covariate", "debias", ["--window", "0.01", "--moving", "9", "m"], M)
case("debias pair: both covariates and --svd", "debias", G + ["--fasta", "f", "--svd", "5", "m"], M)
case("debias pair: --zscore alone and no matrix", "debias", G + ["--zscore"], M)
case("debias pair: --window --moving and no matrix", "debias", G + ["--window", "0.01", "--moving", "9"], M)

# ---- emdepth: its flags, every cross-flag check, then what it reads before the device
case("emdepth missing value", "emdepth", ["m", "--scales"], M)
case("emdepth --level x", "emdepth", ["--normalize", "--level", "x", "m"], M)
case("emdepth --level -1", "emdepth", ["--normalize", "--level=-1", "m"], M)
case("emdepth --gc-window 0", "emdepth", G + ["--gc-window", "0", "m"], M)
case("emdepth --gc-window nan", "emdepth", G + ["--gc-window", "nan", "m"], M)
case("emdepth --gc-moving 2", "emdepth", G + ["--gc-moving", "2", "m"], M)
case("emdepth --gc-moving 9x", "emdepth", G + ["--gc-moving", "9x", "m"], M)
case("emdepth --svd nan", "emdepth", ["--svd", "nan", "m"], M)
case("emdepth --svd 5%", "emdepth", ["--svd", "5%", "m"], M)
case("emdepth --cnvs=", "emdepth", ["--cnvs=", "m"], M)
case("emdepth --scales empty word", "emdepth", ["--scales", "", "m"], M)
case("emdepth --zscore", "emdepth", ["--svd", "5", "--zscore", "m"], M)
case("emdepth --fasta", "emdepth", ["--fasta", "f", "m"], M)
case("emdepth --window", "emdepth", G + ["--window", "0.1", "m"], M)
case("emdepth --normalize=1", "emdepth", ["--normalize=1", "m"], M)
case("emdepth two matrices", "emdepth", ["m", "n"], M)
case("emdepth -- --normalize", "emdepth", ["--", "--normalize", "m"], M)
case("emdepth --normalize and --scales", "emdepth", ["--normalize", "--scales", "s", "m"], M)
case("emdepth --gc-values and --gc-fasta", "emdepth", G + ["--gc-fasta", "f", "m"], M)
case("emdepth --log2 without --svd", "emdepth", ["--log2", "m"], M)
case("emdepth --svd and --scales", "emdepth", ["--svd", "5", "--scales", "s", "m"], M)
case("emdepth --gc-values and --scales", "emdepth", G + ["--scales", "s", "m"], M)
case("emdepth --gc-fasta and --scales", "emdepth", ["--gc-fasta", "f", "--scales", "s", "m"], M)
case("emdepth --gc-window without a covariate", "emdepth", ["--gc-window", "0.01", "m"], M)
case("emdepth --gc-moving without a covariate", "emdepth", ["--gc-moving", "9", "m"], M)
case("emdepth --gc-window and --gc-moving", "emdepth", G + ["--gc-window", "0.01", "--gc-moving", "9", "m"], M)
case("emdepth --level without --normalize", "emdepth", ["--level", "3", "m"], M)
case("emdepth --level with --scales", "emdepth", ["--level", "3", "--scales", "s", "m"], M)
case("emdepth pair: --svd --scales --normalize", "emdepth", ["--svd", "5", "--scales", "s", "--normalize", "m"], M)
case("emdepth pair: --log2 --zscore", "emdepth", ["--log2", "--zscore", "m"], M)
case("emdepth pair: --gc-window --gc-moving without a covariate", "emdepth", ["--gc-window", "0.01", "--gc-moving", "9", "m"], M)
case("emdepth pair: --svd --gc-values --scales", "emdepth", ["--svd", "5"] + G + ["--scales", "s", "m"], M)
case("emdepth pair: --level alone and no matrix", "emdepth", ["--level", "3"], M)
case("emdepth pair: --gc-moving alone and --level", "emdepth", ["--gc-moving", "9", "--level", "3", "m"], M)
case("emdepth scales file not there", "emdepth", ["--scales", "s", "m"], M)
case("emdepth too few factors", "emdepth", ["--scales", "s", "m"], {"m": GOOD, "s": "1\n\n 2 \n"})
case("emdepth too many factors", "emdepth", ["--scales", "s", "m"], {"m": GOOD, "s": "1\n2\n3\n4\n"})
case("emdepth a negative factor", "emdepth", ["--scales", "s", "m"], {"m": GOOD, "s": "1\n\n-2\n3\n"})
case("emdepth a factor that is no number", "emdepth", ["--scales=s.gz", "m"], {"m": GOOD, "s.gz": "1\n2\nx\n"})
case("emdepth a scaled depth beyond float32", "emdepth", ["--scales", "s", "m"], {"m": GOOD, "s": "1\n1\n3e38\n"})
case("emdepth --cnvs start not decimal", "emdepth", ["--cnvs", "out", "m"], {"m": GOOD + "chr2\t1e3\t2000\t1\t2\t3\n"})
case("emdepth --cnvs start empty", "emdepth", ["--cnvs", "out", "m"], {"m": GOOD + "chr2\t\t2000\t1\t2\t3\n"})
case("emdepth --cnvs start 4294967296", "emdepth", ["--cnvs", "out", "m"], {"m": HEADER + "chr1\t4294967296\t4294967297\t1\t2\t3\n"})
case("emdepth --cnvs end 4294967296", "emdepth", ["--cnvs", "out", "m"], {"m": GOOD + "\n" + "chr3\t4294967295\t4294967296\t1\t2\t3\n"})
case("emdepth --cnvs end negative", "emdepth", ["--cnvs=out", "m.gz"], {"m.gz": GOOD + "chr3\t5\t-6\t1\t2\t3\n"})
case("emdepth GOLEFT_EMDEPTH_ROWS=0", "emdepth", ["m"], M, {"GOLEFT_EMDEPTH_ROWS": "0"})


def run_case(exe, c, timeout=60):
    """(exit code, stdout, stderr) of one case: a fresh child process in a fresh working directory"""
    name, cmd, argv, files, env = c
    with tempfile.TemporaryDirectory() as d:
        for fn, text in files.items():
            data = text.encode()
            with open(os.path.join(d, fn), "wb") as f:
                f.write(gzip.compress(data, mtime=0) if fn.endswith(".gz") else data)
        base = {k: v for k, v in os.environ.items() if not k.startswith("GOLEFT_")}
        p = subprocess.run([exe, cmd] + argv, cwd=d, env=dict(base, **env), stdin=subprocess.DEVNULL, capture_output=True,
                           timeout=timeout)
        left = sorted(set(os.listdir(d)) - set(files))
    return p.returncode, p.stdout.decode(), p.stderr.decode(), left


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--exe", required=True, help="goleft-depth of a build of the parent commit")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "cli_refusals.json"))
    a = ap.parse_args()
    rows = []
    for c in CASES:
        code, out, err, left = run_case(os.path.abspath(a.exe), c)
        assert "no usable MI355X device" not in err, "%s reaches the device: %s" % (c[0], err)
        assert code in (1, 2, 255) or (code == 0 and any(h in c[2] for h in ("-h", "--help"))), (c[0], code, err)
        assert not left, "%s leaves %s behind" % (c[0], left)
        rows.append({"name": c[0], "cmd": c[1], "argv": c[2], "files": c[3], "env": c[4], "exit": code, "stdout": out, "stderr": err})
    with open(a.out, "w") as f:
        json.dump(rows, f, indent=0, sort_keys=True)
        f.write("\n")
    print("%d cases recorded in %s" % (len(rows), a.out))


if __name__ == "__main__":
    sys.exit(main())
