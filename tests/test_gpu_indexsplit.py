"""GPU: `indexsplit` -- the cohort's cell sums through the ABI, bit for bit against a numpy loop that adds
sizes.astype(float64) / 1e9 sample after sample, whatever the batching; `goleft-depth indexsplit` byte for byte against
the restatement of indexsplit.go (tests/indexsplit_ref.py); and `goleft-depth samplename` against covstats_ref's Names.
Every CLI call runs under its own timeout; nothing is retried."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from goleft_amd import _lib
from tests import covstats_ref as CR
from tests import indexcov_ref as IR
from tests import indexsplit_ref as R
from tests.helpers import ROOT

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "goleft_amd", "goleft-depth")
GOLD = os.path.join(ROOT, "tests", "golden", "ref")
E_INVALID, E_STATE, E_RANGE, E_CAPACITY = -1, -4, -5, -8


# ---- through the ABI ----------------------------------------------------------------------------------------------------
class Ctx:
    def __init__(self):
        self.lib = _lib.load()
        self.h = C.c_void_p()
        assert self.lib.gd_create(0, C.byref(self.h)) == 0

    def ok(self, rc):
        assert rc == 0, self.lib.gd_last_error(self.h).decode()

    def close(self):
        self.lib.gd_destroy(self.h)


@pytest.fixture(scope="module")
def ctx():
    c = Ctx()
    yield c
    c.close()


def layout(samples, Rn):
    """samples: per sample a list (one per reference) of int64 size arrays -> the arrays of gd_indexsplit_add."""
    flat, soff, toff, tcnt = [np.zeros(0, np.int64)], [0], [], []
    for s in samples:
        at = soff[-1]
        for r in range(Rn):
            toff.append(at)
            tcnt.append(len(s[r]))
            at += len(s[r])
            flat.append(np.asarray(s[r], np.int64))
        soff.append(at)
    return (np.array(soff, np.int64), np.ascontiguousarray(np.concatenate(flat), np.int64), np.array(toff, np.int64),
            np.array(tcnt, np.int32))


def add(ctx, samples, Rn):
    soff, sizes, toff, tcnt = layout(samples, Rn)
    return ctx.lib.gd_indexsplit_add(ctx.h, len(samples), soff.ctypes.data, sizes.ctypes.data, toff.ctypes.data, tcnt.ctypes.data)


def sums(ctx, n):
    out = np.full(n, np.nan)
    ctx.ok(ctx.lib.gd_indexsplit_sums(ctx.h, out.ctypes.data, n))
    return out


def device(ctx, samples, longest, batches=None):
    """The cell vector after the samples were added in batches of the given sizes (the rest in a last one)."""
    L = np.array(longest, np.int32)
    ctx.ok(ctx.lib.gd_indexsplit_begin(ctx.h, len(L), L.ctypes.data))
    at = 0
    for n in list(batches or []) + [len(samples)]:
        part = samples[at:at + n]
        at += len(part)
        if part:
            ctx.ok(add(ctx, part, len(L)))
    assert at == len(samples)
    return sums(ctx, int(L.sum()))


def numpy_cells(samples, longest):
    cells = [np.zeros(l, np.float64) for l in longest]
    for s in samples:                                        # sample after sample: the reference's order of additions
        for r, v in enumerate(s):
            cells[r][:len(v)] += np.asarray(v, np.int64).astype(np.float64) / 1e9
    return np.concatenate(cells)


def random_cohort(rng, N, tiles):
    """Ragged: shorter samples, samples without a reference, zeros, sizes above 2^53 (odd ones: not doubles)."""
    out = []
    for s in range(N):
        scale = rng.uniform(0.3, 3)
        per = []
        for r, t in enumerate(tiles):
            v = (rng.integers(2000, 60000, t) * scale).astype(np.int64)
            v[rng.integers(0, t, max(1, t // 40))] = 0
            big = rng.integers(0, t, 3)
            v[big] = (1 << 53) + 1 + 2 * rng.integers(0, 1 << 40, 3) + (rng.integers(0, 512, 3) << 53)
            v[int(rng.integers(0, t))] = int(rng.integers(1, 1 << 62)) | 1
            if s % 5 == 4 and r == len(tiles) - 2:
                v = v[:t // 2]
            if s % 3 == 2 and r == len(tiles) - 1:
                v = v[:rng.integers(1, t)]
            if s % 7 == 6 and r == 0:
                v = v[:0]                                    # a sample without this reference
            per.append(v)
        if s % 4 == 3:
            per[-1] = per[-1][:0]                            # an index with fewer references
        out.append(per)
    return out


def longest_of(samples, Rn):
    return [max(len(s[r]) for s in samples) for r in range(Rn)]


@pytest.mark.parametrize("N,tiles", [(1, (300, 40)), (2, (64, 33)), (7, (1000, 129, 77)), (64, (900, 310, 65, 120)),
                                     (300, (257, 100, 31))])
def test_abi_bit_exact_against_numpy(ctx, N, tiles):
    rng = np.random.default_rng(100 + N)
    samples = random_cohort(rng, N, tiles)
    longest = longest_of(samples, len(tiles))
    want = numpy_cells(samples, longest)
    assert (np.concatenate([np.concatenate(s) for s in samples]) > (1 << 53)).sum() >= N
    got = device(ctx, samples, longest)
    print(N, tiles, "cells", len(want), "differing", int((got.view(np.uint64) != want.view(np.uint64)).sum()))
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    # a reference nobody has, and references beyond the grid's second dimension
    wide = [[s[0]] + [np.zeros(0, np.int64)] * 3 + [s[1]] for s in samples[:3]]
    lw = longest_of(wide, 5)
    assert np.array_equal(device(ctx, wide, lw).view(np.uint64), numpy_cells(wide, lw).view(np.uint64))


def test_many_references(ctx):
    # more references than a grid has rows (65 535): the kernel strides over them
    rng = np.random.default_rng(3)
    Rn = 70000
    samples = [[rng.integers(0, 1 << 40, int(n)) for n in rng.integers(0, 4, Rn)] for _ in range(3)]
    longest = longest_of(samples, Rn)
    got = device(ctx, samples, longest, batches=[2])
    assert np.array_equal(got.view(np.uint64), numpy_cells(samples, longest).view(np.uint64))


def test_batching_does_not_change_a_bit(ctx):
    rng = np.random.default_rng(64)
    tiles = (700, 210, 65)
    samples = random_cohort(rng, 64, tiles)
    longest = longest_of(samples, len(tiles))
    one = device(ctx, samples, longest)
    cut = device(ctx, samples, longest, batches=[1, 7])     # 1, 7 and the 56 that are left
    each = device(ctx, samples, longest, batches=[1] * 63)
    want = numpy_cells(samples, longest)
    # the order matters to these sums: the same samples reversed give other bits somewhere
    assert not np.array_equal(numpy_cells(samples[::-1], longest).view(np.uint64), want.view(np.uint64))
    for got in (one, cut, each):
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64))


def test_bad_layouts_are_refused_and_leave_nothing_behind():
    c = Ctx()
    try:
        lib, h = c.lib, c.h
        buf = np.zeros(8)
        one = [[np.array([5, 6, 7], np.int64), np.array([1], np.int64)]]
        assert add(c, one, 2) == E_STATE and lib.gd_indexsplit_sums(h, buf.ctypes.data, 8) == E_STATE
        L = np.array([3, 2], np.int32)
        c.ok(lib.gd_indexsplit_begin(h, 2, L.ctypes.data))
        c.ok(add(c, one, 2))
        before = sums(c, 5)
        assert before.tolist() == [5e-9, 6e-9, 7e-9, 1e-9, 0.0]
        assert lib.gd_indexsplit_sums(h, buf.ctypes.data, 4) == E_CAPACITY and b"5 cells" in lib.gd_last_error(h)
        # more tiles than begin was told
        assert add(c, [[np.array([1, 2, 3, 4], np.int64), np.zeros(0, np.int64)]], 2) == E_RANGE
        assert b"reference 0" in lib.gd_last_error(h)
        # a negative size
        assert add(c, [[np.array([1, -2, 3], np.int64), np.zeros(0, np.int64)]], 2) == E_INVALID
        # tiles outside their sample, sample_off that does not start at 0 or decreases, no samples
        soff, sizes, toff, tcnt = layout(one + one, 2)
        bad = toff.copy(); bad[2] = 0
        assert lib.gd_indexsplit_add(h, 2, soff.ctypes.data, sizes.ctypes.data, bad.ctypes.data, tcnt.ctypes.data) == E_RANGE
        bad = tcnt.copy(); bad[3] = 2
        assert lib.gd_indexsplit_add(h, 2, soff.ctypes.data, sizes.ctypes.data, toff.ctypes.data, bad.ctypes.data) == E_RANGE
        bad = tcnt.copy(); bad[0] = -1
        assert lib.gd_indexsplit_add(h, 2, soff.ctypes.data, sizes.ctypes.data, toff.ctypes.data, bad.ctypes.data) == E_RANGE
        bad = soff.copy(); bad[0] = 1
        assert lib.gd_indexsplit_add(h, 2, bad.ctypes.data, sizes.ctypes.data, toff.ctypes.data, tcnt.ctypes.data) == E_INVALID
        bad = soff.copy(); bad[2] = 1
        assert lib.gd_indexsplit_add(h, 2, bad.ctypes.data, sizes.ctypes.data, toff.ctypes.data, tcnt.ctypes.data) in (E_INVALID, E_RANGE)
        assert lib.gd_indexsplit_add(h, 0, soff.ctypes.data, sizes.ctypes.data, toff.ctypes.data, tcnt.ctypes.data) == E_RANGE
        assert lib.gd_indexsplit_add(h, 2, None, sizes.ctypes.data, toff.ctypes.data, tcnt.ctypes.data) == E_INVALID
        # none of it reached the sums, and the state still takes a good batch
        assert np.array_equal(sums(c, 5).view(np.uint64), before.view(np.uint64))
        c.ok(add(c, one, 2))
        assert sums(c, 5).tolist() == [5e-9 + 5e-9, 6e-9 + 6e-9, 7e-9 + 7e-9, 1e-9 + 1e-9, 0.0]
        # a refused begin drops what was there
        for n_refs, longest in ((0, [1]), (2, [3, -1]), (2, [3, (1 << 24) + 1])):
            c.ok(lib.gd_indexsplit_begin(h, 2, L.ctypes.data))
            bad = np.array(longest, np.int32)
            assert lib.gd_indexsplit_begin(h, n_refs, bad.ctypes.data) == E_RANGE
            assert lib.gd_indexsplit_sums(h, buf.ctypes.data, 8) == E_STATE and add(c, one, 2) == E_STATE
        # begin zeroes: nothing of the earlier cohort is left
        c.ok(lib.gd_indexsplit_begin(h, 2, L.ctypes.data))
        assert sums(c, 5).tolist() == [0.0] * 5
        # no reference has a tile
        Z = np.zeros(2, np.int32)
        c.ok(lib.gd_indexsplit_begin(h, 2, Z.ctypes.data))
        c.ok(add(c, [[np.zeros(0, np.int64)] * 2], 2))
        c.ok(lib.gd_indexsplit_sums(h, None, 0))
    finally:
        c.close()


# ---- the CLI against the restatement ------------------------------------------------------------------------------------
def cli(args, timeout=600, word="indexsplit", env=None):
    r = subprocess.run([EXE, word] + [str(a) for a in args], capture_output=True, text=True, timeout=timeout,
                       env=dict(os.environ, **(env or {})))
    return r.returncode, r.stdout, r.stderr


def check(paths, N, fai=None, problematic=None):
    args = ["-n", N] + (["--fai", fai] if fai else []) + (["-p", problematic] if problematic else []) + list(paths)
    try:
        want = R.indexsplit([str(p) for p in paths], N, fai=fai, problematic=problematic)
    except R.Fatal as e:
        rc, out, err = cli(args)
        assert rc == 1 and out == "" and os.path.sep in str(e) and str(e) in err, (rc, out, str(e), err)
        return None
    rc, out, err = cli(args)
    assert rc == 0, err
    if out != want:
        g, w = out.splitlines(), want.splitlines()
        first = next((i for i, (x, y) in enumerate(zip(g, w)) if x != y), min(len(g), len(w)))
        print("rows", len(g), len(w), "first difference at", first, g[first:first + 2], w[first:first + 2])
    assert out == want
    return want


@pytest.mark.parametrize("name", ["t.bam", "hla.bam", "t-empty.bam", "sample_issue_27_0001.bam"])
@pytest.mark.parametrize("N", [1, 5, 40])
def test_reference_fixtures_singly(name, N):
    want = check([os.path.join(GOLD, name)], N)
    assert (want is None) == (name in ("hla.bam", "t-empty.bam"))
    if want is not None and N == 1:
        assert R.partition_gaps(want, IR.bam_header(os.path.join(GOLD, name))[1]) == []


def test_reference_fixtures_together():
    paths = [os.path.join(GOLD, n) for n in ("t.bam", "sample_issue_27_0001.bam")]
    for N in (1, 7, 1000):
        assert check(paths, N) is not None
        assert check(paths[::-1], N) is not None             # the references are the first input's


def test_bare_bai_with_a_fai(tmp_path):
    bam = os.path.join(GOLD, "sample_issue_27_0001.bam")
    _, refs = IR.bam_header(bam)
    fai = tmp_path / "ref.fai"
    off = 6
    lines = []
    for name, ln in refs:
        lines.append("%s\t%d\t%d\t60\t61\n" % (name, ln, off))
        off += ln + ln // 60 + len(name) + 2
    fai.write_text("".join(reversed(lines)))                 # ReadFai sorts by offset, not by line
    want = check([bam + ".bai"], 20, fai=str(fai))
    assert want is not None and want == R.indexsplit([bam], 20)


HOT = (2.5, 4.0, 5.5, 7.0, 8.5, 10.0, 11.5, 13.0)
CHROMS = [str(i) for i in range(1, 23)] + ["X", "Y", "GL000201.1", "decoy", "chrUn_late"]


def synth_cohort(d, N, seed):
    """N .bai files over CHROMS: shared structure, a centromere of tiles without reads, hot tiles of several heights
    early on eight chromosomes, `decoy` without a tile in any sample, `chrUn_late` in the .fai only, a few samples
    short of a chromosome's end and a few whose index ends two references early; returns (paths, fai, refs)."""
    rng = np.random.default_rng(seed)
    tiles = [int(rng.integers(60, 160)) for _ in range(22)] + [80, 40, 12, 0]
    shape = [rng.integers(40000, 70000, t).astype(np.float64) for t in tiles]
    for r in range(3):
        shape[r][50:58] = 0
    # every sixth tile of eight chromosomes is hot, each chromosome at its own height: a sixth of the tiles is enough to
    # keep them below mean + 3 sd, so chop leaves them and they are cut 2 .. 8 ways at N = 1000; chromosome 20 has one
    # tile far above it, which chop turns into 8 means
    for r, h in zip(range(8, 16), HOT):
        shape[r][3::6] *= h
    shape[19][30] *= 40
    os.makedirs(str(d), exist_ok=True)
    paths = []
    for s in range(N):
        scale = rng.uniform(0.5, 2.0)
        refs = []
        at = 1 << 20
        for r, t in enumerate(tiles):
            v = (shape[r] * scale * rng.uniform(0.9, 1.1, t)).astype(np.int64)
            if s % 13 == 5 and r == 6:
                v = v[:len(v) // 3]
            iv = np.concatenate([[at], at + np.cumsum(v)]).astype(np.uint64) if len(v) else np.zeros(0, np.uint64)
            at = int(iv[-1]) + 4096 if len(iv) else at
            refs.append((iv, None))
        if s % 11 == 3:
            refs = refs[:-2]
        p = os.path.join(str(d), "s%03d.bai" % s)
        IR.write_bai(p, refs)
        paths.append(p)
    fai = os.path.join(str(d), "ref.fai")
    lengths = [t * 16384 - int(rng.integers(0, 16000)) if t else 4000 for t in tiles] + [9000]
    with open(fai, "w") as f:
        off = 10
        for c, ln in zip(CHROMS, lengths):
            f.write("%s\t%d\t%d\t60\t61\n" % (c, ln, off))
            off += ln + 100
    bed = os.path.join(str(d), "problematic.bed")
    with open(bed, "w") as f:
        f.write("1\t100000\t900000\n2\t16384\t32768\nX\t0\t50000\nX\t70000\t70000\n7:1-3000000\ndecoy\t0\t100\n22\t0\t100000")
    return paths, fai, bed, list(zip(CHROMS, lengths))


@pytest.fixture(scope="module")
def cohort(tmp_path_factory):
    return synth_cohort(tmp_path_factory.mktemp("cohort"), 64, 2025)


@pytest.mark.parametrize("with_p", [False, True])
def test_cohort_of_64(cohort, with_p):
    paths, fai, bed, refs = cohort
    kinds, threes = set(), {}
    for N in (1, 10, 1000, 100000):
        want = check(paths, N, fai=fai, problematic=bed if with_p else None)
        assert want is not None
        splits = [int(ln.split("\t")[4]) for ln in want.splitlines()]
        kinds |= set(splits)
        print("N", N, "-p" if with_p else "", "rows", len(splits), "splits", sorted(set(splits)))
        if N <= 10:
            assert R.partition_gaps(want, refs) == []        # (the restatement's rows; the CLI wrote the same bytes)
        if N == 1000:
            # every kind of row in one run: references without data, whole regions, tiles cut 2 .. 8 ways
            assert set(splits) == set(range(9)), sorted(set(splits))
            threes[with_p] = splits.count(3)
        if N == 100000:
            assert splits.count(8) > 20000
    assert kinds == set(range(9)), sorted(kinds)
    if with_p:
        # the regions matter: more rows at N = 10, and at N = 1000 the pieces of three that hold less than a quarter chunk
        assert len(check(paths, 10, fai=fai, problematic=bed)) > len(check(paths, 10, fai=fai))
        assert threes[True] > 3 * R.indexsplit(paths, 1000, fai=fai).count("\t3\n") > 0


def test_python_entry_writes_the_same_bytes(cohort, tmp_path):
    from goleft_amd import indexsplit
    paths, fai, bed, _ = cohort
    rc, out, err = cli(["-n", 1000, "--fai", fai, "-p", bed] + paths[:9])
    assert rc == 0, err
    dst = tmp_path / "regions.bed"
    assert indexsplit.Main(["-n", "1000", "--fai", fai, "-p", bed] + paths[:9], out_path=str(dst)) == 0
    assert dst.read_text() == out and out == R.indexsplit(paths[:9], 1000, fai=fai, problematic=bed)


def test_timing_line(cohort):
    import json
    paths, fai, _, refs = cohort
    rc, out, err = cli(["-n", 100, "--fai", fai] + paths, env={"GOLEFT_INDEXSPLIT_TIMING": "1"})
    assert rc == 0, err
    t = json.loads(err.strip().splitlines()[-1])
    print(t)
    # (the last two references have no tile in any index; every other one ends inside its last tile)
    assert t["samples"] == 64 and t["references"] == len(CHROMS)
    assert t["cells"] == sum((ln + 16383) // 16384 for _, ln in refs[:-2]) > 2000
    for k in ("index_read_s", "upload_s", "kernel_s", "readback_s", "scan_s", "total_s"):
        assert t[k] >= 0


# ---- errors -------------------------------------------------------------------------------------------------------------
def failing(args, named, rc_want=1):
    rc, out, err = cli(args)
    assert rc == rc_want and named in err and out == "", (rc, out, err)


def test_errors_name_the_argument_and_print_no_rows(tmp_path, cohort):
    paths, fai, bed, _ = cohort
    failing(["-n", 10, "--fai", fai, paths[0], str(tmp_path / "x.crai")], "x.crai")
    failing(["-n", 10, "--fai", fai, str(tmp_path / "y.cram")], "y.cram")
    failing(["-n", 10, "--fai", fai, paths[0], str(tmp_path / "gone.bai")], "gone.bai")
    failing(["-n", 10, paths[0]], "s000.bai")                # a bare .bai without --fai
    failing(["-n", 10, "--fai", str(tmp_path / "no.fai"), paths[0]], "no.fai")
    failing(["-n", 10, "--fai", fai, "-p", str(tmp_path / "no.bed"), paths[0]], "no.bed")
    bad = str(tmp_path / "dec.bai")
    IR.write_bai(bad, [(np.array([1 << 20, 3 << 20, 2 << 20, 4 << 20], np.uint64), None)])
    failing(["-n", 10, "--fai", fai, paths[0], bad], "dec.bai")
    zero = str(tmp_path / "zero.bai")
    IR.write_bai(zero, [(np.array([1 << 20] * 5, np.uint64), None)])
    failing(["-n", 10, "--fai", fai, zero], "zero.bai")      # a cohort without data
    with pytest.raises(R.Fatal):
        R.indexsplit([zero], 10, fai=fai)
    refs = [("c1", 1 << 20)]
    noidx = str(tmp_path / "noidx.bam")
    CR.write_bam(noidx, refs, [CR.Rec(0, 100 * i, 0x3, 100 * i + 300, 500, ((0, 100),)) for i in range(10)], index=False)
    failing(["-n", 10, noidx], "noidx.bam")
    failing(["--fai", fai, paths[0]], "--n", rc_want=255)
    failing(["-n", 0, "--fai", fai, paths[0]], "-n", rc_want=255)
    failing(["-n", 10, "--fai", fai], "indexes", rc_want=255)


# ---- samplename ---------------------------------------------------------------------------------------------------------
def header_bam(tmp_path, name, rg_lines):
    p = str(tmp_path / name)
    text = "@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:c1\tLN:1048576\n" + "".join(ln + "\n" for ln in rg_lines)
    CR.write_bam(p, [("c1", 1 << 20)], [CR.Rec(0, 100, 0x3, 400, 500, ((0, 100),))], header_text=text, index=False)
    return p, text


def samplename(args):
    return cli(args, word="samplename", timeout=120, env={"HIP_VISIBLE_DEVICES": "", "ROCR_VISIBLE_DEVICES": ""})


@pytest.mark.parametrize("name", ["t.bam", "hla.bam", "t-empty.bam", "sample_issue_27_0001.bam"])
def test_samplename_on_the_reference_fixtures(name):
    p = os.path.join(GOLD, name)
    names = CR.sample_names(IR.bam_header(p)[0])
    rc, out, err = samplename([p])                           # (no device is visible to it: it needs none)
    assert rc == 0 and out == "\n".join(names) + "\n", (out, err)
    rc, out, err = samplename(["-e", p])
    if len(names) == 1:
        assert rc == 0 and out == names[0] + "\n"
    else:
        assert rc != 0 and out == "" and "goleft/samplename: found multiple samples in %s" % p in err


def test_samplename_on_synthetic_headers(tmp_path):
    cases = [
        ("one.bam", ["@RG\tID:a\tPL:x\tSM:alpha\tLB:l"], ["alpha"]),
        ("nosm.bam", ["@RG\tID:a\tPL:x"], []),
        ("none.bam", [], []),
        ("many.bam", ["@RG\tID:a\tSM:zeta", "@RG\tID:b\tSM:alpha", "@RG\tID:c", "@RG\tID:d\tSM:zeta", "@RG\tID:e\tSM:mid"],
         ["zeta", "alpha", "mid"]),
        ("same.bam", ["@RG\tID:a\tSM:s1", "@RG\tID:b\tSM:s1"], ["s1"]),
    ]
    for name, rgs, want in cases:
        p, text = header_bam(tmp_path, name, rgs)
        assert CR.sample_names(text) == want
        rc, out, err = samplename([p])
        assert rc == 0 and out == "\n".join(want) + "\n", (name, out, err)
        rc, out, err = samplename(["-e", p])
        if len(want) == 1:
            assert rc == 0 and out == want[0] + "\n", (name, out, err)
        else:
            assert rc != 0 and out == "" and "goleft/samplename: found multiple samples in %s" % p in err, (name, rc, out, err)
    rc, out, err = samplename([str(tmp_path / "gone.bam")])
    assert rc == 1 and out == "" and "gone.bam" in err
    rc, out, err = samplename([])
    assert rc == 255 and out == ""
