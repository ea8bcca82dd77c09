"""GPU: `indexcov` -- the device results through the ABI, bit for bit against numpy on the same inputs (medians, depths,
cells, slots, counters, copy numbers, pca8 bytes, the exact Gram matrix), and `goleft-depth indexcov` against the
restatement of indexcov.go (tests/indexcov_ref.py): BED (decompressed), .roc and .ped byte for byte except the PC
columns, which agree within one printed unit up to one sign per column.  Every CLI call runs under its own timeout;
nothing is retried."""
import ctypes as C
import gzip
import os
import subprocess

import numpy as np
import pytest

from goleft_amd import _hostlib, _lib
from tests import covstats_ref as CR
from tests import indexcov_ref as R
from tests.helpers import ROOT

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "goleft_amd", "goleft-depth")
GOLD = os.path.join(ROOT, "tests", "golden", "ref")
FIXTURES = ["t.bam", "hla.bam", "t-empty.bam", "sample_issue_27_0001.bam"]
F32 = np.float32


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


def device(ctx, samples, is_sex, depths=None, gram=True):
    """samples: per sample a list (one per reference) of int64 size arrays, every reference reported."""
    lib, h = ctx.lib, ctx.h
    N, Rn = len(samples), len(is_sex)
    flat, soff, toff, tcnt = [], [0], [], []
    for s in samples:
        at = soff[-1]
        for r in range(Rn):
            toff.append(at)
            tcnt.append(len(s[r]))
            at += len(s[r])
            flat.append(np.asarray(s[r], np.int64))
        soff.append(at)
    sizes = np.ascontiguousarray(np.concatenate(flat), np.int64)
    soff, toff = np.array(soff, np.int64), np.array(toff, np.int64)
    tcnt, sex = np.array(tcnt, np.int32), np.array(is_sex, np.uint8)
    ctx.ok(lib.gd_indexcov_upload(h, N, Rn, soff.ctypes.data, sizes.ctypes.data, toff.ctypes.data, tcnt.ctypes.data, sex.ctypes.data))
    med = np.zeros(N, np.int64)
    ctx.ok(lib.gd_indexcov_medians(h, med.ctypes.data))
    dep = np.zeros(len(sizes), np.float32)
    ctx.ok(lib.gd_indexcov_depths(h, dep.ctypes.data, dep.size))
    out = dict(median=med, depth=dep.copy(), soff=soff, toff=toff.reshape(N, Rn))
    if depths is not None:
        d = np.ascontiguousarray(depths, np.float32)
        ctx.ok(lib.gd_indexcov_set_depths(h, d.ctypes.data, d.size))
    ctx.ok(lib.gd_indexcov_compute(h, 1 if gram else 0))
    dims = _lib.GdIndexcovDims()
    longest, coff, xoff = np.zeros(Rn, np.int32), np.zeros(Rn, np.int64), np.zeros(Rn, np.int64)
    ctx.ok(lib.gd_indexcov_get_dims(h, C.byref(dims), longest.ctypes.data, coff.ctypes.data, xoff.ctypes.data))
    cells = np.zeros(dims.n_cells, np.uint32)
    ctx.ok(lib.gd_indexcov_cells(h, 0, dims.n_cells, cells.ctypes.data))
    slots = np.zeros((Rn, N, 70), np.int32)
    ctx.ok(lib.gd_indexcov_slots(h, slots.ctypes.data))
    counters = np.zeros((N, 4), np.int64)
    ctx.ok(lib.gd_indexcov_counters(h, counters.ctypes.data))
    cn = np.zeros((Rn, N), np.float64)
    ctx.ok(lib.gd_indexcov_cn(h, cn.ctypes.data))
    X = np.zeros((N, dims.m), np.uint8)
    ctx.ok(lib.gd_indexcov_pca8(h, X.ctypes.data))
    out.update(longest=longest, cell_off=coff, col_off=xoff, cells=cells, slots=slots, counters=counters, cn=cn, X=X, m=dims.m)
    if gram:
        G = np.zeros((N, N), np.int64)
        ctx.ok(lib.gd_indexcov_gram(h, G.ctypes.data))
        out["G"] = G
    return out


def host_cells(x):
    x = np.ascontiguousarray(x, np.float32)
    out = np.zeros(x.size, np.uint32)
    _hostlib.load().gdh_round3g(x.ctypes.data, x.size, out.ctypes.data)
    return out


def cells_numpy(x):
    """digits | (exponent + 128) << 16 from Python's exact %.2e of the float32's value."""
    out = np.zeros(len(x), np.uint32)
    for i, v in enumerate(np.asarray(x, np.float32).tolist()):
        if v != 0:
            m, e = ("%.2e" % v).split("e")
            out[i] = int(m.replace(".", "")) | ((int(e) + 128) << 16)
    return out


def random_cohort(rng, N, tiles, n_sex=1):
    """Per sample [ref0 .. ref_k] sizes with shared structure, zero runs, outliers and short samples."""
    shape = [rng.integers(2000, 60000, t) for t in tiles]
    out = []
    for s in range(N):
        scale = rng.uniform(0.3, 3)
        per = []
        for r, t in enumerate(tiles):
            v = (shape[r] * scale * rng.uniform(0.8, 1.2, t)).astype(np.int64)
            v[rng.integers(0, t, max(1, t // 50))] = 0
            if t > 20:
                a = int(rng.integers(0, t - 10)); v[a:a + 7] = 0
                v[int(rng.integers(0, t))] = int(1e12)                     # above 50 000 x the median
                v[int(rng.integers(0, t))] = int(shape[r].mean() * scale * 20)   # above MaxCN
            if s % 5 == 4 and r == len(tiles) - 2:
                v = v[:t // 2]                                             # a shorter sample
            if s % 7 == 6 and r == 0:
                v = v[:0]                                                  # a sample without this reference
            if r >= len(tiles) - n_sex:
                v = (v * (0.01 if s % 2 else 0.5)).astype(np.int64)        # a sex reference: half depth / almost nothing
            per.append(v)
        out.append(per)
    return out


@pytest.mark.parametrize("N,tiles", [(1, (300, 40)), (2, (64, 33)), (7, (1000, 129, 77)), (64, (900, 310, 65, 120)),
                                     (300, (257, 100, 31))])
def test_abi_bit_exact_against_numpy(ctx, N, tiles):
    rng = np.random.default_rng(N)
    samples = random_cohort(rng, N, tiles)
    Rn = len(tiles)
    is_sex = [0] * (Rn - 1) + [1]
    got = device(ctx, samples, is_sex)
    med = [R.median_size(s) for s in samples]
    assert got["median"].tolist() == med
    depths = [[R.normalized_depth(s, r, m) for r in range(Rn)] for s, m in zip(samples, med)]
    assert np.array_equal(got["depth"].view(np.uint32), np.concatenate([np.concatenate(d) for d in depths]).view(np.uint32))
    longest = [max(len(depths[s][r]) for s in range(N)) for r in range(Rn)]
    assert got["longest"].tolist() == longest
    M = sum(l + 1 for l in longest[:-1])
    assert got["m"] == M and M % 64 != 0
    X = np.zeros((N, M), np.uint8)
    counters = np.zeros((N, 4), np.int64)
    col = 0
    for r in range(Rn):
        cells = got["cells"][got["cell_off"][r]:got["cell_off"][r] + longest[r] * N].reshape(longest[r], N)
        for s in range(N):
            d = depths[s][r]
            assert np.array_equal(cells[:len(d), s], cells_numpy(d)) and (cells[len(d):, s] == 0).all()
            assert np.array_equal(got["slots"][r, s], R.slots_of(d))
            if not is_sex[r]:
                dp = np.minimum(d, F32(8))
                X[s, col:col + len(d)] = R.pca8_bytes(dp)
                o = (dp < F32(0.85)) | (dp > F32(1.15))
                hi = dp > F32(1.15)
                miss = longest[r] - len(d)
                counters[s] += (o.sum() + miss, (o & ~hi & (dp < F32(0.15))).sum() + miss, hi.sum(), (~o).sum())
        if is_sex[r]:
            assert got["cn"][r].tolist() == R.get_cn([depths[s][r] for s in range(N)])
        else:
            col += longest[r] + 1
    assert np.array_equal(got["counters"], counters)
    assert np.array_equal(got["X"], X)
    Xi = X.astype(np.int64)
    assert np.array_equal(got["G"], Xi @ Xi.T)


def depths_for_bytes(b):
    """float32 depths whose pca8 byte is b (0 .. 255): int(8191.875 * d + 0.5) == b."""
    d = ((b.astype(np.float64) + 0.25) / 8191.875).astype(np.float32)
    assert np.array_equal(R.pca8_bytes(d), b)
    return d


def test_gram_asymmetric_bytes_and_past_the_32_bit_bound(ctx):
    # every byte 255: 255^2 * 140 001 > 2^31 (and, biased, 127^2 * 140 001 > 2^31): a missing flush cannot pass
    N, M = 33, 140001
    samples = [[np.ones(M - 1, np.int64)] for _ in range(N)]
    X = np.full((N, M - 1), 255, np.uint8)
    got = device(ctx, samples, [0], depths=depths_for_bytes(X).ravel())
    assert got["m"] == M and np.array_equal(got["X"][:, :M - 1], X)
    assert (got["G"] == 255 * 255 * (M - 1)).all() and 255 * 255 * (M - 1) > 2 ** 32
    # asymmetric rows: row i is i + column pattern, so a transposed tile, a shifted lane map or a swapped block shows
    rng = np.random.default_rng(9)
    N, M = 70, 4099
    X = ((np.arange(N)[:, None] * 37 + np.arange(M - 1)[None, :] * (np.arange(N)[:, None] % 5 + 1)) % 256).astype(np.uint8)
    X[rng.integers(0, N, 50), rng.integers(0, M - 1, 50)] = 255
    got = device(ctx, [[np.ones(M - 1, np.int64)] for _ in range(N)], [0], depths=depths_for_bytes(X).ravel())
    Xi = X.astype(np.int64)
    assert np.array_equal(got["X"][:, :M - 1], X) and np.array_equal(got["G"], Xi @ Xi.T)


# ---- the CLI against the restatement ------------------------------------------------------------------------------------
def cli(args, timeout=600):
    r = subprocess.run([EXE, "indexcov"] + [str(a) for a in args], capture_output=True, text=True, timeout=timeout)
    return r.returncode, r.stderr


def outputs(d):
    base = os.path.join(str(d), os.path.basename(str(d)) + "-indexcov")
    raw = open(base + ".bed.gz", "rb").read()
    bed = gzip.decompress(raw)
    # valid BGZF with the EOF member, as the repository's own member walk sees it
    off, size, hdr, isize, crc = _hostlib.list_members(raw, 0, [], threads=1)
    assert int(off[-1]) + int(size[-1]) == len(raw) and isize[-1] == 0 and int(isize.sum()) == len(bed)
    return bed.decode(), open(base + ".roc").read(), open(base + ".ped").read()


def check(paths, d, extra=(), min_gap=False, **kw):
    try:
        want = R.indexcov([str(p) for p in paths], str(d), **kw)
    except R.Fatal as e:
        rc, err = cli(["-d", d] + list(extra) + list(paths))
        # a fatal of the restatement that carries a path must name that path; the others are the (FATAL) of checkSexes
        # or of a cohort without a column for the principal components
        assert rc != 0, err
        if str(e) == "(FATAL)":
            assert "(FATAL)" in err, err
        else:
            assert os.path.sep in str(e) and str(e) in err, (str(e), err)
        assert not os.path.exists(os.path.join(str(d), os.path.basename(str(d)) + "-indexcov.ped"))
        return None
    rc, err = cli(["-d", d] + list(extra) + list(paths))
    assert rc == 0, err
    bed, roc, ped = outputs(d)
    assert bed == want.bed
    assert roc == want.roc
    got_rows, got_pcs = R.strip_pcs(ped, want.n_front, want.n_pc)
    want_rows, want_pcs = R.strip_pcs(want.ped, want.n_front, want.n_pc)
    assert got_rows == want_rows
    assert ped.splitlines()[0] == want.ped.splitlines()[0]
    if min_gap:
        # the condition under which both fp64 routes print the same cells up to a %.2f tie: separated singular values
        sv = want.sv
        assert want.n_pc == 5 and all((sv[k] - sv[k + 1]) / sv[0] >= 1e-6 for k in range(5)), sv[:6]
        sign = np.sign((got_pcs * want_pcs).sum(axis=0))
        sign[sign == 0] = 1
        assert np.abs(got_pcs * sign - want_pcs).max() <= 0.01 + 1e-12, np.abs(got_pcs * sign - want_pcs).max()
    return want


@pytest.mark.parametrize("name", FIXTURES)
def test_reference_fixtures_singly(tmp_path, name):
    check([os.path.join(GOLD, name)], tmp_path / "out")


def test_reference_fixtures_together(tmp_path):
    usable = []
    for name in FIXTURES:
        try:
            R.indexcov([os.path.join(GOLD, name)], str(tmp_path / "probe"))
            usable.append(os.path.join(GOLD, name))
        except R.Fatal:
            pass
    assert usable
    check(usable, tmp_path / "out")


def test_bare_bai_with_a_fai(tmp_path):
    bam = os.path.join(GOLD, "sample_issue_27_0001.bam")
    _, refs = R.bam_header(bam)
    fai = tmp_path / "ref.fai"
    off = 6
    lines = []
    for name, ln in refs:
        lines.append("%s\t%d\t%d\t60\t61\n" % (name, ln, off))
        off += ln + ln // 60 + len(name) + 2
    fai.write_text("".join(reversed(lines)))                 # ReadFai sorts by offset, not by line
    want = check([bam + ".bai"], tmp_path / "out", extra=["-f", fai], fai=str(fai))
    assert want is not None and want.names == ["sample_issue_27_0001-bam"]


CHROMS = [str(i) for i in range(1, 23)] + ["X", "Y", "GL000201.1", "chr5_random"]


def synth_cohort(d, N, seed, n_tiles=None):
    """N .bai files over CHROMS with shared structure, zero runs, half the samples at half depth on X and near zero on
    Y, a few outlier tiles and a few samples one reference short; returns (paths, fai)."""
    rng = np.random.default_rng(seed)
    tiles = n_tiles or [int(rng.integers(110, 400)) for _ in range(22)] + [150, 60, 12, 30]
    shape = [rng.integers(20000, 90000, t).astype(np.float64) for t in tiles]
    for r in range(3):
        shape[r][50:58] = 0                                  # a centromere: repeated offsets in every sample
    groups = rng.integers(0, 3, N)
    gshape = [[sh * rng.uniform(0.7, 1.3, len(sh)) for sh in shape] for _ in range(3)]
    os.makedirs(str(d), exist_ok=True)
    paths = []
    for s in range(N):
        scale = rng.uniform(0.5, 2.0)
        refs = []
        at = 1 << 20
        for r, t in enumerate(tiles):
            v = gshape[groups[s]][r] * scale * rng.uniform(0.9, 1.1, t)
            if CHROMS[r] == "X" and s % 2:
                v = v * 0.5
            if CHROMS[r] == "Y" and not s % 2:
                v = v * rng.choice([0.001, 0.01, 0.0], t, p=[0.5, 0.2, 0.3])
            v = v.astype(np.int64)
            if s % 9 == 0 and r == 4:
                v[7] = 10 ** 13                              # above 50 000 x the median
            if s % 11 == 3 and r == 21:
                v = v[:0]                                    # a sample one reference short
            if s % 13 == 5 and r == 6:
                v = v[:len(v) // 3]
            iv = np.concatenate([[at], at + np.cumsum(v)]).astype(np.uint64) if len(v) else np.zeros(0, np.uint64)
            at = int(iv[-1]) + 4096 if len(iv) else at
            refs.append((iv, (int(1000 + s + r), int(s)) if s % 4 else None))
        p = os.path.join(str(d), "s%03d.bai" % s)
        R.write_bai(p, refs)
        paths.append(p)
    fai = os.path.join(str(d), "ref.fai")
    with open(fai, "w") as f:
        off = 10
        for c, t in zip(CHROMS, tiles):
            f.write("%s\t%d\t%d\t60\t61\n" % (c, t * 16384, off))
            off += t * 16384 + 100
    return paths, fai


@pytest.fixture(scope="module")
def cohort(tmp_path_factory):
    return synth_cohort(tmp_path_factory.mktemp("cohort"), 64, 2024)


def test_cohort_of_64(cohort, tmp_path):
    paths, fai = cohort
    want = check(paths, tmp_path / "out", extra=["-f", fai], fai=fai, min_gap=True)
    assert "chr5_random" not in want.bed and "GL000201.1\t" in want.bed and "5e+04" in want.bed


def test_cohort_extra_normalize(cohort, tmp_path):
    paths, fai = cohort
    check(paths, tmp_path / "out", extra=["-n", "-f", fai], fai=fai, extra_normalize=True, min_gap=True)


def test_cohort_sex_and_exclude_variants(cohort, tmp_path):
    paths, fai = cohort
    check(paths, tmp_path / "a", extra=["-X", "", "-f", fai], fai=fai, sex="", min_gap=True)
    check(paths, tmp_path / "b", extra=["-X", "chrX,chrY", "-f", fai], fai=fai, sex="chrX,chrY", min_gap=True)
    want = check(paths, tmp_path / "c", extra=["-p", "", "-f", fai], fai=fai, exclude="", min_gap=True)
    assert "chr5_random\t" in want.bed
    check(paths[:20], tmp_path / "d", extra=["-e", "-f", fai], fai=fai, include_gl=True, min_gap=True)


@pytest.mark.parametrize("n", [1, 2, 4, 5, 7])
def test_small_cohorts(cohort, tmp_path, n):
    paths, fai = cohort
    want = check(paths[:n], tmp_path / "out", extra=["-n", "-f", fai], fai=fai, extra_normalize=True, min_gap=n >= 7)
    assert (want.n_pc == 0) == (n < 3)
    check(paths[:n], tmp_path / "out2", extra=["-f", fai], fai=fai, min_gap=n >= 7)


# ---- errors -------------------------------------------------------------------------------------------------------------
def pe(pos):
    return CR.Rec(0, pos, 0x3, pos + 300, 500, ((0, 100),))


def failing(tmp_path, args, named):
    d = tmp_path / "out"
    rc, err = cli(["-d", d] + args)
    assert rc != 0 and named in err, err
    assert not os.path.exists(os.path.join(str(d), "out-indexcov.ped"))


def test_errors_name_the_argument_and_leave_no_ped(tmp_path, cohort):
    paths, fai = cohort
    refs = [("c1", 1 << 20)]
    good = str(tmp_path / "good.bam")
    CR.write_bam(good, refs, [pe(100 * i) for i in range(3000)], block=4096)
    noidx = str(tmp_path / "noidx.bam")
    CR.write_bam(noidx, refs, [pe(100 * i) for i in range(10)], index=False)
    failing(tmp_path, [good, noidx], "noidx.bam")
    failing(tmp_path, [good, str(tmp_path / "x.crai")], "x.crai")
    failing(tmp_path, ["-c", "c1", good], "-c")
    two = str(tmp_path / "two.bam")
    CR.write_bam(two, refs, [pe(100 * i) for i in range(3000)], block=4096,
                 header_text="@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:c1\tLN:1048576\n@RG\tID:a\tSM:x\n@RG\tID:b\tSM:y\n")
    failing(tmp_path, [two], "two.bam")
    failing(tmp_path, [paths[0]], "s000.bai")                # a .bai without -f
    bad = str(tmp_path / "dec.bai")
    R.write_bai(bad, [(np.array([1 << 20, 3 << 20, 2 << 20, 4 << 20], np.uint64), None)])
    failing(tmp_path, ["-f", fai, bad], "dec.bai")


def test_python_entry_writes_the_same_files(cohort, tmp_path):
    from goleft_amd import indexcov
    paths, fai = cohort
    assert cli(["-d", tmp_path / "a", "-f", fai] + paths[:9])[0] == 0
    assert indexcov.Main(["-d", str(tmp_path / "b"), "-f", fai] + paths[:9]) == 0
    for x, y in zip(outputs(tmp_path / "a"), outputs(tmp_path / "b")):
        assert x == y
