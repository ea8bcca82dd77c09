"""CPU: the pieces of `indexcov` that need no device -- the host instance of the %.3g digit function against Python's own
exact formatting, the restatement (tests/indexcov_ref.py) against hand-computed values of a toy cohort, the Gram route
to the principal components against numpy's SVD, and the new ABI symbols."""
import ctypes as C
import os

import numpy as np
import pytest

from goleft_amd import _hostlib, _lib
from tests import indexcov_ref as R
from tests.indexcov_shapes import notation_edges, tie_neighbourhood, tiny_quotients


def digits(x):
    x = np.ascontiguousarray(x, np.float32)
    out = np.zeros(x.size, np.uint32)
    _hostlib.load().gdh_round3g(x.ctypes.data, x.size, out.ctypes.data)
    return out


def text(cell):
    buf = C.create_string_buffer(16)
    n = _hostlib.load().gdh_fmt3g(int(cell), buf, 16)
    assert n > 0
    return buf.value.decode()


def want_cell(x):
    """(digits, exponent) of the exact value of the float32 x rounded half-even to three significant digits."""
    if x == 0:
        return 0, 0
    m, e = ("%.2e" % float(x)).split("e")
    return int(m.replace(".", "")), int(e)


def check(values):
    v = np.ascontiguousarray(values, np.float32)
    got = digits(v)
    for x, c in zip(v.tolist(), got.tolist()):
        d, e = want_cell(np.float32(x))
        assert (c & 0xffff, (c >> 16) - 128 if d else 0) == (d, e), (x, hex(c))
        assert text(c) == "%.3g" % float(np.float32(x)), x


def test_round3g_ties_and_their_neighbours():
    v = tie_neighbourhood()
    assert len(v) > 27000
    exact = [x for x in v.tolist() if "%.3g" % x != "%.3g" % float(np.nextafter(np.float32(x), np.float32(np.inf)))]
    assert exact                                             # the grid does cross rounding boundaries
    check(v)


def test_round3g_notation_boundaries_and_small_quotients():
    check(notation_edges())
    tiny = tiny_quotients()
    assert sum(0 < float(x) < 1.17549435e-38 for x in tiny) >= 2 and 0.0 in [float(x) for x in tiny]
    check(tiny)
    assert text(digits([50000])[0]) == "5e+04" and text(digits([0.0001])[0]) == "0.0001" and text(digits([1000])[0]) == "1e+03"


def test_round3g_random_values():
    rng = np.random.default_rng(27)
    v = np.concatenate([
        np.exp(rng.uniform(np.log(1e-5), np.log(5e4), 700000)),
        rng.uniform(0, 3, 200000),
        np.exp(rng.uniform(np.log(1e-44), np.log(1e-5), 100000)),
    ]).astype(np.float32)
    got = digits(v)
    strs = np.char.mod("%.2e", v.astype(np.float64))
    d = np.array([int(s[0] + s[2:4]) for s in strs])
    e = np.array([int(s[5:]) for s in strs])
    nz = v != 0
    assert np.array_equal((got & 0xffff)[nz], d[nz]) and np.array_equal(((got >> 16).astype(np.int64) - 128)[nz], e[nz])
    assert (got[~nz] == 0).all()
    for x, c in zip(v[:20000].tolist(), got[:20000].tolist()):
        assert text(c) == "%.3g" % x


# ---- the restatement on a toy cohort, by hand -----------------------------------------------------------------------------
def intervals(sizes, start=1 << 16):
    return np.concatenate([[start], start + np.cumsum(sizes)]).astype(np.uint64)


@pytest.fixture()
def toy(tmp_path):
    a0 = [100] * 40 + [0] * 5 + [100] * 53 + [200, 1000000]        # 100 tiles: a run of repeated offsets, two outliers
    ax = [1, 1, 1, 1, 100, 100, 100, 200, 200, 0]                   # 4 of 10 tiles below 0.02: more than 30 %
    b0, bx = [50] * 60, [50] * 10                                   # shorter than the longest
    c0, cx = [300] * 99 + [600], [150] * 10
    paths = []
    for name, s0, sx, st in (("A", a0, ax, (10, 1)), ("B", b0, bx, (20, 2)), ("C", c0, cx, None)):
        p = str(tmp_path / (name + ".bai"))
        R.write_bai(p, [(intervals(s0), st), (intervals(sx, 1 << 40), st)])
        paths.append(p)
    fai = tmp_path / "ref.fai"
    fai.write_text("X\t163840\t2000000\t60\t61\nchr1\t1638400\t6\t60\t61\n")      # ReadFai sorts by offset: chr1 first
    return paths, str(fai), tmp_path


def test_restatement_on_a_toy_cohort(toy):
    paths, fai, tmp = toy
    sizes = [R.read_bai(p)[0] for p in paths]
    # the 98 % cap bites for A: without it the cumulative sum would pass total / 2 only at the 1 000 000 tile
    assert [R.median_size(s) for s in sizes] == [100, 50, 300]
    dA = R.normalized_depth(sizes[0], 0, 100)
    assert dA[99] == 10000 and dA[98] == 2 and (dA[40:45] == 0).all() and len(dA) == 100
    assert R.get_cn([R.normalized_depth(s, 1, m) for s, m in zip(sizes, (100, 50, 300))]) == [2.0, 2.0, 1.0]
    res = R.indexcov(paths, str(tmp / "out"), fai=fai)
    bed = res.bed.splitlines()
    assert bed[0] == "#chrom\tstart\tend\tA\tB\tC" and len(bed) == 1 + 100 + 10
    assert bed[1] == "chr1\t0\t16384\t1\t1\t1" and bed[41] == "chr1\t655360\t671744\t0\t1\t1"
    assert bed[61] == "chr1\t983040\t999424\t1\t0\t1"                # B has 60 tiles
    assert bed[100] == "chr1\t1622016\t1638400\t1e+04\t0\t2"
    assert bed[101] == "X\t0\t16384\t0.01\t1\t0.5"
    assert res.pca8.shape == (3, 101) and res.pca8[0, 99] == 255 and res.pca8[1, 60:].sum() == 0
    ped = [ln.split("\t") for ln in res.ped.splitlines()]
    assert ped[0][6:13] == ["CNX", "bins.out", "bins.lo", "bins.hi", "bins.in", "slope", "p.out"]
    assert ped[0][13:] == ["PC1", "PC2", "PC3", "mapped", "unmapped"]
    assert ped[1][:12] == ["unknown", "A", "-9", "-9", "2", "-9", "2.00", "7", "5", "2", "93", "NaN"]
    assert ped[2][:11] == ["unknown", "B", "-9", "-9", "2", "-9", "2.00", "40", "40", "0", "60"] and ped[2][12] == "0.67"
    assert ped[3][:11] == ["unknown", "C", "-9", "-9", "1", "-9", "1.00", "1", "0", "1", "99"]
    assert ped[1][-2:] == ["20", "2"] and ped[3][-2:] == ["0", "0"]
    assert ped[1][15] == "0.00"                                      # the third of three components has no variance
    roc = res.roc.splitlines()
    assert len(roc) == 2 * 71 and roc[1].split("\t")[:2] == ["chr1", "0.00"] and roc[1].split("\t")[2:] == ["1.00"] * 3


def test_gram_route_matches_the_svd():
    rng = np.random.default_rng(5)
    lib = _hostlib.load()
    for n, m in ((7, 300), (12, 5000), (40, 20000)):
        base = rng.integers(0, 256, (3, m))
        X = np.clip(base[rng.integers(0, 3, n)] + rng.integers(-40, 40, (n, m)), 0, 255).astype(np.uint8)
        G = X.astype(np.int64) @ X.astype(np.int64).T
        want, sv = R.principal_components(X)
        got = np.zeros((n, 5))
        sg = np.zeros(5)
        assert lib.gdh_indexcov_pcs(G.ctypes.data, n, 5, got.ctypes.data, sg.ctypes.data) == 0
        assert np.allclose(sg, sv[:5], rtol=1e-9, atol=1e-6)
        sign = np.sign((got * want).sum(axis=0))
        print(n, m, np.abs(got * sign - want).max(), np.abs(want).max())
        assert np.abs(got * sign - want).max() <= 1e-6


def test_abi_symbols_resolve():
    lib = _lib.load()
    for name in _lib.SYMBOLS:
        if name.startswith("gd_indexcov_"):
            assert getattr(lib, name)
    assert sum(n.startswith("gd_indexcov_") for n in _lib.SYMBOLS) == 13
    # the entry points were only added: the version stays, the revision counts the addition, and both are the header's
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(_lib.SO_PATH)), "include", "goleft_depth.h")).read()
    assert lib.gd_abi_version() == int(re.search(r"#define\s+GD_ABI_VERSION\s+(\d+)", hdr).group(1))
    assert lib.gd_abi_revision() == int(re.search(r"#define\s+GD_ABI_REVISION\s+(\d+)", hdr).group(1)) >= 1
    host = _hostlib.load()
    for name in ("gdh_indexcov_main", "gdh_indexcov_run", "gdh_round3g", "gdh_fmt3g", "gdh_indexcov_pcs"):
        assert getattr(host, name)
    assert os.path.exists(os.path.join(os.path.dirname(_lib.SO_PATH), "indexcov.py"))
