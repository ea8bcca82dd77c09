"""GPU: indexcov's device kernels through the ABI on the crafted inputs of tests/indexcov_shapes.py -- the two selects of
the median kernel (duplicates across the rank, a cumulative sum equal to total / 2, total == 0, a median of 0, sizes
past 2^53), the 50 000 cap, GetCN's select at the 0.3 share and at float32(0.02), the device instance of gd_round3g at
every three-digit tie, every float32 next to a slot, pca8 or counter threshold, a second compute on one upload, and
the Gram kernel across its 16 384-column flush.  Everything is compared as integers or bit patterns with the
restatement (tests/indexcov_ref.py); tests/test_indexcov_shapes.py shows that the inputs reach these edges."""
import ctypes as C

import numpy as np
import pytest

from goleft_amd import _lib
from tests import indexcov_ref as R
from tests import indexcov_shapes as S
from tests.test_gpu_indexcov import Ctx, cells_numpy, depths_for_bytes, device, host_cells, random_cohort

pytestmark = pytest.mark.gpu

F32 = np.float32


@pytest.fixture(scope="module")
def ctx():
    c = Ctx()
    yield c
    c.close()


def results(ctx, N, Rn, gram=True):
    """Everything gd_indexcov_compute left behind, read back as device() of tests/test_gpu_indexcov.py does."""
    lib, h = ctx.lib, ctx.h
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
    out = dict(longest=longest, cell_off=coff, col_off=xoff, cells=cells, slots=slots, counters=counters, cn=cn, X=X, m=dims.m,
               m_pad=dims.m_pad)
    if gram:
        out["G"] = np.zeros((N, N), np.int64)
        ctx.ok(lib.gd_indexcov_gram(h, out["G"].ctypes.data))
    return out


def restated(depths, is_sex):
    """What compute must leave for depths[sample][reference] (float32 arrays): the expressions of
    test_abi_bit_exact_against_numpy, gathered.  The copy number of a reference that is no sex reference, or that no
    sample has a tile on, is the 0 the buffer was cleared to."""
    N, Rn = len(depths), len(is_sex)
    longest = [max(len(depths[s][r]) for s in range(N)) for r in range(Rn)]
    M = sum(l + 1 for l, x in zip(longest, is_sex) if not x)
    X, counters = np.zeros((N, M), np.uint8), np.zeros((N, 4), np.int64)
    slots, cn, cells = np.zeros((Rn, N, 70), np.int64), np.zeros((Rn, N)), []
    col = 0
    for r in range(Rn):
        c = np.zeros((longest[r], N), np.uint32)
        for s in range(N):
            d = depths[s][r]
            c[:len(d), s] = cells_numpy(d)
            slots[r, s] = R.slots_of(d)
            if not is_sex[r]:
                dp = np.minimum(d, F32(8))
                X[s, col:col + len(d)] = R.pca8_bytes(dp)
                o = (dp < F32(0.85)) | (dp > F32(1.15))
                hi = dp > F32(1.15)
                miss = longest[r] - len(d)
                counters[s] += (o.sum() + miss, (o & ~hi & (dp < F32(0.15))).sum() + miss, hi.sum(), (~o).sum())
        cells.append(c)
        if is_sex[r]:
            if longest[r] > 0:
                cn[r] = R.get_cn([depths[s][r] for s in range(N)])
        else:
            col += longest[r] + 1
    Xi = X.astype(np.int64)
    return dict(longest=longest, m=M, cells=cells, slots=slots, counters=counters, cn=cn, X=X, G=Xi @ Xi.T)


def same(got, want, gram=True):
    N = want["X"].shape[0]
    assert got["longest"].tolist() == want["longest"] and got["m"] == want["m"]
    for r, c in enumerate(want["cells"]):
        at = int(got["cell_off"][r])
        assert np.array_equal(got["cells"][at:at + c.size].reshape(c.shape), c), r
    assert got["cells"].size == sum(c.size for c in want["cells"])
    assert np.array_equal(got["slots"], want["slots"])
    assert np.array_equal(got["counters"], want["counters"])
    assert np.array_equal(got["X"], want["X"])
    assert got["cn"].tolist() == want["cn"].tolist()                 # float64 ==, element by element
    if gram:
        assert np.array_equal(got["G"], want["G"])
    assert got["X"].shape[0] == N


def split(flat, samples):
    """The flat depths of a cohort as depths[sample][reference]."""
    out, at = [], 0
    for s in samples:
        per = []
        for v in s:
            per.append(np.asarray(flat[at:at + len(v)], F32))
            at += len(v)
        out.append(per)
    assert at == len(flat)
    return out


# ---- the median kernel and the depths ---------------------------------------------------------------------------------------
def test_median_and_depth_edges(ctx):
    shapes = S.median_shapes()
    names = [name for name, _ in shapes]
    samples = [np.array_split(v, 3) for _, v in shapes]              # two autosomes and a sex reference per sample
    is_sex = [0, 0, 1]
    got = device(ctx, samples, is_sex)
    med = [R.median_size(s) for s in samples]
    wrong = [(n, g, w) for n, g, w in zip(names, got["median"].tolist(), med) if g != w]
    assert not wrong, wrong[:10]
    # the depths lie parallel to the sizes; a sample whose median is 0 has none in the reference and zeros on the device
    depths = [[R.normalized_depth(s, r, m) for r in range(3)] for s, m in zip(samples, med)]
    flat = np.concatenate([np.concatenate(d) if m else np.zeros(sum(len(v) for v in s), F32)
                           for d, s, m in zip(depths, samples, med)])
    assert np.array_equal(got["depth"].view(np.uint32), flat.view(np.uint32))
    cap = [i for i, n in enumerate(names) if n.startswith("cap-")]
    assert len(cap) == 3 and all((np.concatenate(depths[i]) == 50000).sum() >= 3 for i in cap)
    want = restated(depths, is_sex)
    same(got, want)
    # a sample whose median is 0: no tile anywhere, whatever its tile counts were
    zero = [i for i, m in enumerate(med) if m == 0]
    assert len(zero) >= 4
    longest = want["longest"]
    assert max(len(samples[i][0]) for i in zero) > max(longest)      # the sample with the most tiles does not set `longest`
    for i in zero:
        for r in range(3):
            at = int(got["cell_off"][r])
            assert (got["cells"][at:at + longest[r] * len(samples)].reshape(longest[r], -1)[:, i] == 0).all()
        assert got["counters"][i].tolist() == [longest[0] + longest[1], longest[0] + longest[1], 0, 0]
        assert (got["X"][i] == 0).all() and (got["slots"][:, i] == 0).all()
        assert got["cn"][2, i] == -0.1
        assert (got["G"][i] == 0).all() and (got["G"][:, i] == 0).all()


# ---- GetCN ------------------------------------------------------------------------------------------------------------------
def test_cn_selection_edges(ctx):
    shapes = S.cn_shapes()
    names = [name for name, _ in shapes]
    samples = [[np.ones(1, np.int64), np.ones(len(d), np.int64)] for _, d in shapes]     # every median is 1
    depths = [[np.ones(1, F32), d] for _, d in shapes]
    got = device(ctx, samples, [0, 1], depths=np.concatenate([np.concatenate(d) for d in depths]))
    assert (got["median"] == 1).all()
    want = R.get_cn([d for _, d in shapes])
    wrong = [(n, g, w) for n, g, w in zip(names, got["cn"][1].tolist(), want) if g != w]
    assert not wrong, wrong[:10]
    assert min(len(d) for _, d in shapes) == 0 and got["longest"][1] == max(len(d) for _, d in shapes)
    same(got, restated(depths, [0, 1]))


# ---- gd_round3g on the device -----------------------------------------------------------------------------------------------
def test_device_cells_at_three_digit_ties(ctx):
    v = S.cell_values()
    got = device(ctx, [[np.ones(len(v), np.int64)]], [0], depths=v, gram=False)
    assert got["longest"].tolist() == [len(v)] and got["cells"].size == len(v)
    want = cells_numpy(v)
    wrong = np.flatnonzero(got["cells"] != want)
    assert wrong.size == 0, [(float(v[i]), hex(got["cells"][i]), hex(want[i])) for i in wrong[:10]]
    assert np.array_equal(got["cells"], host_cells(v))               # the two instances of the one text


# ---- slots, bytes and counters at their thresholds --------------------------------------------------------------------------
def test_slot_byte_and_counter_thresholds(ctx):
    # (three depths well above MaxCN behind the thresholds: there the cell of d and the cell of min(d, 8) differ)
    v = np.concatenate([S.threshold_depths(), np.array([9.5, 123.5, 50000], F32)])
    got = device(ctx, [[np.ones(len(v), np.int64)]], [0], depths=v, gram=False)
    assert np.array_equal(got["slots"][0, 0], R.slots_of(v)) and got["slots"].sum() == len(v)
    dp = np.minimum(v, F32(8))
    X = R.pca8_bytes(dp)
    wrong = np.flatnonzero(got["X"][0, :len(v)] != X)
    assert wrong.size == 0, [(float(v[i]), int(got["X"][0, i]), int(X[i])) for i in wrong[:10]]
    assert got["m"] == len(v) + 1 and got["X"][0, len(v)] == 0
    o = (dp < F32(0.85)) | (dp > F32(1.15))
    hi = dp > F32(1.15)
    assert got["counters"][0].tolist() == [o.sum(), (o & ~hi & (dp < F32(0.15))).sum(), hi.sum(), (~o).sum()]
    # the cells are made from the depth itself, not from min(d, 8)
    assert np.array_equal(got["cells"], cells_numpy(v)) and (v > 8).sum() >= 6
    assert (cells_numpy(v[-3:]) != cells_numpy(dp[-3:])).all()


# ---- a second compute on one upload -----------------------------------------------------------------------------------------
def test_recompute_does_not_accumulate(ctx):
    rng = np.random.default_rng(77)
    N, tiles, is_sex = 7, (1000, 129, 77), [0, 0, 1]
    samples = random_cohort(rng, N, tiles)
    first = device(ctx, samples, is_sex)
    same(first, restated(split(first["depth"], samples), is_sex))
    assert first["counters"].sum() > 0 and (first["cn"][2] > 0).all()
    ctx.ok(ctx.lib.gd_indexcov_compute(ctx.h, 1))
    again = results(ctx, N, 3)
    for k in ("longest", "cells", "slots", "counters", "cn", "X", "G"):
        assert np.array_equal(first[k], again[k]), k
    # other depths on the same upload: fewer tiles inside the band, zeros where bytes stood, lows on the sex reference
    d2 = rng.uniform(0, 3, first["depth"].size).astype(F32)
    d2[rng.integers(0, d2.size, d2.size // 3)] = 0
    d2[rng.integers(0, d2.size, d2.size // 10)] = F32(0.01)
    ctx.ok(ctx.lib.gd_indexcov_set_depths(ctx.h, d2.ctypes.data, d2.size))
    ctx.ok(ctx.lib.gd_indexcov_compute(ctx.h, 1))
    third = results(ctx, N, 3)
    want = restated(split(d2, samples), is_sex)
    same(third, want)
    assert not np.array_equal(third["counters"], first["counters"]) and not np.array_equal(third["cn"], first["cn"])
    assert ((third["X"] == 0) & (first["X"] != 0)).sum() > 100       # bytes of the first depths that had to go


# ---- the Gram kernel across its flush ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("longest", [16319, 16383, 16384, 16447])
@pytest.mark.parametrize("N", [32, 33, 65])
def test_gram_asymmetric_across_the_flush_boundary(ctx, N, longest):
    # m = longest + 1 columns (the last one the zero behind the tiles), padded to 64: 16 320 is one chunk of 255 steps,
    # not a multiple of the four waves; 16 384 one chunk exactly; 16 448 a second chunk of one step -- of padding alone
    # for longest = 16 384, of 63 bytes of the pattern for 16 447
    rng = np.random.default_rng(N * 100000 + longest)
    X = ((np.arange(N)[:, None] * 37 + np.arange(longest)[None, :] * (np.arange(N)[:, None] % 5 + 1)) % 256).astype(np.uint8)
    X[rng.integers(0, N, 50), rng.integers(0, longest, 50)] = 255
    X[:, -1] = 255 - np.arange(N)                                    # the last column before the padding is not 0
    device(ctx, [[np.ones(longest, np.int64)] for _ in range(N)], [0], depths=depths_for_bytes(X).ravel())
    got = results(ctx, N, 1)
    assert got["m"] == longest + 1 and got["m_pad"] == {16319: 16320, 16383: 16384, 16384: 16448, 16447: 16448}[longest]
    Xi = X.astype(np.int64)
    assert np.array_equal(got["X"][:, :longest], X) and (got["X"][:, longest] == 0).all()
    assert np.array_equal(got["G"], Xi @ Xi.T)
