"""-m gpu: gd_depth_hist and gd_region_bins through DepthEngine against the numpy restatement
(tests/depth_hist_ref.py) applied to the CPU oracle's per-base vectors: exact equality everywhere.

One module-scoped context, computed once, three contigs.  Contig A: 2^20 positions without a read (every lane of every wave
on bin 0: the whole-wave add), then 2^18 positions that alternate 1 / 0 (one-base reads: no two neighbours merge), then a
plateau of 3 to an end that is no multiple of 4.  Contig B (150 001) is H.random_reads merged with H.edge_reads.  Contig C
is a staircase: 70 000 one-op reads start at S + i and all end at E, so every depth 1 .. 70 000 occurs exactly once and
then a plateau of 70 000 follows over two chunks and three positions: one position on each side of the edge of the LDS
range (bins below 8192 are counted in LDS, the others in the global table), of every n_bins - 1 used, and of 65535.  A
position outside its region counted as depth 0 shows in every region that does not start and end on a chunk's edge."""
import ctypes as C

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import depth_hist_ref as D
from tests import helpers as H
from tests.test_gpu_perbase_runs import CUTS32, merged

pytestmark = pytest.mark.gpu

ZERO, ALT, FLAT = 1 << 20, 1 << 18, 10_003
LA, LB = ZERO + ALT + FLAT, 150_001
S, STEPS = 4_099, 70_000
E = S + STEPS + 2 * 4096 + 3
LC = E + 1_706
LENS = (LA, LB, LC)
LDS_BINS = 8192
N_BINS = [1, 2, 3, 64, LDS_BINS - 1, LDS_BINS, LDS_BINS + 1, 65535, 65536]
CUT_LISTS = [None, [1], [1, 4, 100], [8191, 8192, 70000], CUTS32]
SPANS = (0, 1, 4, 16, 4096, 3 * 4096 + 16)
E_INVALID, E_STATE, E_RANGE = -1, -4, -5


def one_op_reads(pos, span):
    n = len(pos)
    assert (np.diff(pos) >= 0).all()
    return po.Reads(np.asarray(pos, np.int32), np.zeros(n, np.uint16), np.full(n, 60, np.uint8), np.arange(n + 1, dtype=np.uint32),
                    (np.asarray(span, np.uint32) << 4))                  # one M op per record


def reads_a():
    pos = np.concatenate([np.arange(ZERO, ZERO + ALT, 2, dtype=np.int64), np.full(3, ZERO + ALT, np.int64)])
    span = np.concatenate([np.ones(ALT // 2, np.int64), np.full(3, FLAT, np.int64)])
    return one_op_reads(pos, span)


def reads_c():
    pos = S + np.arange(STEPS, dtype=np.int64)
    return one_op_reads(pos, E - pos)


@pytest.fixture(scope="module")
def world():
    """(engine, [oracle vector of A, B, C]): computed once, unchanged by the tests."""
    from goleft_amd.engine import DepthEngine
    rng = np.random.default_rng(322)
    reads = [reads_a(), merged(H.random_reads(rng, LB, 9_000), H.edge_reads(rng, LB, 4_000)), reads_c()]
    eng = DepthEngine(0)
    eng.set_params()
    eng.set_contigs(list(LENS))
    for tid, r in enumerate(reads):
        eng.push(tid, r.pos, r.flag, r.mapq, r.cigar_off, r.cigar)
    eng.compute()
    depth = [po.perbase_c(r, 1, 0, L, diff=(tid == 2)) for tid, (r, L) in enumerate(zip(reads, LENS))]
    yield eng, depth
    eng.close()


@pytest.fixture(scope="module")
def region_lists():
    """The lists both entries are run on: every alignment of both ends at several bases; duplicates, overlaps, empties and
    all contigs in one list; random short regions with one whole contig among them."""
    aligned = []
    for tid, base in ((0, ZERO - 8192 - 8), (0, ZERO + ALT - 4100), (1, 70_000), (2, S + LDS_BINS - 4100), (2, E - 3 * 4096 - 40)):
        for ds in range(4):
            for de in range(4):
                aligned += [(tid, base + ds, base + span + de) for span in SPANS if ds <= span + de]
    mixed = [(1, 100, 9000), (1, 100, 9000), (0, ZERO - 50, ZERO + 50), (1, 5000, 5000), (2, S - 10, S + 9000), (1, 4000, 12_000),
             (2, 0, 0), (0, LA - 5, LA), (2, LC, LC), (1, 0, LB), (2, S + 8000, E + 100), (0, 0, 1), (1, 100, 9000)]
    rng = np.random.default_rng(7)
    tid = rng.integers(0, 3, size=5000)
    length = rng.integers(1, 301, size=5000)
    start = (rng.random(5000) * (np.array(LENS)[tid] - length)).astype(np.int64)
    rand = [(int(t), int(s), int(s + n)) for t, s, n in zip(tid, start, length)]
    rand.insert(2500, (1, 0, LB))
    return {"aligned": aligned, "mixed": mixed, "random": rand}


def same_hist(eng, depth, regions, n_bins):
    want = D.hist(depth, regions, n_bins)
    t, s, e = ([r[k] for r in regions] for k in range(3))
    got = eng.depth_hist(t, s, e, n_bins)
    assert got[0].dtype == np.uint64 and got[0].shape == (n_bins,)
    bad = np.flatnonzero(got[0] != want[0])
    assert bad.size == 0, (len(regions), regions[:3], n_bins, int(bad[0]), int(got[0][bad[0]]), int(want[0][bad[0]]))
    assert got[1:] == want[1:], (len(regions), regions[:3], n_bins, got[1:], want[1:])
    return want


def same_bins(eng, depth, regions, cuts):
    want = np.stack([D.bins(depth[t], s, e, cuts) for t, s, e in regions])
    t, s, e = ([r[k] for r in regions] for k in range(3))
    got = eng.region_bins(t, s, e, cuts)
    assert got.dtype == np.uint64 and got.shape == want.shape
    bad = np.argwhere(got != want)
    assert bad.size == 0, (cuts, regions[int(bad[0][0])], got[int(bad[0][0])].tolist(), want[int(bad[0][0])].tolist())
    assert (got.sum(axis=1) == np.array(e) - np.array(s)).all()


def test_the_designed_profiles_are_what_the_oracle_sees(world):
    _, depth = world
    a, c = depth[0], depth[2]
    assert not a[:ZERO].any() and np.array_equal(a[ZERO:ZERO + ALT], np.tile(np.array([1, 0], np.int32), ALT // 2))
    assert (a[ZERO + ALT:] == 3).all() and LA % 4 == 3
    assert not c[:S].any() and np.array_equal(c[S:S + STEPS], np.arange(1, STEPS + 1)) and (c[S + STEPS:E] == STEPS).all() and not c[E:].any()
    assert len(np.unique(depth[1])) > 8


@pytest.mark.parametrize("n_bins", N_BINS)
def test_whole_contigs(world, n_bins):
    eng, depth = world
    for tid, L in enumerate(LENS):
        bins, total, lo, hi = same_hist(eng, depth, [(tid, 0, L)], n_bins)
        assert int(bins.sum()) == L
    same_hist(eng, depth, [(2, S, E)], n_bins)                             # the staircase alone: no position at depth 0
    same_hist(eng, depth, [(0, 0, LA), (1, 0, LB), (2, 0, LC)], n_bins)
    t = eng.dist_timing()
    assert set(t) == {"upload_s", "kernel_s", "readback_s"} and all(v > 0 for v in t.values())


def test_a_single_region_as_scalars(world):
    eng, depth = world
    got = eng.depth_hist(1, 10, 5000, 16)
    want = D.hist(depth, [(1, 10, 5000)], 16)
    assert np.array_equal(got[0], want[0]) and got[1:] == want[1:]
    assert np.array_equal(eng.region_bins(1, 10, 5000, [1, 4])[0], D.bins(depth[1], 10, 5000, [1, 4]))


def test_heads_and_tails_of_every_alignment(world, region_lists):
    """start and end over all residues mod 4 (the element loads next to the 16-byte loads), spans from 0 to three chunks:
    each region alone, then all of them in one call."""
    eng, depth = world
    for r in region_lists["aligned"]:
        same_hist(eng, depth, [r], 65536 if r[0] == 2 else 64)
    for n_bins in (64, LDS_BINS, 65536):
        same_hist(eng, depth, region_lists["aligned"], n_bins)


@pytest.mark.parametrize("n_bins", N_BINS)
def test_region_lists(world, region_lists, n_bins):
    eng, depth = world
    same_hist(eng, depth, region_lists["mixed"], n_bins)
    same_hist(eng, depth, region_lists["random"], n_bins)
    same_hist(eng, depth, region_lists["mixed"][::-1], n_bins)


def test_no_region_and_no_position(world):
    eng, depth = world
    for regions in ([], [(1, 77, 77)], [(0, LA, LA), (2, 0, 0)]):
        t, s, e = ([r[k] for r in regions] for k in range(3))
        bins, total, lo, hi = eng.depth_hist(np.array(t, np.int32), np.array(s, np.int64), np.array(e, np.int64), 100)
        assert not bins.any() and (total, lo, hi) == (0, 0, 0)
        got = eng.region_bins(np.array(t, np.int32), np.array(s, np.int64), np.array(e, np.int64), [1, 2])
        assert got.shape == (len(regions), 3) and not got.any()


def test_a_second_call_starts_from_zero(world):
    """A smaller table and a smaller region the second time: what the first call left would show."""
    eng, depth = world
    same_hist(eng, depth, [(2, 0, LC), (1, 0, LB)], 65536)
    same_hist(eng, depth, [(1, 40_000, 40_100)], 8)
    same_hist(eng, depth, [(2, S + 100, S + 110)], 70)
    same_bins(eng, depth, [(2, 0, LC), (1, 0, LB)], CUTS32)
    same_bins(eng, depth, [(1, 40_000, 40_100)], [2])


def _raw_hist(eng, regions, n_bins, stats=True, cap=None):
    """The C call itself: (rc, bins, sum, min, max), sentinels where nothing was written."""
    t = np.array([r[0] for r in regions], np.int32)
    s = np.array([r[1] for r in regions], np.int64)
    e = np.array([r[2] for r in regions], np.int64)
    bins = np.full(max(cap if cap is not None else n_bins, 1), 0xDEADBEEF, np.uint64)
    tot, lo, hi = C.c_int64(-7), C.c_int32(-8), C.c_int32(-9)
    rc = eng._lib.gd_depth_hist(eng._ctx, len(regions), t.ctypes.data, s.ctypes.data, e.ctypes.data, n_bins, bins.ctypes.data,
                                C.byref(tot) if stats else None, C.byref(lo) if stats else None, C.byref(hi) if stats else None)
    return rc, bins, tot.value, lo.value, hi.value


def _raw_bins(eng, regions, cuts):
    t = np.array([r[0] for r in regions], np.int32)
    s = np.array([r[1] for r in regions], np.int64)
    e = np.array([r[2] for r in regions], np.int64)
    c = np.ascontiguousarray(cuts, np.int32)
    out = np.full((len(regions), 34), 0xDEADBEEF, np.uint64)
    rc = eng._lib.gd_region_bins(eng._ctx, len(regions), t.ctypes.data, s.ctypes.data, e.ctypes.data, c.size,
                                 c.ctypes.data if c.size else None, out.ctypes.data)
    return rc, out


def test_null_for_sum_min_and_max(world):
    eng, depth = world
    want = D.hist(depth, [(1, 0, LB), (2, S, E)], 65536)
    rc, bins, tot, lo, hi = _raw_hist(eng, [(1, 0, LB), (2, S, E)], 65536, stats=False)
    assert rc == 0 and np.array_equal(bins, want[0]) and (tot, lo, hi) == (-7, -8, -9)
    tot = C.c_int64(-7)
    t, s, e = np.array([2], np.int32), np.array([S], np.int64), np.array([E], np.int64)
    bins = np.zeros(4, np.uint64)
    assert eng._lib.gd_depth_hist(eng._ctx, 1, t.ctypes.data, s.ctypes.data, e.ctypes.data, 4, bins.ctypes.data, C.byref(tot), None, None) == 0
    assert tot.value == D.hist(depth, [(2, S, E)], 4)[1] and bins.tolist() == [0, 1, 1, E - S - 2]


@pytest.mark.parametrize("cuts", CUT_LISTS)
def test_region_bins(world, region_lists, cuts):
    eng, depth = world
    for name in ("aligned", "mixed", "random"):
        same_bins(eng, depth, region_lists[name], cuts)
    same_bins(eng, depth, [(0, 0, LA), (1, 0, LB), (2, 0, LC)], cuts)
    same_bins(eng, depth, [(2, S, E)], cuts)


def test_two_calls_give_the_same_numbers(world, region_lists):
    eng, _ = world
    t, s, e = ([r[k] for r in region_lists["random"]] for k in range(3))
    a, b = eng.depth_hist(t, s, e, 65536), eng.depth_hist(t, s, e, 65536)
    assert a[0].tobytes() == b[0].tobytes() and a[1:] == b[1:]
    assert eng.region_bins(t, s, e, [1, 4, 100]).tobytes() == eng.region_bins(t, s, e, [1, 4, 100]).tobytes()


def test_refusals_leave_the_context_and_the_outputs_as_they_were(world):
    eng, depth = world
    ok = (1, 5, 70_001)
    bad_regions = [(1, -1, 10), (1, 20, 10), (1, 0, LB + 1), (1, LB + 1, LB + 1), (-1, 0, 10), (3, 0, 10)]
    for bad in bad_regions:
        for regions in ([bad], [ok, bad], [bad, ok]):
            rc, bins, tot, lo, hi = _raw_hist(eng, regions, 64)
            assert rc == E_RANGE, (regions, rc)
            assert (bins == 0xDEADBEEF).all() and (tot, lo, hi) == (-7, -8, -9)
            rc, out = _raw_bins(eng, regions, [1, 2])
            assert rc == E_RANGE and (out == 0xDEADBEEF).all(), (regions, rc)
        same_hist(eng, depth, [ok], 64)
        same_bins(eng, depth, [ok], [1, 2])
    for n_bins in (0, -1, 65537, 2 ** 31 - 1):
        rc, bins, tot, lo, hi = _raw_hist(eng, [ok], n_bins, cap=8)
        assert rc == E_INVALID and (bins == 0xDEADBEEF).all() and (tot, lo, hi) == (-7, -8, -9), n_bins
        same_hist(eng, depth, [ok, (2, S, S + 100)], 65536)
    assert _raw_hist(eng, [(1, -1, 10)], 0, cap=8)[0] == E_RANGE                 # coordinates are judged before the bins
    for cuts in ([2, 2], [3, 2], [0], [-5, 3], list(range(1, 34))):
        rc, out = _raw_bins(eng, [ok], cuts)
        assert rc == E_INVALID and (out == 0xDEADBEEF).all(), cuts
        same_bins(eng, depth, [ok, (0, ZERO - 3, ZERO + 3)], [1, 2])
    assert _raw_bins(eng, [(1, 20, 10)], [3, 2])[0] == E_RANGE
    t = np.array([1], np.int32)
    s = np.array([0], np.int64)
    assert eng._lib.gd_depth_hist(eng._ctx, 1, t.ctypes.data, s.ctypes.data, s.ctypes.data, 4, None, None, None, None) == E_INVALID
    assert eng._lib.gd_depth_hist(eng._ctx, 1, None, s.ctypes.data, s.ctypes.data, 4, t.ctypes.data, None, None, None) == E_INVALID
    assert eng._lib.gd_region_bins(eng._ctx, 1, t.ctypes.data, s.ctypes.data, s.ctypes.data, 0, None, None) == E_INVALID
    assert eng._lib.gd_region_bins(eng._ctx, 1, t.ctypes.data, s.ctypes.data, s.ctypes.data, 2, None, s.ctypes.data) == E_INVALID
    same_hist(eng, depth, [ok], 64)


def test_state_refusals():
    """Before a compute, while one is in flight, and after a compute that kept no per-base vector -- on a context of its
    own: the module's is computed once."""
    from goleft_amd.engine import DepthEngine
    rng = np.random.default_rng(98)
    L = 20_011
    r = H.random_reads(rng, L, 1_500)
    d = [po.perbase_c(r, 1, 0, L)]
    whole = [(0, 0, L)]

    def refused(eng):
        rc, bins, tot, lo, hi = _raw_hist(eng, whole, 16)
        rc2, out = _raw_bins(eng, whole, [1])
        return rc == rc2 == E_STATE and (bins == 0xDEADBEEF).all() and (tot, lo, hi) == (-7, -8, -9) and (out == 0xDEADBEEF).all()

    with DepthEngine(0) as eng:
        eng.set_params()
        eng.set_contigs([L])
        eng.push(0, r.pos, r.flag, r.mapq, r.cigar_off, r.cigar)
        assert refused(eng)                                                            # before a compute
        assert _raw_hist(eng, [], 16)[0] == E_STATE and _raw_bins(eng, [], [])[0] == E_STATE
        eng.compute()
        same_hist(eng, d, whole, 16)
        eng.compute_launch()
        ok = refused(eng)
        eng.compute_finish()
        assert ok                                                                      # while one is in flight
        same_bins(eng, d, [(0, 3, L - 3)], [2, 4, 100])
        eng.set_outputs(perbase=False)
        assert refused(eng)                                                            # (the outputs changed: no results)
        eng.compute()
        assert refused(eng)                                                            # computed without GD_OUT_PERBASE
        assert _raw_hist(eng, [(0, 5, 5)], 16)[0] == E_STATE and _raw_hist(eng, [], 16)[0] == E_STATE
        eng.set_outputs(perbase=True)
        eng.compute()
        same_hist(eng, d, whole, 16)
        same_bins(eng, d, whole, [1])


def test_the_long_read_route_produces_the_vector_too():
    """GD_PATH_CHUNK: the per-base vector has another producer (gd_ltile2_kernel)."""
    from goleft_amd import engine as EN
    rng = np.random.default_rng(5)
    L = 60_001
    r = H.long_cigar_reads(rng, L, [int(x) for x in rng.integers(1, 900, size=120)], skip_every=7)
    d = [po.perbase_c(r, 1, 0, L)]
    with EN.DepthEngine(0) as eng:
        eng.set_params()
        eng.set_path(EN.PATH_CHUNK)
        eng.set_contigs([L])
        eng.push(0, r.pos, r.flag, r.mapq, r.cigar_off, r.cigar)
        eng.compute()
        assert eng.stats().tile_kernel == EN.TK_LONG
        same_hist(eng, d, [(0, 0, L)], 256)
        same_hist(eng, d, [(0, 4097, L - 2), (0, 12_345, 23_456)], 4)
        same_bins(eng, d, [(0, 0, L), (0, 4097, L - 2), (0, 12_345, 23_456)], [1, 2, 100])
