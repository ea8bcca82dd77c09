"""-m gpu: gd_perbase_runs through DepthEngine against the numpy restatement
(tests/perbase_runs_ref.py) applied to the CPU oracle's per-base vector: exact equality everywhere.

One module-scoped context, computed once.  Contig A (3 * 2^20 + 5 positions) is designed: depth alternates 1 / 0 at every
position of [0, 2^21) -- one-base reads at the even positions: 2^21 runs, 512 chunks of 4096 run starts each, many rounds
of the scan --, then it is 3 to the end (three long reads), and on top of that a read starts at m - 1, m and m + 1 for
every m = 2^21 + 2^j, j = 4 .. 20: a run boundary just before, on and just after every edge a lane (16 positions), a wave
(1024), a chunk (4096 -- a power of two: its multiples are in the sweep) or any power-of-two chunk up to 2^20 can have.
Contig B (150 001) is H.random_reads merged with H.edge_reads, at the default filter."""
import ctypes as C

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import helpers as H
from tests import perbase_runs_ref as R

pytestmark = pytest.mark.gpu

ALT = 1 << 21                               # end of the alternating part of contig A
LA, LB = 3 * (1 << 20) + 5, 150_001
STEPS = [ALT + (1 << j) for j in range(4, 21)]
E_INVALID, E_STATE, E_RANGE, E_CAPACITY = -1, -4, -5, -8
CUTS32 = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 14, 16, 18, 20, 25, 30, 35, 40, 50, 60, 70, 80, 90, 100, 150, 200, 300, 1000,
          100000, 2 ** 30, 2 ** 31 - 1]


def merged(a, b):
    """Two record sets as one, in position order."""
    pos = np.concatenate([a.pos, b.pos])
    order = np.argsort(pos, kind="stable")
    nops = np.concatenate([np.diff(a.cigar_off.astype(np.int64)), np.diff(b.cigar_off.astype(np.int64))])
    first = np.concatenate([a.cigar_off[:-1].astype(np.int64), b.cigar_off[:-1].astype(np.int64) + len(a.cigar)])
    cig = np.concatenate([a.cigar, b.cigar])
    off = np.zeros(len(pos) + 1, np.uint32)
    off[1:] = np.cumsum(nops[order])
    idx = np.concatenate([np.arange(first[k], first[k] + nops[k]) for k in order]) if len(order) else np.zeros(0, np.int64)
    return po.Reads(pos[order].astype(np.int32), np.concatenate([a.flag, b.flag])[order], np.concatenate([a.mapq, b.mapq])[order],
                    off, cig[idx.astype(np.int64)].astype(np.uint32))


def reads_a():
    pos = [np.arange(0, ALT, 2, dtype=np.int64), np.full(3, ALT, np.int64)]
    span = [np.ones(ALT // 2, np.int64), np.full(3, LA - ALT, np.int64)]
    for m in STEPS:
        pos.append(np.array([m - 1, m, m + 1], np.int64))
        span.append(np.full(3, 8, np.int64))
    pos, span = np.concatenate(pos), np.concatenate(span)
    assert (np.diff(pos) >= 0).all()
    n = len(pos)
    return po.Reads(pos.astype(np.int32), np.zeros(n, np.uint16), np.full(n, 60, np.uint8), np.arange(n + 1, dtype=np.uint32),
                    (span.astype(np.uint32) << 4))                       # one M op per record


@pytest.fixture(scope="module")
def world():
    """(engine, [oracle vector of A, of B]): computed once, unchanged by the tests."""
    from goleft_amd.engine import DepthEngine
    rng = np.random.default_rng(321)
    reads = [reads_a(), merged(H.random_reads(rng, LB, 9_000), H.edge_reads(rng, LB, 4_000))]
    eng = DepthEngine(0)
    eng.set_params()
    eng.set_contigs([LA, LB])
    for tid, r in enumerate(reads):
        eng.push(tid, r.pos, r.flag, r.mapq, r.cigar_off, r.cigar)
    eng.compute()
    depth = [po.perbase_c(r, 1, 0, L) for r, L in zip(reads, (LA, LB))]
    yield eng, depth
    eng.close()


def same(eng, depth, tid, start, end, cuts=None):
    ws, wv = R.runs(depth[tid], start, end, cuts)
    gs, gv = eng.perbase_runs(tid, start, end, cuts)
    assert gs.dtype == np.uint32 and gv.dtype == np.int32
    assert gs.shape == ws.shape, (tid, start, end, cuts, gs.shape, ws.shape)
    bad = np.flatnonzero((gs != ws) | (gv != wv))
    assert bad.size == 0, (tid, start, end, cuts, int(bad[0]), int(gs[bad[0]]), int(gv[bad[0]]), int(ws[bad[0]]), int(wv[bad[0]]))
    return len(ws)


def test_the_designed_profile_is_what_the_oracle_sees(world):
    _, depth = world
    a = depth[0]
    assert np.array_equal(a[:ALT], np.tile(np.array([1, 0], np.int32), ALT // 2))
    assert a[ALT] == 3 and a[LA - 10] == 3 and a[LA - 1] == 6 and int(a[ALT:].min()) == 3
    for m in STEPS:
        assert a[m - 2:m + 10].tolist() == [3, 4, 5, 6, 6, 6, 6, 6, 6, 5, 4, 3][:LA - m + 2], m      # (the last ones hang over the end)


def test_whole_contigs(world):
    eng, depth = world
    assert same(eng, depth, 0, 0, LA) == ALT + 1 + 6 * len(STEPS) - 3                     # (the last step's reads end with the contig)
    assert same(eng, depth, 1, 0, LB) > 1000
    assert eng.perbase_runs(0)[0].shape[0] == ALT + 1 + 6 * len(STEPS) - 3  # end=None: the contig's length
    t = eng.perbase_runs_timing()
    assert set(t) == {"count_s", "scan_s", "emit_s", "readback_s"} and all(v > 0 for v in t.values())


def test_empty_and_single_position_regions(world):
    eng, depth = world
    for tid, L in ((0, LA), (1, LB)):
        for p in (0, L // 2, L):
            s, v = eng.perbase_runs(tid, p, p)
            assert s.shape == (0,) and v.shape == (0,)
        assert same(eng, depth, tid, 0, 1) == 1
        assert same(eng, depth, tid, L - 1, L) == 1


@pytest.mark.parametrize("tid, base", [(0, 4096 * 3), (0, ALT - 8), (0, ALT + 4096 - 8), (1, 70_000)])
def test_heads_and_tails_of_every_alignment(world, tid, base):
    """start and end over all residues mod 4 (the scalar head and tail next to the 16-byte loads), short and long."""
    eng, depth = world
    for ds in range(4):
        for de in range(4):
            for span in (0, 4, 16, 4096, 3 * 4096 + 16):
                if ds <= span + de:
                    same(eng, depth, tid, base + ds, base + span + de)


def test_regions_of_the_designed_parts(world):
    eng, depth = world
    assert same(eng, depth, 0, 1000, 1000 + 3 * 4096 + 7) == 3 * 4096 + 7                 # inside the alternating part
    assert same(eng, depth, 0, ALT + 300, ALT + 500) == 1                                 # inside the constant part: one run
    assert same(eng, depth, 0, ALT + (1 << 19) + 20, ALT + (1 << 20) - 20) == 1
    assert same(eng, depth, 0, LA - 4, LA) == 1
    assert same(eng, depth, 0, ALT - 5000, ALT + 5000) > 5000                             # across their border
    assert same(eng, depth, 0, ALT + 1, ALT + 9) == 1                                     # a start strictly inside a run
    for m in STEPS:                                                                      # ... and at, before and behind every step
        for s in (m - 2, m - 1, m, m + 1, m + 2, m + 3):
            same(eng, depth, 0, s, min(LA, m + 40))
        same(eng, depth, 0, m - 4100, min(LA, m + 4100))
    d = depth[1]
    inside = [int(p) for p in np.flatnonzero((d[1:-1] == d[:-2]) & (d[1:-1] == d[2:]) & (d[1:-1] > 0))[:5] + 1]
    assert len(inside) == 5
    for p in inside:                                                                      # contig B: a start strictly inside a run
        same(eng, depth, 1, p, min(LB, p + 9000))


def test_cuts(world):
    eng, depth = world
    present = int(np.bincount(depth[1]).argmax() or 7)                                    # a depth the vector holds
    assert (depth[1] == present).any()
    sweeps = [[1], [1, 2], [2, 4, 100], CUTS32, [present], [present - 1] if present > 1 else [present + 2], [present + 1],
              [max(1, present - 1), present, present + 1] if present > 1 else [present, present + 1], [3], [4], [5], [3, 4, 5, 6, 7]]
    for cuts in sweeps:
        same(eng, depth, 1, 0, LB, cuts)
        same(eng, depth, 1, 33_333, 77_777, cuts)
        same(eng, depth, 0, ALT - 4099, ALT + 4099, cuts)
    for cuts in ([1], [2, 4, 100], [4], [3, 4, 5, 6, 7], CUTS32):
        same(eng, depth, 0, 0, LA, cuts)
    s, v = eng.perbase_runs(0, 0, ALT, [2])                                               # depths 0 and 1 share bin 0: one run
    assert s.tolist() == [0] and v.tolist() == [0]


def _raw(eng, tid, start, end, cuts, cap, sentinel=True):
    """The C call itself: (rc, n, starts, values) with room for cap runs, sentinel filled."""
    c = np.ascontiguousarray(cuts, np.int32)
    s = np.full(max(cap, 1), 0xDEADBEEF, np.uint32)
    v = np.full(max(cap, 1), -77, np.int32)
    n = C.c_size_t(12345)
    rc = eng._lib.gd_perbase_runs(eng._ctx, tid, start, end, c.size, c.ctypes.data if c.size else None, s.ctypes.data, v.ctypes.data,
                                  cap, C.byref(n))
    return rc, n.value, s, v


def test_capacity_protocol(world):
    eng, depth = world
    for tid, a, b, cuts in ((1, 10, 90_000, []), (1, 0, LB, [2, 4, 100]), (0, ALT - 10_000, ALT + 100, [])):
        ws, wv = R.runs(depth[tid], a, b, cuts)
        k = len(ws)
        n = C.c_size_t()
        c = np.ascontiguousarray(cuts, np.int32)
        rc = eng._lib.gd_perbase_runs(eng._ctx, tid, a, b, c.size, c.ctypes.data if c.size else None, None, None, 0, C.byref(n))
        assert (rc, n.value) == (E_CAPACITY, k)                                            # the counting call
        rc, got, s, v = _raw(eng, tid, a, b, cuts, k - 1)
        assert (rc, got) == (E_CAPACITY, k)
        assert (s == 0xDEADBEEF).all() and (v == -77).all()                                # outputs untouched
        rc, got, s, v = _raw(eng, tid, a, b, cuts, k)
        assert (rc, got) == (0, k) and np.array_equal(s, ws) and np.array_equal(v, wv)
        rc, got, s, v = _raw(eng, tid, a, b, cuts, k + 3)
        assert (rc, got) == (0, k) and np.array_equal(s[:k], ws) and (s[k:] == 0xDEADBEEF).all() and (v[k:] == -77).all()


def test_two_calls_give_the_same_bytes(world):
    eng, _ = world
    for tid, cuts in ((0, None), (1, None), (1, [1, 4, 100])):
        a, b = eng.perbase_runs(tid, 0, None, cuts), eng.perbase_runs(tid, 0, None, cuts)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_refusals_leave_the_context_as_it_was(world):
    eng, depth = world
    cases = [(E_RANGE, (1, -1, 10, [])), (E_RANGE, (1, 20, 10, [])), (E_RANGE, (1, 0, LB + 1, [])), (E_RANGE, (1, LB + 1, LB + 1, [])),
             (E_RANGE, (-1, 0, 10, [])), (E_RANGE, (2, 0, 10, [])),
             (E_INVALID, (1, 0, 10, [2, 2])), (E_INVALID, (1, 0, 10, [3, 2])), (E_INVALID, (1, 0, 10, [0])),
             (E_INVALID, (1, 0, 10, [-5, 3])), (E_INVALID, (1, 0, 10, list(range(1, 34))))]
    for want, (tid, a, b, cuts) in cases:
        rc, n, s, v = _raw(eng, tid, a, b, cuts, 64)
        assert rc == want, (tid, a, b, cuts, rc)
        assert n == 12345 and (s == 0xDEADBEEF).all() and (v == -77).all()
        same(eng, depth, 1, 5, 70_001, [1, 2])
        same(eng, depth, 0, ALT - 50, ALT + 50)


def test_state_refusals():
    """Before a compute, while one is in flight, and after a compute that kept no per-base vector -- on a context of its
    own: the module's is computed once."""
    from goleft_amd.engine import DepthEngine
    rng = np.random.default_rng(99)
    L = 20_011
    r = H.random_reads(rng, L, 1_500)
    d = [po.perbase_c(r, 1, 0, L)]
    with DepthEngine(0) as eng:
        eng.set_params()
        eng.set_contigs([L])
        eng.push(0, r.pos, r.flag, r.mapq, r.cigar_off, r.cigar)
        assert _raw(eng, 0, 0, L, [], 64)[0] == E_STATE                                    # before a compute
        eng.compute()
        same(eng, d, 0, 0, L)
        eng.compute_launch()
        rc, n, s, v = _raw(eng, 0, 0, L, [], 64)
        eng.compute_finish()
        assert rc == E_STATE and n == 12345 and (s == 0xDEADBEEF).all()                    # while one is in flight
        same(eng, d, 0, 3, L - 3, [2, 4, 100])
        eng.set_outputs(perbase=False)
        assert _raw(eng, 0, 0, L, [], 64)[0] == E_STATE                                    # (the outputs changed: no results)
        eng.compute()
        assert _raw(eng, 0, 0, L, [], 64)[0] == E_STATE                                    # computed without GD_OUT_PERBASE
        assert _raw(eng, 0, 5, 5, [], 64)[0] == E_STATE
        eng.set_outputs(perbase=True)
        eng.compute()
        same(eng, d, 0, 0, L)
        same(eng, d, 0, 1, L - 1, [1])


def test_the_long_read_route_produces_the_vector_too():
    """GD_PATH_CHUNK: the per-base vector has another producer (gd_ltile2_kernel)."""
    from goleft_amd import engine as E
    rng = np.random.default_rng(5)
    L = 60_001
    r = H.long_cigar_reads(rng, L, [int(x) for x in rng.integers(1, 900, size=120)], skip_every=7)
    d = [po.perbase_c(r, 1, 0, L)]
    with E.DepthEngine(0) as eng:
        eng.set_params()
        eng.set_path(E.PATH_CHUNK)
        eng.set_contigs([L])
        eng.push(0, r.pos, r.flag, r.mapq, r.cigar_off, r.cigar)
        eng.compute()
        assert eng.stats().tile_kernel == E.TK_LONG
        assert same(eng, d, 0, 0, L) > 100
        same(eng, d, 0, 4097, L - 2, [1, 2])
        same(eng, d, 0, 12_345, 23_456, [2, 4, 100])
