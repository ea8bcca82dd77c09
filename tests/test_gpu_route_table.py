"""-m gpu: which kernel gd_compute runs -- its route -- for every combination of what the route depends on, and that
each route computes what the oracle computes.

The rule, in order:

    path SCATTER, per-base not kept                                   GD_E_INVALID, nothing launched
    path SCATTER                                                      TK_SCATTER          path SCATTER
    path CHUNK, or AUTO and more than 6 ops per read                  TK_LONG             path CHUNK   (sums-only ignored)
    sums-only, W >= 32, fast kernel on, arrays aligned                TK_SUMS_STREAM_RAW  path TILE
    sums-only, W >= 32 otherwise                                      TK_TILE_SUMS        path TILE
    fast kernel on and arrays aligned                                 TK_FAST_RAW         path TILE
    otherwise                                                         TK_GENERIC          path TILE

One context per row.  (AUTO leaving the tile path after a long span and the look-back re-run are pinned by
test_gpu_parity, test_gpu_ingest_index and test_gpu_async.)"""
import itertools

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import helpers as H
from tests.test_gpu_filter_edges import device_arrays

pytestmark = pytest.mark.gpu

LENS = (9_001, 5_000)                   # neither a multiple of the 4096-position tile: clipped tiles on the slow list
N_READS = 300
Q, MASK, MINCOV = 1, 0x704, 4
E_INVALID, E_STATE = -1, -4
OUTPUTS = ("perbase", "windows", "sums")


def make_reads(rng, length, n, ops_per_read):
    """n records of exactly ops_per_read[k] ops each (M I D N S = X, 1-40 bases), spans far below 32 768."""
    pos = np.sort(rng.integers(0, length, size=n)).astype(np.int32)
    off = np.zeros(n + 1, np.uint32)
    off[1:] = np.cumsum(ops_per_read)
    m = int(off[-1])
    ops = rng.choice([0, 1, 2, 3, 4, 7, 8], size=m, p=[0.5, 0.1, 0.15, 0.05, 0.05, 0.1, 0.05])
    lens = rng.integers(1, 41, size=m)
    cigar = ((lens.astype(np.uint32) << 4) | ops.astype(np.uint32)).astype(np.uint32)
    flag = rng.choice([0, 16, 99, 0x400, 0x100, 0x4], size=n, p=[0.4, 0.3, 0.15, 0.05, 0.05, 0.05]).astype(np.uint16)
    mapq = rng.choice([0, 1, 60], size=n, p=[0.1, 0.2, 0.7]).astype(np.uint8)
    return po.Reads(pos, flag, mapq, off, cigar)


class Shape:
    """The records of one shape and what the oracle makes of them, computed once."""

    def __init__(self, name):
        rng = np.random.default_rng({"short": 11, "long": 12}[name])
        self.reads = {}
        for tid, L in enumerate(LENS):
            nops = rng.integers(1, 3, size=N_READS) if name == "short" else np.full(N_READS, 8)
            self.reads[tid] = make_reads(rng, L, N_READS, nops)
        n_ops, n = sum(r.n_ops for r in self.reads.values()), sum(r.n for r in self.reads.values())
        assert (n_ops > 6 * n) == (name == "long")
        self.depth = {t: po.perbase_c(r, Q, 0, LENS[t], flag_mask=MASK) for t, r in self.reads.items()}
        self.win = {(t, W): H.oracle_windows(d, W) for t, d in self.depth.items() for W in (25, 100)}
        self.runs = {(t, W): H.oracle_runs(d, MINCOV, 0, po.step_for(W)) for t, d in self.depth.items() for W in (25, 100)}


@pytest.fixture(scope="module")
def shapes():
    return {name: Shape(name) for name in ("short", "long")}


def expected_route(path, out, fast, aligned, W, shape):
    """(tile_kernel, path) or the error, literally the table in the module docstring."""
    if path == "SCATTER" and out != "perbase":
        return E_INVALID
    if path == "SCATTER":
        return "TK_SCATTER", "SCATTER"
    if path == "CHUNK" or (path == "AUTO" and shape == "long"):
        return "TK_LONG", "CHUNK"
    if out == "sums" and W >= 32 and fast and aligned:
        return "TK_SUMS_STREAM_RAW", "TILE"
    if out == "sums" and W >= 32:
        return "TK_TILE_SUMS", "TILE"
    if fast and aligned:
        return "TK_FAST_RAW", "TILE"
    return "TK_GENERIC", "TILE"


def configure(eng, sh, path, out, fast, aligned, W):
    from goleft_amd import engine as E
    eng.set_path(getattr(E, "PATH_" + path))
    eng.set_outputs(perbase=out == "perbase", sums_only=out == "sums")
    eng.set_option(E.OPT_FAST_KERNEL, fast)
    eng.set_params(window_size=W, min_mapq=Q, min_cov=MINCOV, flag_mask=MASK)
    eng.set_contigs(LENS)
    for tid, r in sh.reads.items():
        eng.adopt_device(tid, *device_arrays(r, () if aligned else ("pos",)))


def check_results(eng, sh, W, sums_only_route, perbase, row):
    from goleft_amd.engine import GdError
    for tid in range(len(LENS)):
        ws, wm = sh.win[tid, W]
        assert np.array_equal(eng.window_sums(tid), ws), "%s: window sums of contig %d" % (row, tid)
        if sums_only_route:
            for what, call in (("windows with minima", eng.windows), ("callable runs", eng.callable_runs)):
                with pytest.raises(GdError) as ei:
                    call(tid)
                assert ei.value.status == E_STATE, "%s: %s answered %d" % (row, what, ei.value.status)
            continue
        sums, mins = eng.windows(tid)
        assert np.array_equal(sums, ws), "%s: window sums of contig %d" % (row, tid)
        assert np.array_equal(mins, wm), "%s: window minima of contig %d" % (row, tid)
        assert np.array_equal(eng.callable_runs(tid), sh.runs[tid, W]), "%s: callable runs of contig %d" % (row, tid)
        if perbase:
            assert np.array_equal(eng.perbase(tid), sh.depth[tid]), "%s: per-base depth of contig %d" % (row, tid)


@pytest.mark.parametrize("shape", ["short", "long"])
@pytest.mark.parametrize("path", ["AUTO", "TILE", "SCATTER", "CHUNK"])
def test_route_table(shapes, path, shape):
    from goleft_amd import engine as E
    from goleft_amd.engine import DepthEngine, GdError
    sh = shapes[shape]
    for out, fast, aligned, W in itertools.product(OUTPUTS, (0, 1), (True, False), (25, 100)):
        row = "path %s, %s, fast_kernel %d, %s, W %d, %s reads" % (path, out, fast, "aligned" if aligned else "misaligned",
                                                                   W, shape)
        want = expected_route(path, out, fast, aligned, W, shape)
        with DepthEngine(0) as eng:
            configure(eng, sh, path, out, fast, aligned, W)
            if want == E_INVALID:
                with pytest.raises(GdError) as ei:
                    eng.compute()
                assert ei.value.status == E_INVALID, "%s: status %d" % (row, ei.value.status)
                continue
            eng.compute()
            st = eng.stats()
            assert (st.tile_kernel, st.path) == (getattr(E, want[0]), getattr(E, "PATH_" + want[1])), \
                "%s: ran kernel %d on path %d, expected %s on %s" % (row, st.tile_kernel, st.path, want[0], want[1])
            check_results(eng, sh, W, want[0] in ("TK_SUMS_STREAM_RAW", "TK_TILE_SUMS"), out == "perbase", row)


def test_a_sums_only_attempt_rerun_on_the_long_read_route_has_minima_and_runs():
    """AUTO, sums-only, the straight-line kernels off: the first attempt is TK_TILE_SUMS; one spliced read of 60 kb
    makes the compute run again as TK_LONG, which ignores sums-only -- so what the results answer follows the LAST
    attempt: minima and callable runs are there."""
    from goleft_amd import engine as E
    from goleft_amd.engine import DepthEngine
    L, W = 100_001, 100
    rng = np.random.default_rng(13)
    r = make_reads(rng, L, N_READS, rng.integers(1, 3, size=N_READS))
    k = int(np.searchsorted(r.pos, 20_000))
    a, b = int(r.cigar_off[k]), int(r.cigar_off[k + 1])
    cigar = np.concatenate([r.cigar[:a], np.array([50 << 4, (60_000 << 4) | 3, 50 << 4], np.uint32), r.cigar[b:]])
    off = r.cigar_off.astype(np.int64)
    off[k + 1:] += 3 - (b - a)
    flag, mapq = r.flag.copy(), r.mapq.copy()
    flag[k], mapq[k] = 0, 60
    r = po.Reads(r.pos, flag, mapq, off.astype(np.uint32), cigar)
    assert r.n_ops <= 6 * r.n
    d = po.perbase_c(r, Q, 0, L, flag_mask=MASK)
    ws, wm = H.oracle_windows(d, W)
    with DepthEngine(0) as eng:
        eng.set_path(E.PATH_AUTO)
        eng.set_outputs(perbase=False, sums_only=True)
        eng.set_option(E.OPT_FAST_KERNEL, 0)
        eng.set_params(window_size=W, min_mapq=Q, min_cov=MINCOV, flag_mask=MASK)
        eng.set_contigs([L])
        eng.push(0, r.pos, r.flag, r.mapq, r.cigar_off, r.cigar)
        eng.compute()
        st = eng.stats()
        assert (st.tile_kernel, st.path) == (E.TK_LONG, E.PATH_CHUNK) and st.reruns >= 1, (st.tile_kernel, st.path, st.reruns)
        sums, mins = eng.windows(0)
        assert np.array_equal(sums, ws) and np.array_equal(mins, wm)
        assert np.array_equal(eng.callable_runs(0), H.oracle_runs(d, MINCOV, 0, po.step_for(W)))


def test_compute_after_a_refused_enqueue(shapes):
    """Windows-only output on the scatter path is refused (before anything is enqueued); the next compute of the same
    context is as good as a fresh context's, its count of slow tiles -- which alternates between two device counters
    from compute to compute -- included."""
    from goleft_amd import engine as E
    from goleft_amd.engine import DepthEngine, GdError
    sh = shapes["short"]
    with DepthEngine(0) as fresh:
        configure(fresh, sh, "TILE", "perbase", 1, True, 100)
        fresh.compute()
        want_slow = fresh.stats().n_slow_tiles
    assert want_slow >= len(LENS)                          # at least the clipped last tile of each contig
    with DepthEngine(0) as eng:
        configure(eng, sh, "SCATTER", "windows", 1, True, 100)
        with pytest.raises(GdError) as ei:
            eng.compute()
        assert ei.value.status == E_INVALID
        eng.set_path(E.PATH_TILE)
        eng.set_outputs(perbase=True)
        eng.compute()
        st = eng.stats()
        assert (st.tile_kernel, st.path) == (E.TK_FAST_RAW, E.PATH_TILE)
        assert st.n_slow_tiles == want_slow
        check_results(eng, sh, 100, False, True, "after the refused enqueue")
