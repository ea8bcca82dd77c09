"""-m gpu: the long-read kernels at their structural edges -- the deletion-list pass (gd_dels_raw_kernel: the lane's
and the wave's walk at 24 | 25 ops, the wave walk's batches of 256 ops and its three load slots, list slots and index
slots exactly full and one past, the merging fallback walks, the 2^22-base op limit and the two position caps, units
of 64 reads, several contigs and blocks) and the long-read tile kernel (gd_ltile2_kernel: candidate batches of 256,
reads and deletions on the tile's edges, the look-back's rounding, the index and the bisected list, pieces of 64 and
the 128-item queue, clipped tiles).  The shapes come from tests/long_shapes.py; tests/test_long_shapes.py shows on the
CPU that each one reaches its edge.

Every case runs through the C ABI on GD_PATH_CHUNK, with the per-base vector kept and dropped (gd_ltile2_kernel<1> and
<2>), and is compared with the C oracle, exactly: the whole per-base vector where it is kept, window sums and minima,
the class runs of every contig, and for one case per family --bed regions around the crafted positions.  gd_stats says
which kernel ran; n_tiles, n_runs, reruns, lookback, max_span_seen and n_deletions are held against the routing model.
Every case is computed twice on its context and once more after gd_rebuild_derived: no result may change."""
import numpy as np
import pytest

from tests import helpers as H
from tests import long_shapes as LS
from tests.test_gpu_tile_shapes import run_start, same

pytestmark = pytest.mark.gpu

OUTPUTS = {"perbase": True, "windows": False}              # gd_ltile2_kernel<1> / <2>
SECOND_W = 512                                             # the deletion-list cases again on a divisor of the tile size


def regions_of(c):
    """A few --bed regions that straddle the positions a case is about (tile edges otherwise)."""
    L = c.lengths[0]
    at = [c.mark["t0"]] if "t0" in c.mark else [LS.T, 2 * LS.T]
    pts = sorted({p for a in at for p in (a, a + 1024, a + LS.T)} | {0, L})
    out = []
    for p in pts:
        for a, b in ((p - 7, p + 9), (p - 300, p + 1), (p, p + 1), (p - 1, p)):
            if 0 <= a < b and a < L:
                out.append((0, a, b))
    return out[:24]


def configure(eng, c, perbase, W):
    from goleft_amd import engine as E
    eng.set_path(E.PATH_CHUNK)
    eng.set_outputs(perbase=perbase)
    eng.set_option(E.OPT_INGEST_INDEX, int(c.index))
    eng.set_params(window_size=W, min_mapq=c.Q, min_cov=c.min_cov, max_mean_depth=c.max_mean_depth, flag_mask=c.flag_mask)
    eng.set_contigs(c.lengths)
    for tid, r in c.reads.items():
        cuts = LS.block_cuts(r.n, c.blocks)
        for a, b in zip(cuts, cuts[1:]):
            s = r.slice(a, b)
            eng.push(tid, s.pos, s.flag, s.mapq, s.cigar_off, s.cigar)


def check(eng, c, out, W, attempt, with_regions):
    """One compute of a configured case against the oracle and the model -> list of messages (empty: all equal)."""
    from goleft_amd import engine as E
    perbase = OUTPUTS[out]
    eng.compute()
    st = eng.stats()
    ctx0 = "case %s (%s), W %d, %s, compute %d" % (c.name, c.edge, W, out, attempt)
    if st.tile_kernel != E.TK_LONG or st.path != E.PATH_CHUNK:
        return ["%s: ran kernel %s on path %d, expected gd_ltile2_kernel on GD_PATH_CHUNK" % (ctx0, E.TK_NAMES[st.tile_kernel], st.path)]
    bad = []
    orc = LS.oracle(c.name, 0 if W == c.W else W)
    for t, L in enumerate(c.lengths):
        ctx = "%s, contig %d" % (ctx0, t)
        ws, wm, runs, d = orc[t]
        wpos = lambda k, g, w: k * W
        if perbase:
            bad.append(same(eng.perbase(t), d, ctx, "per-base depths", lambda k, g, w: k))
        sums, mins = eng.windows(t)
        bad.append(same(sums, ws, ctx, "window sums", wpos))
        bad.append(same(mins, wm, ctx, "window minima", wpos))
        bad.append(same(eng.callable_runs(t), runs, ctx, "callable runs", run_start))
    if with_regions and perbase:
        reg = regions_of(c)
        rs, rm, rr = eng.regions([r[0] for r in reg], [r[1] for r in reg], [r[2] for r in reg])
        for k, (t, a, b) in enumerate(reg):
            ctx = "%s, contig %d, --bed region %d-%d" % (ctx0, t, a, b)
            d = np.zeros(b - a, np.int32)
            hi = min(b, c.lengths[t])
            d[:hi - a] = orc[t][3][a:hi]
            ws, wm = H.oracle_windows(d, W, a)
            wpos = lambda k, g, w, a=a: max(a, (a // W + k) * W)
            bad.append(same(rs[k], ws, ctx, "region window sums", wpos))
            bad.append(same(rm[k], wm, ctx, "region window minima", wpos))
            bad.append(same(rr[k], H.oracle_runs(d, c.min_cov, c.max_mean_depth, 1 << 62, a), ctx, "region runs", run_start))
    # the routing model
    want = dict(LS.job_model(c), n_tiles=c.n_tiles, n_runs=sum(len(o[2]) for o in orc), reruns=0)
    for k, v in want.items():
        if getattr(st, k) != v:
            bad.append("%s: gd_stats.%s is %d, the model says %d" % (ctx0, k, getattr(st, k), v))
    return [b for b in bad if b]


# (contigs too long for a per-base vector run with the vector dropped only)
PAIRS = [(f, o) for f in LS.FAMILIES for o in OUTPUTS
         if not OUTPUTS[o] or not all(LS.case(n).sparse for n in LS.names(f))]


@pytest.mark.parametrize("family,out", PAIRS)
def test_long_read_kernels_at_structural_edges(family, out):
    from goleft_amd.engine import DepthEngine
    bad = []
    with DepthEngine(0) as eng:                            # one context per family and output, shared by its cases
        for i, name in enumerate(LS.names(family)):
            c = LS.case(name)
            assert not (c.sparse and OUTPUTS[out])
            for W in (c.W, SECOND_W) if family in LS.DL_FAMILIES and not c.sparse else (c.W,):
                configure(eng, c, OUTPUTS[out], W)
                for attempt in (1, 2):
                    bad += check(eng, c, out, W, attempt, with_regions=i == 0 and attempt == 1)
                eng.rebuild_derived()                      # the same structures again, into the block they occupy
                bad += check(eng, c, out, W, 3, False)
    assert not bad, "%d comparisons differ:\n%s" % (len(bad), "\n".join(bad[:16]))
