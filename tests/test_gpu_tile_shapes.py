"""-m gpu: the short-read tile kernels at their structural edges -- the prep kernel's ordinary-tile rule (1024 reads,
1280 ops, the rounding of lo), the straight-line kernel's inline interval, its 120-entry queue and its three window
paths, the one-ballot any_noisy shortcut, the generic kernel's batches and per-wave queue, phase C's groups of 1024
tiles, the read-back's 4096 boundaries and the boundary list's growth.  The shapes come from tests/tile_shapes.py;
tests/test_tile_shapes.py shows on the CPU that each one reaches its edge.

Every case runs through the C ABI on every tile route -- the window, class and phase C shapes also on the long-read tile
kernel, which instantiates the same phase B / C code with its own LDS layout and carry -- and is compared with the C oracle, exactly: the whole per-base
vector where the route keeps one, window sums and minima, the class runs of every contig, and for one case per family
--bed regions around the crafted positions.  gd_stats says which kernel ran; n_slow_tiles, n_tiles, n_runs, reruns,
lookback and max_span_seen are held against the routing model.  Every case is computed twice on its context (the
alternating slow-tile counters, a raised or a tightened look-back, a grown boundary list): no result may change."""
import numpy as np
import pytest

from tests import helpers as H
from tests import tile_shapes as TS

pytestmark = pytest.mark.gpu

# route -> (records arrive by, per-base vector kept, sums only, options, gd_stats.tile_kernel)
ROUTES = {
    "fast": ("push", True, False, {}, "TK_FAST_RAW"),                        # gd_tile_fast_kernel<1> + gd_tile_slow_kernel
    "fast-windows": ("push", False, False, {}, "TK_FAST_RAW"),               # gd_tile_fast_kernel<2>: no per-base stores
    "generic": ("push", True, False, {"OPT_FAST_KERNEL": 0}, "TK_GENERIC"),  # gd_tile_kernel for every tile
    "generic-misaligned": (("pos",), True, False, {}, "TK_GENERIC"),         # `pos` at element offset 1 of its tensor
    "tile-sums": (("pos",), False, True, {}, "TK_TILE_SUMS"),                # gd_tile_sums_kernel (window cases, W >= 32)
    "long": ("push", True, False, {"path": "PATH_CHUNK"}, "TK_LONG"),        # gd_ltile2_kernel<1>: the same phase B / C code
    "long-windows": ("push", False, False, {"path": "PATH_CHUNK"}, "TK_LONG"),   # gd_ltile2_kernel<2>: no per-base stores
}
LONG_FAMILIES = ("windows", "classes", "phase-c", "phase-c-large")


def long_stats(c):
    """(lookback, max_span_seen) of a case on the long-read path: the largest span of ALL reads with ops (the filter is
    applied per tile), rounded up to 64 and at least 64; the hint does not matter."""
    span = max([int(H.ref_span(c.get(t)).max()) for t in range(len(c.lengths)) if c.lengths[t] > 0 and c.get(t).n] + [0])
    return max(64, (span + 63) & ~63), span


def first_diff(got, want):
    n = min(len(got), len(want))
    neq = np.flatnonzero((got[:n] != want[:n]).reshape(n, -1).any(1))
    return int(neq[0]) if len(neq) else n


def same(got, want, ctx, what, pos_of):
    """None when equal; else a message that names the case, the route and the first position that differs."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape == want.shape and np.array_equal(got, want):
        return None
    k = first_diff(got, want)
    return "%s: %s differ from the oracle first at position %d (entry %d: got %s, want %s; %d vs %d entries)" % (
        ctx, what, pos_of(k, got, want), k, got[k].tolist() if k < len(got) else "-",
        want[k].tolist() if k < len(want) else "-", len(got), len(want))


def run_start(k, got, want):
    return int((want if k < len(want) else got)[k][0])


def regions_of(c):
    """A few --bed regions that straddle the positions a case is about (tile, quarter and contig edges otherwise)."""
    L = c.lengths[0]
    at = [c.mark[k] for k in ("t0", "empty", "filtered") if k in c.mark] or [TS.T]
    pts = sorted({p for a in at for p in (a, a + TS.CHUNK, a + TS.T)} | {0, L})
    out = []
    for p in pts:
        for a, b in ((p - 7, p + 9), (p - 300, p + 1), (p, p + 1), (p - 1, p)):
            if 0 <= a < b and a < L:
                out.append((0, a, b))
    return out[:24]


def configure(eng, c, route):
    from goleft_amd import engine as E
    how, perbase, sums_only, opts, _ = ROUTES[route]
    eng.set_path(getattr(E, opts.get("path", "PATH_TILE")))
    eng.set_outputs(perbase=perbase, sums_only=sums_only)
    eng.set_option(E.OPT_FAST_KERNEL, opts.get("OPT_FAST_KERNEL", 1))
    eng.set_option(E.OPT_INGEST_INDEX, int(c.index))
    eng.set_params(window_size=c.W, min_mapq=c.Q, min_cov=c.min_cov, max_mean_depth=c.max_mean_depth, flag_mask=c.flag_mask,
                   max_span_hint=c.hint, step=c.step)
    eng.set_contigs(c.lengths)
    for tid, r in c.reads.items():
        if how == "push":
            eng.push(tid, r.pos, r.flag, r.mapq, r.cigar_off, r.cigar)
        else:
            eng.adopt_device(tid, *H.device_arrays(r, how))


def check(eng, c, route, attempt, with_regions):
    """One compute of a configured case against the oracle and the model -> list of messages (empty: all equal)."""
    from goleft_amd import engine as E
    _, perbase, sums_only, _, tk = ROUTES[route]
    eng.compute()
    st = eng.stats()
    ctx0 = "case %s (%s), route %s, compute %d" % (c.name, c.edge, route, attempt)
    bad = []
    if st.tile_kernel != getattr(E, tk):
        return ["%s: ran kernel %s, expected %s" % (ctx0, E.TK_NAMES[st.tile_kernel], tk)]
    orc = TS.oracle(c.name)
    for t, L in enumerate(c.lengths):
        ctx = "%s, contig %d" % (ctx0, t)
        d, ws, wm, runs = orc[t]
        wpos = lambda k, g, w: k * c.W
        if sums_only:
            bad.append(same(eng.window_sums(t), ws, ctx, "window sums", wpos))
            continue
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
            d[:hi - a] = orc[t][0][a:hi]
            ws, wm = H.oracle_windows(d, c.W, a)
            wpos = lambda k, g, w, a=a: max(a, (a // c.W + k) * c.W)
            bad.append(same(rs[k], ws, ctx, "region window sums", wpos))
            bad.append(same(rm[k], wm, ctx, "region window minima", wpos))
            bad.append(same(rr[k], H.oracle_runs(d, c.min_cov, c.max_mean_depth, 1 << 62, a), ctx, "region runs", run_start))
    # the routing model
    lookback, lb_reruns, span = TS.lookback_of(c, attempt)
    if route.startswith("long"):
        (lookback, span), lb_reruns = long_stats(c), 0
    want = dict(n_tiles=c.n_tiles, lookback=lookback, max_span_seen=span)
    if not sums_only:
        want["n_runs"] = TS.boundaries(c)[0]
    # a re-run happens once: the raised look-back and the grown boundary list stay with the context
    want["reruns"] = (lb_reruns + (TS.capacity_reruns(c) if c.fresh and not sums_only else 0)) if attempt == 1 else 0
    if route.startswith("fast"):
        want["n_slow_tiles"] = TS.n_slow(c)
    for k, v in want.items():
        if getattr(st, k) != v:
            bad.append("%s: gd_stats.%s is %d, the model says %d" % (ctx0, k, getattr(st, k), v))
    return [b for b in bad if b]


def cases_for(family, route):
    out = [TS.case(n) for n in TS.names(family)]
    if route == "tile-sums":
        out = [c for c in out if c.W >= 32]
    return out


# (the sums-only tile kernel runs the window cases only)
# ... and the long-read tile kernel the families that are about phase B and phase C
PAIRS = [(f, r) for f in TS.FAMILIES for r in ROUTES
         if (f == "windows" if r == "tile-sums" else f in LONG_FAMILIES if r.startswith("long") else True)]


@pytest.mark.parametrize("family,route", PAIRS)
def test_tile_kernels_at_structural_edges(family, route):
    from goleft_amd.engine import DepthEngine
    bad, eng = [], None
    try:
        for i, c in enumerate(cases_for(family, route)):
            if eng is None or c.fresh:                     # one context per route, shared by the cases that can
                if eng is not None:
                    eng.close()
                eng = DepthEngine(0)
            configure(eng, c, route)
            for attempt in (1, 2):
                bad += check(eng, c, route, attempt, with_regions=i == 0 and attempt == 1)
            if c.fresh:
                eng.close()
                eng = None
    finally:
        if eng is not None:
            eng.close()
    assert not bad, "%d comparisons differ:\n%s" % (len(bad), "\n".join(bad[:16]))
