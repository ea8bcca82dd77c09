"""-m gpu: every kernel route at the edges of the read filter and of the coverage classes, against the C oracle.

Each kernel unpacks FLAG and MAPQ its own way (vector loads taken apart with shifts, `flag << 8 | MAPQ` words, byte and
short buffer loads, plain loads, the device BAM read's two bytes per flag), and drops CIGAR op codes 9-15 through its
own masks.  The records here come from H.edge_reads: MAPQ bytes with the sign bit set and 255, flags over all 16 bits,
every op code, non-consuming ops of 2^28 - 1 bases.  Every route is pinned by the kernel it reports
(gd_stats.tile_kernel), and every route sees the same parameter matrix: one axis at a time (-Q, flag_mask,
min_cov / max_mean_depth, step) against a default for the others."""
import numpy as np
import pytest

from oracle import bamio, pyoracle as po
from tests import helpers as H

pytestmark = pytest.mark.gpu

LENS = (150_001, 9_001)                 # neither a multiple of the 4096-position tile: a clipped last tile each
Q_AXIS = (-1, 0, 1, 127, 128, 129, 255, 256)
COV_AXIS = ((0, 0), (-3, 0), (1, 1), (4, 2), (4, 4), (4, 5), (1, 2 ** 31 - 1), (2 ** 31 - 1, 0), (3, -7))
BASE = dict(Q=1, flag_mask=0x704, min_cov=4, max_mean_depth=0, step=0)


@pytest.fixture(scope="module")
def reads():
    """Contig 0 is sparse enough that its full tiles are ordinary ones for the straight-line kernel (at most 1024
    reads and 1280 ops in a tile's read range); contig 1 is dense: its tiles, like both clipped last tiles, go on
    the slow list."""
    rng = np.random.default_rng(2024)
    return {0: H.edge_reads(rng, LENS[0], 12_000), 1: H.edge_reads(rng, LENS[1], 2_500)}


@pytest.fixture(scope="module")
def oracle(reads):
    return Oracle(reads)


def param_cases(W, bits=True):
    """The default, then one axis at a time."""
    out = [dict(BASE)]
    out += [dict(BASE, Q=q) for q in Q_AXIS if q != BASE["Q"]]
    masks = [m for m in H.EDGE_FLAG_MASKS if m != BASE["flag_mask"]]
    if bits:
        masks += [1 << b for b in range(16) if 1 << b not in masks]
    out += [dict(BASE, Q=0, flag_mask=m) for m in masks]
    out += [dict(BASE, min_cov=a, max_mean_depth=b) for a, b in COV_AXIS]
    out += [dict(BASE, step=s) for s in (W, W * (2 ** 31 // W + 1))]
    return out


def describe(route, W, p, tid):
    return "route %s, W=%d Q=%d flag_mask=%#x min_cov=%d max_mean_depth=%d step=%d, contig %d" % (
        route, W, p["Q"], p["flag_mask"], p["min_cov"], p["max_mean_depth"], p["step"], tid)


def same(got, want, ctx, what, pos_of):
    """Assert equality; the message names the first position that differs."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape == want.shape and np.array_equal(got, want):
        return
    n = min(len(got), len(want))
    neq = np.flatnonzero((got[:n] != want[:n]).reshape(n, -1).any(1))
    k = int(neq[0]) if len(neq) else n
    pytest.fail("%s: %s differ from the oracle first at position %d (entry %d: got %s, want %s; %d vs %d entries)"
                % (ctx, what, pos_of(k, got, want), k, got[k].tolist() if k < len(got) else "-",
                   want[k].tolist() if k < len(want) else "-", len(got), len(want)))


def at_index(k, got, want):
    return k


def run_start(k, got, want):
    return int((want if k < len(want) else got)[k][0])


class Oracle:
    """Per-base depth and W-window (sums, minima) of each contig for each (Q, flag_mask), computed once."""

    def __init__(self, reads):
        self.reads, self.cache, self.wcache = reads, {}, {}

    def depth(self, tid, q, mask):
        key = (tid, q, mask)
        if key not in self.cache:
            self.cache[key] = po.perbase_c(self.reads[tid], q, 0, LENS[tid], flag_mask=mask)
        return self.cache[key]

    def windows(self, tid, q, mask, W):
        key = (tid, q, mask, W)
        if key not in self.wcache:
            self.wcache[key] = H.oracle_windows(self.depth(tid, q, mask), W)
        return self.wcache[key]


def check_case(eng, oracle, route, W, p, mode, expect_tk, regions=None):
    eng.set_params(window_size=W, min_mapq=p["Q"], min_cov=p["min_cov"], max_mean_depth=p["max_mean_depth"],
                   flag_mask=p["flag_mask"], step=p["step"])
    eng.compute()
    st = eng.stats()
    assert st.tile_kernel == expect_tk, "%s: ran kernel %d, expected %d" % (describe(route, W, p, -1), st.tile_kernel,
                                                                           expect_tk)
    step = p["step"] or po.step_for(W)
    for tid, L in enumerate(LENS):
        ctx = describe(route, W, p, tid)
        d = oracle.depth(tid, p["Q"], p["flag_mask"])
        ws, wm = oracle.windows(tid, p["Q"], p["flag_mask"], W)
        wpos = lambda k, g, w: k * W
        if mode == "sums":
            same(eng.window_sums(tid), ws, ctx, "window sums", wpos)
            continue
        if mode == "perbase":
            same(eng.perbase(tid), d, ctx, "per-base depths", at_index)
        sums, mins = eng.windows(tid)
        same(sums, ws, ctx, "window sums", wpos)
        same(mins, wm, ctx, "window minima", wpos)
        same(eng.callable_runs(tid), H.oracle_runs(d, p["min_cov"], p["max_mean_depth"], step), ctx,
             "callable runs", run_start)
    if regions is not None:
        tids, starts, ends = regions
        rs, rm, rr = eng.regions(tids, starts, ends)
        for k, (t, a, b) in enumerate(zip(tids, starts, ends)):
            ctx = describe(route, W, p, t) + ", --bed region %d-%d" % (a, b)
            d = np.zeros(b - a, np.int32)
            hi = min(b, LENS[t])
            if hi > a:
                d[:hi - a] = oracle.depth(t, p["Q"], p["flag_mask"])[a:hi]
            ws, wm = H.oracle_windows(d, W, a)
            wpos = lambda k, g, w, a=a: max(a, (a // W + k) * W)
            same(rs[k], ws, ctx, "region window sums", wpos)
            same(rm[k], wm, ctx, "region window minima", wpos)
            same(rr[k], H.oracle_runs(d, p["min_cov"], p["max_mean_depth"], 1 << 62, a), ctx, "region runs", run_start)
    return st


def some_regions(seed):
    rng = np.random.default_rng(seed)
    tids, starts, ends = [], [], []
    for _ in range(34):
        t = int(rng.integers(0, len(LENS)))
        a = int(rng.integers(0, LENS[t] + 50))
        tids.append(t)
        starts.append(a)
        ends.append(a + int(rng.choice([1, 7, 120, 600, 5000])))
    for t, L in enumerate(LENS):                                   # the clipped last tile and past the contig end
        tids.append(t)
        starts.append(L - 4500)
        ends.append(L + 300)
    return tids, starts, ends


device_arrays = H.device_arrays        # (shared with tests/test_gpu_tile_shapes.py)


ALL4 = ("pos", "flag", "mapq", "off")
# route -> (how the records arrive, device path, outputs, window size, options, expected gd_stats.tile_kernel)
ROUTES = {
    "tile-fast-pushed": ("push", "tile", "perbase", 100, {}, "TK_FAST_RAW"),
    "tile-generic-option": ("push", "tile", "perbase", 100, {"OPT_FAST_KERNEL": 0}, "TK_GENERIC"),
    "tile-misaligned": (ALL4, "tile", "perbase", 100, {}, "TK_GENERIC"),
    "chunk-pushed": ("push", "chunk", "perbase", 100, {}, "TK_LONG"),
    "chunk-misaligned": (ALL4, "chunk", "perbase", 100, {}, "TK_LONG"),
    "scatter": ("push", "scatter", "perbase", 100, {}, "TK_SCATTER"),
    "sums-stream": ("push", "tile", "sums", 100, {}, "TK_SUMS_STREAM_RAW"),
    "sums-misaligned": (ALL4, "tile", "sums", 100, {}, "TK_TILE_SUMS"),
    "sums-w25": ("push", "tile", "sums-windows", 25, {}, "TK_FAST_RAW"),   # W < 32: the regular windows-only kernel
}
ROUTES.update({"tile-misaligned-%s-only" % a: ((a,), "tile", "perbase", 100, {}, "TK_GENERIC") for a in ALL4})


def setup_route(eng, reads, route):
    from goleft_amd import engine as E
    how, path, mode, W, opts, _ = ROUTES[route]
    eng.set_path({"tile": E.PATH_TILE, "chunk": E.PATH_CHUNK, "scatter": E.PATH_SCATTER}[path])
    eng.set_outputs(perbase=mode == "perbase", sums_only=mode.startswith("sums"))
    for k, v in opts.items():
        eng.set_option(getattr(E, k), v)
    eng.set_params(window_size=W)
    eng.set_contigs(LENS)
    for tid, r in reads.items():
        if how == "push":
            eng.push(tid, r.pos, r.flag, r.mapq, r.cigar_off, r.cigar)
        else:
            eng.adopt_device(tid, *device_arrays(r, how))


@pytest.mark.parametrize("route", list(ROUTES))
def test_route_matches_oracle_at_filter_and_class_edges(reads, oracle, route):
    from goleft_amd import engine as E
    from goleft_amd.engine import DepthEngine
    how, path, mode, W, _, tk = ROUTES[route]
    single = route.endswith("-only")          # the single-misaligned-array routes: the filter axes, no single bits
    cases = param_cases(W, bits=not single)
    if single:
        cases = [p for p in cases if p["min_cov"] == BASE["min_cov"] and p["step"] == BASE["step"]]
    regions = some_regions(5) if mode == "perbase" and not single else None
    want_path = {"tile": E.PATH_TILE, "chunk": E.PATH_CHUNK, "scatter": E.PATH_SCATTER}[path]
    with DepthEngine(0) as eng:
        setup_route(eng, reads, route)
        for i, p in enumerate(cases):
            st = check_case(eng, oracle, route, W, p, mode, getattr(E, tk), regions)
            assert st.path == want_path, "%s: path %d" % (describe(route, W, p, -1), st.path)
            if i == 0 and tk == "TK_FAST_RAW" and mode == "perbase":
                # both kernels of the route did work: most tiles ran the straight-line kernel, a few the slow one
                assert 0 < st.n_slow_tiles <= st.n_tiles // 4, "route %s: %d of %d tiles on the slow list" % (
                    route, st.n_slow_tiles, st.n_tiles)


# ---- the BAM decoders and the CLI on the same records ---------------------------------------------------------------

@pytest.fixture(scope="module")
def edge_bam(tmp_path_factory):
    """The edge records written as BAM files -- one read of 70 000 ops (CG tag) with every op code among them --
    once with a .bai (the device decodes) and once without (the host decodes)."""
    rng = np.random.default_rng(77)
    lens = (120_001, 6_001)
    contigs = [("e0", lens[0]), ("e1", lens[1])]
    reads = {0: H.edge_reads(rng, lens[0], 24_000, long_ops=70_000), 1: H.edge_reads(rng, lens[1], 1_500)}
    d = tmp_path_factory.mktemp("edgebam")
    idx, plain = d / "idx", d / "plain"
    idx.mkdir()
    plain.mkdir()
    bamio.write_bam(str(idx / "e.bam"), contigs, reads, unplaced=2, index=True)
    bamio.write_bam(str(plain / "e.bam"), contigs, reads, unplaced=2)
    for sub in (idx, plain):
        (sub / "e.fa.fai").write_text("".join("%s\t%d\t6\t60\t61\n" % c for c in contigs))
    _, back, rb, _ = bamio.read_bam(str(idx / "e.bam"))
    assert back == contigs
    assert int(np.diff(rb[0].cigar_off.astype(np.int64)).max()) == 70_000
    for t in reads:
        for f in ("pos", "flag", "mapq", "cigar_off", "cigar"):
            assert np.array_equal(getattr(rb[t], f), getattr(reads[t], f)), (t, f)
    return contigs, reads, idx, plain


def test_device_bam_decoder_keeps_every_flag_bit_and_mapq_byte(edge_bam):
    """gd_ingest_bgzf on the indexed file, then one compute per flag bit (flag_mask = 1 << b) and per MAPQ edge:
    each flag bit and each MAPQ byte must have been decoded exactly as written."""
    from goleft_amd.engine import DepthEngine
    from tests.test_gpu_bamdecode import ingest_contig
    contigs, reads, idx, _ = edge_bam
    path = str(idx / "e.bam")
    cases = [(0, 1 << b) for b in range(16)] + [(q, 0) for q in H.EDGE_MAPQ + (256,)] + [(1, 0x704)]
    with DepthEngine(0) as eng:
        eng.set_params(window_size=100, min_mapq=0, flag_mask=0)
        eng.set_contigs([c[1] for c in contigs])
        for tid in range(len(contigs)):
            assert ingest_contig(eng, path, tid) == reads[tid].n
        for q, m in cases:
            eng.set_params(window_size=100, min_mapq=q, min_cov=4, flag_mask=m)
            eng.compute()
            for tid, (_, L) in enumerate(contigs):
                ctx = "device BAM decode, Q=%d flag_mask=%#x, contig %d" % (q, m, tid)
                same(eng.perbase(tid), po.perbase_c(reads[tid], q, 0, L, flag_mask=m), ctx, "per-base depths",
                     at_index)


@pytest.mark.parametrize("Q", [0, 128, 255])
@pytest.mark.parametrize("decoder", ["device", "host"])
def test_cli_beds_at_mapq_edges(edge_bam, decoder, Q):
    """`goleft depth -Q {0,128,255}` on the edge records: .depth.bed and .callable.bed byte for byte the oracle's,
    read through the device decoder (indexed file) and through the host decoder (no index)."""
    from goleft_amd import depth
    contigs, reads, idx, plain = edge_bam
    d = idx if decoder == "device" else plain
    prefix = d / ("q%d" % Q)
    rc = depth.Main([str(a) for a in ["-Q", Q, "--ordered", "--windowsize", 250, "--prefix", prefix,
                                      "--reference", d / "e.fa", d / "e.bam"]])
    assert rc == 0
    hd, ca = po.depth_run_oracle(contigs, reads, W=250, Q=Q, mincov=4)
    got_hd, got_ca = open("%s.depth.bed" % prefix).read(), open("%s.callable.bed" % prefix).read()
    for what, got, want in (("depth.bed", got_hd, hd), ("callable.bed", got_ca, ca)):
        if got != want:
            g, w = got.splitlines(), want.splitlines()
            k = next((i for i, (a, b) in enumerate(zip(g, w)) if a != b), min(len(g), len(w)))
            pytest.fail("%s decoder, -Q %d: %s differs first at row %d: got %r, want %r"
                        % (decoder, Q, what, k, g[k] if k < len(g) else None, w[k] if k < len(w) else None))
