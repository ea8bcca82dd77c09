"""-m gpu: the multidepth kernels at their structural edges -- the run look-around across word boundaries, the contig's
end, z0 / E / the flush test at their off-by-ones, splitBlocks, more than 256 chunks, more than one workgroup of words
and of (chunk, run) pairs, the three-launch scan behind each of ps / prs / pre / nblk, the flag kernels at every
remainder of the sample loop and of the last word, the sums kernel at chosen word bounds, and the ABI's refusals.
The shapes come from tests/md_shapes.py; tests/test_md_shapes.py shows on the CPU that each one sits on its edge.

Blocks must equal the oracle's (oracle/pyoracle.py::multidepth_py) as integers, bitmaps numpy's bit for bit, sums the
sequential loop's doubles with ==.  No tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

from oracle import bamio, pyoracle as po
from tests import helpers as H
from tests import md_shapes as M

pytestmark = pytest.mark.gpu

GD_E_INVALID, GD_E_STATE, GD_E_RANGE, GD_E_CAPACITY = -1, -4, -5, -8


def differs(got, want, ctx):
    """None when the device's blocks equal the oracle's; else a message with the first block that differs."""
    d = M.first_difference(got, want)
    if d is None:
        return None
    return "%s: block %d: device %s, oracle %s (%d against %d blocks)" % (ctx, d[0], d[1], d[2], len(got), len(want))


def device_blocks(eng, c):
    eng.md_load_flags(c.any, c.suf)
    return eng.md_blocks(*c.params)


@pytest.mark.parametrize("name", M.NAMES)
def test_block_finder_at_structural_edges(name):
    from goleft_amd.engine import DepthEngine
    c = M.case(name)
    want = M.oracle_blocks(name)
    with DepthEngine(0) as eng:
        got = device_blocks(eng, c)
    bad = differs(got, want, "case %s (chunk %d, max_skip %d, min_size %d, window %d)" % ((name,) + c.params))
    assert not bad, bad


@pytest.mark.parametrize("name", M.HOSTLIB_NAMES)
def test_block_finder_through_the_host_library(name):
    from goleft_amd import _hostlib as hl
    c = M.case(name)
    got = hl.multidepth_blocks(c.any, c.suf, *c.params)
    bad = differs(got, M.oracle_blocks(name), "case %s, gdh_multidepth_blocks" % name)
    assert not bad, bad


def test_one_engine_long_short_long():
    """The bitmap and scan buffers only grow, and the suf words sit at d_md_bits + nw of the CURRENT load: a long
    contig, a short one and the long one again on one engine give what fresh engines give."""
    from goleft_amd.engine import DepthEngine
    longest = max(M.NAMES, key=lambda n: len(M.case(n).any))
    order = (longest, "last-site-L1", "last-site-L31", "streams-to-contig-end", longest)
    assert len(M.case("last-site-L1").any) == min(len(M.case(n).any) for n in M.NAMES)
    fresh = {}
    for name in set(order):
        with DepthEngine(0) as eng:
            fresh[name] = device_blocks(eng, M.case(name))
    with DepthEngine(0) as eng:
        for k, name in enumerate(order):
            got = device_blocks(eng, M.case(name))
            bad = differs(got, fresh[name], "step %d, case %s, used engine against a fresh one" % (k, name)) or \
                differs(got, M.oracle_blocks(name), "step %d, case %s, used engine" % (k, name))
            assert not bad, bad


@pytest.fixture(scope="module", params=M.FLAG_S)
def samples(request):
    """One engine whose contigs are the S samples of every length of M.FLAG_L, computed once; with the oracle's
    per-base depths."""
    from goleft_amd.engine import DepthEngine
    S, Q = request.param, 5
    eng = DepthEngine(0)
    eng.set_params(window_size=100, min_mapq=Q, min_cov=4)
    eng.set_contigs([L for L in M.FLAG_L for _ in range(S)])
    depth = {}
    for li, L in enumerate(M.FLAG_L):
        streams = M.flag_reads(S, L)
        for s, r in enumerate(streams):
            eng.push(li * S + s, r.pos, r.flag, r.mapq, r.cigar_off, r.cigar)
        depth[L] = np.stack([po.perbase_c(r, Q, 0, L) for r in streams])
        depth[L].setflags(write=False)
    eng.compute()
    yield S, eng, depth
    eng.close()


def flags_of(D, min_cov, min_samples):
    return (D > 0).any(0), (D >= min_cov).sum(0) > min_samples


def test_flags_and_sums_at_word_and_sample_edges(samples):
    S, eng, depth = samples
    for li, L in enumerate(M.FLAG_L):
        D = depth[L]
        tids = list(range(li * S, (li + 1) * S))
        assert not (D > 0).any(0).all(), "some position is covered by no sample"
        for min_cov in M.FLAG_MIN_COV:
            for ms in M.flag_min_samples(S):
                ctx = "S %d, L %d, min_cov %d, min_samples %d" % (S, L, min_cov, ms)
                want_any, want_suf = flags_of(D, min_cov, ms)
                if ms == -1:
                    assert want_suf.all()
                if ms == S:
                    assert not want_suf.any()
                any_, suf = eng.md_flags(tids, min_cov, ms)
                assert np.array_equal(any_, want_any) and np.array_equal(suf, want_suf), ctx
                blocks = M.sums_blocks(L, want_suf)
                st, en = np.array([b[0] for b in blocks]), np.array([b[1] for b in blocks])
                want = M.sums_reference(D, want_suf, blocks)
                got = eng.md_sums(st, en, S)
                assert got.shape == want.shape and (got == want).all(), (ctx, np.argwhere(got != want)[:3].tolist())
                # one sample: n_blocks * n_samples = 63, 64, 65 cells, a wave of the sums kernel and one cell either side
                for n in (63, 64, 65):
                    k = np.arange(n) % len(blocks)
                    one = eng.md_sums_group([tids[S - 1]], st[k], en[k])
                    assert one.shape == (n, 1) and (one[:, 0] == want[k, S - 1]).all(), (ctx, n)
                # groups over the resident samples: gd_md_acc_kernel / gd_md_finish_kernel
                for size in M.FLAG_GROUPS.get(S, ()):
                    groups = [tids[g:g + size] for g in range(0, S, size)]
                    eng.md_begin(L)
                    for g in groups:
                        eng.md_accumulate(g, min_cov)
                    any_g, suf_g = eng.md_finish(ms)
                    assert np.array_equal(any_g, want_any) and np.array_equal(suf_g, want_suf), (ctx, size)
                    for g in groups:
                        got_g = eng.md_sums_group(g, st, en)
                        cols = [t - tids[0] for t in g]
                        assert (got_g == want[:, cols]).all(), (ctx, size, g)


def test_flags_in_groups_with_one_group_resident(samples):
    """The documented way: only the group's contigs are selected and computed when it is accumulated or summed."""
    S, eng, depth = samples
    try:
        for li, L in enumerate(M.FLAG_L):
            D = depth[L]
            tids = list(range(li * S, (li + 1) * S))
            groups = [tids[g:g + 3] for g in range(0, S, 3)]
            for min_cov in M.FLAG_MIN_COV:
                eng.md_begin(L)
                for g in groups:
                    eng.select_contigs(g)
                    eng.compute()
                    eng.md_accumulate(g, min_cov)
                for ms in M.flag_min_samples(S):                   # the accumulators stay: one finish per threshold
                    want_any, want_suf = flags_of(D, min_cov, ms)
                    any_g, suf_g = eng.md_finish(ms)
                    assert np.array_equal(any_g, want_any) and np.array_equal(suf_g, want_suf), (S, L, min_cov, ms)
            any_g, suf_g = eng.md_finish(0)                          # min_cov 1, min_samples 0
            blocks = M.sums_blocks(L, suf_g)
            st, en = np.array([b[0] for b in blocks]), np.array([b[1] for b in blocks])
            want = M.sums_reference(D, suf_g, blocks)
            for g in groups:
                eng.select_contigs(g)
                eng.compute()
                got = eng.md_sums_group(g, st, en)
                assert (got == want[:, [t - tids[0] for t in g]]).all(), (S, L, g)
    finally:
        eng.select_contigs([])
        eng.compute()


def test_abi_refusals_leave_the_context_usable():
    from goleft_amd.engine import DepthEngine
    small = M.case("split-in-three")
    want = M.oracle_blocks("split-in-three")
    n = C.c_size_t(77)

    def blocks(eng, chunk, max_skip, starts=None, ends=None, cap=0):
        return eng._lib.gd_md_blocks(eng._ctx, chunk, max_skip, small.min_size, small.window,
                                     starts.ctypes.data if starts is not None else None,
                                     ends.ctypes.data if ends is not None else None, cap, C.byref(n))

    def still_right(eng, what):
        bad = differs(device_blocks(eng, small), want, "after %s" % what)
        assert not bad, bad

    with DepthEngine(0) as eng:
        assert blocks(eng, small.chunk, small.max_skip) == GD_E_STATE and n.value == 0      # no bitmaps yet
        still_right(eng, "GD_E_STATE")
        assert blocks(eng, 0, small.max_skip) == GD_E_INVALID
        still_right(eng, "chunk 0")
        assert blocks(eng, small.chunk, -1) == GD_E_INVALID
        still_right(eng, "max_skip -1")
        L = (1 << 20) + 1
        a = np.zeros(L, bool)
        a[::5] = True
        eng.md_load_flags(a, np.zeros(L, bool))
        assert blocks(eng, 1, small.max_skip) == GD_E_RANGE                                  # 2^20 + 1 chunks
        assert blocks(eng, 2, small.max_skip) == 0 and n.value == 0
        still_right(eng, "GD_E_RANGE")
        assert len(want) >= 2
        st, en = np.full(len(want), -7, np.int64), np.full(len(want), -7, np.int64)
        eng.md_load_flags(small.any, small.suf)
        assert blocks(eng, small.chunk, small.max_skip, st, en, len(want) - 1) == GD_E_CAPACITY
        assert n.value == len(want) and (st == -7).all() and (en == -7).all()               # the true count, nothing written
        assert blocks(eng, small.chunk, small.max_skip, st, en, len(want)) == 0 and n.value == len(want)
        assert [tuple(b) for b in np.stack([st, en], 1).tolist()] == list(want)
        still_right(eng, "GD_E_CAPACITY")


@pytest.mark.parametrize("opt", [("--mincov", 0), ("--minsamples", 1.0)])
def test_cli_at_the_ends_of_its_thresholds(tmp_path, opt):
    """--mincov 0: every printed site is sufficient, no insufficient site ever opens a stream: the header only.
    --minsamples 1.0: more than all samples would have to reach mincov."""
    from goleft_amd import multidepth
    contigs, reads, _ = H.load_golden_bam("t")
    rng = np.random.default_rng(12)
    paths, thinned = [], []
    for s, frac in enumerate([1.0, 0.4]):
        sub = {}
        for tid, r in reads.items():
            keep = np.flatnonzero(rng.random(r.n) < frac)
            off = np.zeros(len(keep) + 1, np.uint32)
            off[1:] = np.cumsum((r.cigar_off[keep + 1] - r.cigar_off[keep]).astype(np.uint32))
            cig = np.concatenate([r.cigar[int(r.cigar_off[i]):int(r.cigar_off[i + 1])] for i in keep]) \
                if len(keep) else np.zeros(0, np.uint32)
            sub[tid] = po.Reads(r.pos[keep], r.flag[keep], r.mapq[keep], off, cig.astype(np.uint32))
        p = str(tmp_path / ("s%d.bam" % s))
        bamio.write_bam(p, contigs, sub, index=(s == 0))
        paths.append(p)
        thinned.append(sub)
    chrom, q = "chrM", 10
    tid = [c[0] for c in contigs].index(chrom)
    L = contigs[tid][1]
    D = [po.perbase_c(t[tid], q, 0, L) if tid in t else np.zeros(L, np.int32) for t in thinned]
    kw = dict(mincov=7, maxskip=10, minsize=15, window=10000000, min_samples=0.5)
    kw[{"--mincov": "mincov", "--minsamples": "min_samples"}[opt[0]]] = opt[1]
    want = ["#chrom\tstart\tend\ts0\ts1"] + po.multidepth_py(chrom, D, **kw)
    assert po.multidepth_py(chrom, D, mincov=7) and len(want) == 1        # blocks at the defaults, none at the extreme
    out = str(tmp_path / "md.txt")
    argv = ["-c", chrom, "-Q", q, "--mincov", kw["mincov"], "-k", kw["maxskip"], "-m", kw["minsize"], "-w", kw["window"],
            "--minsamples", kw["min_samples"]] + paths
    assert multidepth.Main(argv, out) == 0
    assert open(out).read().splitlines() == want
