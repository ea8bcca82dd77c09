"""The shapes of tests/md_shapes.py, on the CPU: the model of the device's set form equals the oracle's sequential
restatement on every case, every case kills the mutants it names and reaches the figure it is named for, and the
constants the model restates are the kernels'.  A case that does not demonstrably sit on its edge fails here -- a device
test on these shapes would pass for the wrong reason otherwise.  Exact integer equality throughout."""
import numpy as np
import pytest

from tests import md_shapes as M


def pairs_of(r, chunk):
    return [p for p in r.pairs if p.chunk == chunk]


@pytest.mark.parametrize("name", M.NAMES)
def test_model_equals_oracle(name):
    c = M.case(name)
    assert c.any.shape == c.suf.shape and not (c.suf & ~c.any).any(), "suf is a subset of any"
    want = M.oracle_blocks(name)
    r = M.modelled(name)
    d = M.first_difference(r.blocks, want)
    assert d is None, "case %s: block %d: model %s, oracle %s (%d against %d blocks)" % ((name,) + d + (len(r.blocks), len(want)))
    assert r.n_blocks == len(want) and r.nw == (len(c.any) + 31) // 32
    assert r.n_chunks == -(-len(c.any) // c.chunk) <= M.MAX_CHUNKS


@pytest.mark.parametrize("name,mutant", [(n, m) for n in M.NAMES for m in M.case(n).kills])
def test_case_kills_its_mutants(name, mutant):
    """A condition on the case: the wrong variant of the decision it is named for gives other blocks."""
    want = M.oracle_blocks(name)
    got = M.modelled(name, mutant).blocks
    assert M.first_difference(got, want) is not None, "case %s does not notice `%s` (%s)" % (name, mutant, M.MUTANTS[mutant])


def test_every_mutant_is_killed_by_a_case_that_names_it():
    named = {m for n in M.NAMES for m in M.case(n).kills}
    assert named == set(M.MUTANTS), sorted(set(M.MUTANTS) - named)
    required = ("no_word_crossing", "gap_ge", "past_chunk_off", "end_lookback_off", "no_z0_clamp", "flush_off", "E_flushes",
                "minsize_unclipped", "window_le", "chunks_256", "scan_block0:ps", "scan_block0:prs", "scan_block0:pre",
                "scan_block0:nblk", "tail_bits", "last_of_chunk")
    assert set(required) <= named


def test_model_constants_are_the_kernels():
    """The model restates the kernels' constants; the sources' are read from their text."""
    k = M.kernel_constants()
    assert set(k["threads"].values()) == {M.THREADS}
    assert k["chunk_stride"] == k["word_stride"] == k["pair_stride"] == M.THREADS
    assert k["scan_block"] == M.SCAN_BLOCK == k["scan_block_threads"] * k["scan_per_thread"]
    assert k["scan_switch_blocks"] * k["scan_block"] == M.SCAN_SWITCH == 16384
    assert k["unit_threads"] == k["unit_launch"] == M.SCAN_THREADS and k["unit_per"] == (M.SCAN_THREADS - 1, M.SCAN_THREADS)
    assert 1 << k["max_chunks_log2"] == M.MAX_CHUNKS


def test_fuzz_model_against_oracle():
    """Small inputs with small parameters, so that the edges collide often: the derivation of the set form does not
    rest on the named cases alone."""
    rng = np.random.default_rng(20240)
    n_blocks = n_multi = 0
    for it in range(3000):
        L = int(rng.integers(1, 301))
        kind = it % 4
        if kind == 0:                                               # dense
            cls = rng.choice(3, L, p=[0.15, 0.25, 0.6])
        elif kind == 1:                                             # sparse
            cls = rng.choice(3, L, p=[0.7, 0.1, 0.2])
        elif kind == 2:                                             # stretches
            cls = np.repeat(rng.choice(3, L), rng.integers(1, 6, L))[:L]
        else:
            cls = rng.choice(3, L, p=[0.4, 0.3, 0.3])
        any_, suf = cls > 0, cls == 2
        chunk, max_skip = int(rng.integers(1, 41)), int(rng.integers(0, 4))
        min_size, window = int(rng.integers(1, 5)), int(rng.integers(1, 9))
        want = M.oracle_blocks_of(any_, suf, chunk, max_skip, min_size, window)
        got = M.model(any_, suf, chunk, max_skip, min_size, window)
        d = M.first_difference(got.blocks, want)
        assert d is None, (it, L, chunk, max_skip, min_size, window, d, np.flatnonzero(suf).tolist(),
                           np.flatnonzero(any_ & ~suf).tolist())
        n_blocks += len(want)
        n_multi += got.n_chunks > 1 and got.n_pairs > got.n_runs
    assert n_blocks > 10000 and n_multi > 300


# ---- each case reaches its edge -------------------------------------------------------------------------------------

def test_word_edge_cases():
    r = M.modelled("word-bit31-bit0-skip0")
    assert M.case("word-bit31-bit0-skip0").max_skip == 0 and (r.starts, r.ends) == ([31], [32])
    for ms in (1, 31, 32, 33, 70, 100):
        c, r = M.case("word-straddle-skip%d" % ms), M.modelled("word-straddle-skip%d" % ms)
        assert c.max_skip == ms and r.n_runs == 3
        a, b = r.starts[0], r.ends[0]
        assert a & 31 == 31 and b - a - 1 == ms and not c.suf[a + 1:b].any()           # gap exactly max_skip: one run
        assert r.starts[1] & 31 == 31 and r.starts[1] == r.ends[1] and r.starts[2] - r.ends[1] - 1 == ms + 1
        if ms >= 70:
            assert (b >> 5) - (a >> 5) >= 3                                             # two or more empty words between
    for ms in (1, 5):
        r = M.modelled("word-inside-skip%d" % ms)
        assert r.n_runs == 3 and r.starts[0] >> 5 == r.ends[0] >> 5 and r.ends[0] - r.starts[0] - 1 == ms
        assert r.ends[1] >> 5 == r.starts[2] >> 5 and r.starts[2] - r.ends[1] - 1 == ms + 1


def test_contig_end_cases():
    r = M.modelled("run-from-0")
    assert r.starts[0] == 0 and r.chunks[0]["z0"] == 2 and r.pairs[0].s == 3 and r.pairs[0].n_blocks == 0
    assert M.modelled("last-site-L1").n_runs == 1 and M.modelled("last-site-L1").blocks == []
    for L in (31, 32, 33, 64, 65):
        c, r = M.case("last-site-L%d" % L), M.modelled("last-site-L%d" % L)
        assert len(c.any) == L and c.suf[L - 1] and r.blocks == [(L - 1, L)]
    c, r = M.case("end-lookahead-cut"), M.modelled("end-lookahead-cut")
    assert r.ends[-1] + c.max_skip + 2 > len(c.any) > r.ends[-1] + 1
    c, r = M.case("flushing-site-at-L-1"), M.modelled("flushing-site-at-L-1")
    p = r.pairs[-1]
    assert r.chunks[0]["pa"] == len(c.any) - 1 == p.e + c.max_skip + 2 and p.last and p.flushed
    assert p.count == c.min_size - 1 and r.blocks == []


def test_z0_cases():
    c, r = M.case("z0-at-chunk-start"), M.modelled("z0-at-chunk-start")
    assert r.chunks[1]["z0"] == c.chunk and r.chunks[1]["n_pairs"] > 0
    c, r = M.case("z0-in-previous-chunk"), M.modelled("z0-in-previous-chunk")
    assert r.chunks[0]["z0"] == c.chunk - 1 and r.chunks[1]["z0"] > c.chunk and c.suf[c.chunk + 1]
    r = M.modelled("no-insufficient-site")
    assert r.n_runs == 1 and r.n_pairs == 0 and r.blocks == []
    c, r = M.case("z0-past-chunk-inside-run"), M.modelled("z0-past-chunk-inside-run")
    ch = r.chunks[0]
    assert ch["z0"] > c.chunk + 1 and ch["E"] == ch["z0"] and r.starts[0] < ch["z0"] < r.ends[0]
    assert [p.n_blocks for p in pairs_of(r, 0)] == [0] and r.n_blocks > 0             # a pair that yields no block


def test_E_cases():
    c, r = M.case("E-at-i+1+chunk"), M.modelled("E-at-i+1+chunk")
    n = c.any & ~c.suf
    assert n[c.chunk + 1] and r.chunks[0]["E"] > c.chunk + 2
    c, r = M.case("E-at-i+2+chunk"), M.modelled("E-at-i+2+chunk")
    assert not (c.any & ~c.suf)[1:c.chunk + 2].any() and r.chunks[0]["E"] == c.chunk + 2
    for name, back, ends in (("E-lookback-continues", 2, False), ("E-lookback-ends", 3, True),
                             ("E-skip1-ends-at-once", 1, True), ("E-skip0-ends-at-once", 1, True)):
        c, r = M.case(name), M.modelled(name)
        p = 20
        assert (c.any & ~c.suf)[p] and p > c.chunk + 1 and c.suf[p - back] and not c.suf[p - back + 1:p].any()
        assert back == (c.max_skip - 1 if not ends else max(c.max_skip, 1))
        assert (r.chunks[0]["E"] == p) == ends and (ends or r.chunks[0]["E"] == len(c.any))
    c, r = M.case("E-site-before-far-z0"), M.modelled("E-site-before-far-z0")
    ch = r.chunks[0]
    assert ch["z0"] == ch["E"] > c.chunk + 1 and c.suf[ch["z0"] - 2] and ch["z0"] - 2 > ch["z0"] - c.max_skip


def test_flush_and_min_size_cases():
    c, r = M.case("flushed-min-size-exact"), M.modelled("flushed-min-size-exact")
    assert [(p.count, p.flushed, p.n_blocks) for p in r.pairs] == [(c.min_size, True, 1), (c.min_size - 1, True, 0),
                                                                     (c.min_size, False, 1)]
    c, r = M.case("unflushed-short-last-run"), M.modelled("unflushed-short-last-run")
    p = r.pairs[-1]
    assert p.last and not p.flushed and p.count < c.min_size and p.n_blocks == 1
    c, r = M.case("later-site-at-e+skip+2"), M.modelled("later-site-at-e+skip+2")
    p = r.pairs[-1]
    assert r.chunks[0]["pa"] == p.e + c.max_skip + 2 and p.flushed and p.count < c.min_size and p.n_blocks == 0
    c, r = M.case("later-site-at-e+skip+1"), M.modelled("later-site-at-e+skip+1")
    p = r.pairs[-1]
    assert r.chunks[0]["pa"] == p.e + c.max_skip + 1 and not p.flushed and p.n_blocks == 1
    c, r = M.case("far-site-is-E"), M.modelled("far-site-is-E")
    p = pairs_of(r, 0)[-1]
    assert r.chunks[0]["E"] == p.e + c.max_skip + 2 < len(c.any) and r.chunks[0]["pa"] == p.e
    assert p.last and p.run < r.n_runs - 1 and not p.flushed and p.count < c.min_size and p.n_blocks == 1
    c, r = M.case("z0-clips-below-min-size"), M.modelled("z0-clips-below-min-size")
    p = r.pairs[0]
    whole = int(c.suf[r.starts[p.run]:r.ends[p.run] + 1].sum())
    assert whole >= c.min_size > p.count > 0 and p.s > r.starts[p.run] and p.flushed and p.n_blocks == 0


def test_split_cases():
    for name in ("window-1", "window-0"):
        c, r = M.case(name), M.modelled(name)
        assert c.window == int(name[-1]) and r.n_pairs == 1 and r.blocks == [(p, p + 1) for p in np.flatnonzero(c.suf)]
    c, r = M.case("window-exact"), M.modelled("window-exact")
    s = np.flatnonzero(c.suf)
    assert s[1] - s[0] == c.window - 1 and s[2] - s[0] == c.window and r.blocks == [(s[0], s[1] + 1), (s[2], s[2] + 1)]
    c, r = M.case("window-limit-in-empty-word"), M.modelled("window-limit-in-empty-word")
    lim = r.blocks[0][0] + c.window - 1
    assert lim < r.pairs[0].e and not c.suf[(lim >> 5) << 5:lim + 1].any() and (lim >> 5) - ((r.blocks[0][1] - 1) >> 5) >= 2
    c, r = M.case("window-max"), M.modelled("window-max")
    assert c.window == (1 << 31) - 1 and len(r.blocks) == 1
    r = M.modelled("split-in-three")
    assert r.n_pairs == 1 and r.pairs[0].n_blocks >= 3


def test_chunk_cases():
    r = M.modelled("chunks-probe-429")
    assert (r.n_chunks, r.n_blocks) == (429, 857)
    for n in (256, 257, 600):
        for chunk in (7, 1):
            c, r = M.case("chunks-%d-of-%d" % (n, chunk)), M.modelled("chunks-%d-of-%d" % (n, chunk))
            assert c.chunk == chunk and r.n_chunks == n
            with_pairs = [k for k, ch in enumerate(r.chunks) if ch["n_pairs"]]
            assert with_pairs[-1] == (n - 1 if chunk == 7 else n - 2)              # the last chunk that can hold a pair
            assert pairs_of(r, with_pairs[-1])[-1].n_blocks == 1
            assert (max(with_pairs) >= M.THREADS) == (n > M.THREADS + (chunk == 1))
    r = M.modelled("chunks-empty-between")
    has = np.array([ch["n_pairs"] > 0 for ch in r.chunks])
    edges = np.flatnonzero(np.diff(has.astype(int)))
    assert r.n_chunks == 600 and not has[0] and has[-1] and len(edges) == 5          # empty, busy, empty, busy, empty, busy
    assert has[:M.THREADS].any() and has[M.THREADS:].any() and (~has[M.THREADS:]).any()


def test_stream_case_reaches_the_three_launch_scan_of_the_pairs():
    r = M.modelled("streams-to-contig-end")
    assert (r.n_chunks, r.n_runs, r.n_blocks) == (120, 600, 36180)
    assert r.n_pairs > M.SCAN_SWITCH and (r.n_pairs + M.THREADS - 1) // M.THREADS > 64
    assert all(ch["E"] == 6000 for ch in r.chunks)                                  # every stream runs to the contig end
    assert r.n_pairs // M.SCAN_BLOCK >= 4


@pytest.mark.parametrize("nw", M.SPARSE_NW)
def test_sparse_cases_load_every_scan_block(nw):
    c, r = M.case("sparse-nw-%d" % nw), M.modelled("sparse-nw-%d" % nw)
    assert r.nw == nw == len(c.any) // 32 and c.chunk == 40000 and 100 < r.n_runs < 1000
    assert (nw > M.SCAN_SWITCH) == bool(c.kills)
    n_blocks = -(-nw // M.SCAN_BLOCK)
    assert n_blocks == {16384: 4, 16385: 5, 20480: 5, 20481: 6}[nw]
    runs = list(zip(r.starts, r.ends))
    flushed = {}
    for p in r.pairs:
        if p.flushed and p.s == r.starts[p.run] and p.e == r.ends[p.run]:
            flushed.setdefault(p.s >> 5, set()).add((p.count, p.n_blocks > 0))
    for b in range(n_blocks):
        first, last = M.SCAN_BLOCK * b, min(M.SCAN_BLOCK * (b + 1), nw) - 1
        in_block = lambda w: first <= w <= last
        assert any(s >> 5 == first for s, e in runs), "a run starts in the first word of block %d" % b
        assert any(e >> 5 == last for s, e in runs), "a run ends in the last word of block %d" % b
        if b + 1 < n_blocks:
            straddle = [(s, e) for s, e in runs if s >> 5 == last and e >> 5 == last + 1]
            assert len(straddle) == 1 and straddle[0][1] - straddle[0][0] + 1 < c.min_size
        seen = set().union(*[v for w, v in flushed.items() if in_block(w)])
        assert (c.min_size, True) in seen and (c.min_size - 1, False) in seen, "flushed runs of min_size and one less in block %d" % b


def test_unit_scan_cases():
    for nw, per in ((1023, 1), (1024, 1), (1025, 2)):
        r = M.modelled("unit-scan-nw-%d" % nw)
        assert r.nw == nw and (nw + M.SCAN_THREADS - 1) // M.SCAN_THREADS == per
        assert r.starts[0] >> 5 == 0 and r.ends[-1] >> 5 == nw - 1 and len(r.blocks) == 2


def test_flag_and_sums_shapes():
    assert set(M.FLAG_S) == {4, 7, 8} and set(M.FLAG_L) == {31, 32, 63, 64, 65, 255, 256, 257}
    for S in M.FLAG_S:
        assert M.flag_min_samples(S) == (-1, 0, S - 1, S)
    assert M.FLAG_GROUPS[7] == M.FLAG_GROUPS[8] == (1, 3)
    for L in M.FLAG_L:
        blocks = M.sums_blocks(L)
        assert {(0, L), (L, L), (L - 1, L)} <= set(blocks) and all(0 <= a <= b <= L for a, b in blocks)
        words = [((b - 1) >> 5) - (a >> 5) + 1 for a, b in blocks if b > a]
        assert 1 in words and (L <= 32 or 2 in words) and (L <= 64 or max(words) >= 3)
        if L >= 65:
            bits = {a & 31 for a, b in blocks} | {b & 31 for a, b in blocks}
            assert {0, 31, 1} <= bits
