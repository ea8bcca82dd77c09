"""The shapes of tests/tile_shapes.py, on the CPU: the difference-array reference equals the C oracle on every one of
them, and the routing model shows that each case reaches the edge of the tile kernels it is named for.  A case that
does not demonstrably hit its edge fails here -- a device test on these shapes would pass for the wrong reason
otherwise.  Every case has an entry in EDGES (by name or by family): test_every_case_has_an_edge_assertion holds that."""
import numpy as np
import pytest

from tests import helpers as H
from tests import tile_shapes as TS

T = TS.T


def test_model_constants_are_the_kernels():
    """The routing model restates the kernels' constants; the sources' are read from their text."""
    k = TS.kernel_constants()
    assert (k["T"], k["NT"], k["U"], k["U_generic"]) == (TS.T, TS.NT, TS.U, TS.U)
    assert (k["FAST_CQ"], k["QCAP"], k["CQ"], k["SUPER"]) == (TS.FAST_CQ, TS.QCAP, TS.GEN_CQ, TS.SUPER)
    assert (k["ordinary_reads"], k["spec"], k["far"], k["big"]) == (TS.ORD_READS, TS.SPEC, TS.FAST_FAR, TS.FAST_BIG)
    assert k["lookback"] == TS.DEFAULT_LOOKBACK
    assert TS.NT * TS.U == TS.ORD_READS                   # an ordinary tile is one batch of the straight-line kernel


@pytest.mark.parametrize("family", TS.FAMILIES)
def test_second_reference_equals_oracle(family):
    for name in TS.names(family):
        c = TS.case(name)
        ref, orc = TS.reference(name), TS.oracle(name)
        for t, L in enumerate(c.lengths):
            d, ws, wm, at, cl = ref[t]
            od, ows, owm, oruns = orc[t]
            assert d.dtype == np.int64 and ws.dtype == np.int64 and wm.dtype == np.int32
            bad = np.flatnonzero(d != od)
            assert not len(bad), "%s contig %d position %d: reference %d, oracle %d" % (name, t, bad[0], d[bad[0]], od[bad[0]])
            assert np.array_equal(ws, ows) and np.array_equal(wm, owm), (name, t)
            assert np.array_equal(TS.runs_of(at, cl, L), oruns), (name, t)
            if L <= 3 * T:                                # helpers' window loop, on the small contigs
                hs, hm = H.oracle_windows(od, c.W)
                assert np.array_equal(ws, hs) and np.array_equal(wm, hm), (name, t)


# ---- every case reaches its edge -------------------------------------------------------------------------------------

def marked(c, fast=True):
    return TS.tile_at(c, c.mark.get("ctg", 0), c.mark["t0"], fast)


def neighbours_ordinary(c):
    """The tile before and the tile after the marked one are ordinary tiles with reads of their own."""
    t = marked(c)
    for t0 in (t.t0 - T, t.t0 + T):
        n = TS.tile_at(c, t.ctg, t0)
        assert n.ordinary and n.nrd > 0, (c.name, t0)


def edge_prep_exact(c):
    t = marked(c)
    want = {"prep-1024": (1024, None, 0, True), "prep-1025": (1025, None, 0, False),
            "prep-round-1023+1": (1024, None, 1, True), "prep-round-1022+2": (1024, None, 2, True),
            "prep-round-1024+1": (1025, None, 1, False), "prep-round-1022+3": (1025, None, 3, False),
            "prep-ops-1280": (None, 1280, 0, True), "prep-ops-1281": (None, 1281, 0, False),
            "prep-both": (1024, 1280, 0, True)}[c.name]
    nrd, nst, added, ordinary = want
    assert nrd is None or t.nrd == nrd, (c.name, t)
    assert nst is None or t.nst == nst, (c.name, t)
    assert t.lo_search - t.lo == added and t.ordinary == ordinary, (c.name, t)
    assert t.nrd <= TS.ORD_READS or nrd == 1025 and t.nst <= TS.FAST_CQ        # 1025 reads alone make it slow
    assert t.nst <= TS.FAST_CQ or nst == 1281 and t.nrd <= TS.ORD_READS        # 1281 ops alone make it slow
    assert TS.lookback_of(c)[:2] == (128, 0)
    assert TS.n_slow(c) == (0 if ordinary else 1)
    neighbours_ordinary(c)


def edge_prep_empty(c):
    e, f, z = (TS.tile_at(c, 0, c.mark[k]) for k in ("empty", "filtered", "zero"))
    assert e.nrd == 0 and e.ordinary and not TS.tile_at(c, 0, e.t0 - T).ordinary          # next to the dense one
    a = TS.fast_phase_a(c, f)
    assert f.ordinary and f.nrd >= 300 and a["inline"] == 0 and a["multi"] == 0
    nops = np.diff(c.get(0).cigar_off.astype(np.int64))[z.lo:z.hi]
    assert z.ordinary and (nops == 0).sum() >= 200 and (nops > 0).sum() >= 200
    assert TS.n_slow(c) == 1


def edge_prep_contigs(c):
    tl = TS.tiles(c)
    assert len(tl) == {"prep-contigs-9": 9, "prep-contigs-17": 17}[c.name] and (len(tl) + 7) // 8 * 8 > len(tl)   # workgroups past the last tile
    assert c.lengths[:5] == [T - 1, T, T + 1, 1, 0] and c.get(5).n == 0 and c.lengths[5] > 0
    for t in tl:
        assert t.ordinary == (t.tend - t.t0 == T), t                            # exactly the clipped tiles are slow
    assert TS.n_slow(c) == sum(L % T != 0 for L in c.lengths)
    ctgs = [t.ctg for t in tl]
    assert any(a != b for a, b in zip(ctgs, ctgs[1:]))                          # a contig boundary inside the prep wave


def edge_prep_index(c):
    t = marked(c)
    lookback = TS.lookback_of(c)[0]
    assert (t.t0 - lookback) % 64 != 0
    r = c.get(0)
    exact = int(np.searchsorted(r.pos, t.t0 - lookback))
    assert t.lo_search < exact                                                  # the rounding of `from` adds reads
    last = TS.tiles(c)[-1]
    assert last.tend % 64 != 0 and not last.ordinary
    assert (int(r.pos[-1]) >> 6) + 1 < last.tend >> 6                           # buckets k and k + 1 past the last read's


def edge_noindex(c):
    assert not c.index
    tl = TS.tiles(c)
    assert len(tl) > 4 * 64                                                     # five prep waves
    for ctg in (4, 5):
        r = c.get(ctg)
        tenth = c.lengths[ctg] // 10
        piled = (r.pos >= c.lengths[ctg] - tenth).sum() if ctg == 4 else (r.pos < tenth).sum()
        assert piled > 2 * 8192 and r.n - piled == 1
    found = TS.prep_searches(c)
    for which in ("s0", "hi"):
        branches = {f[3] for f in found if f[0] == which}
        # both probes miss, each way; the start search also brackets (an end search that hits finds it on its last element)
        assert {"left", "right"} <= branches and ("bracket" in branches or which == "hi"), (which, branches)
        miss = [f[4] for f in found if f[0] == which]
        assert min(miss) < -8192 and max(miss) > 8192, (which, min(miss), max(miss))
    # the end is searched for in lane 63 of a prep wave and on a contig's last tile, nowhere else
    asked = {g for g, t in enumerate(tl) if g % 64 == 63 or g + 1 == len(tl) or tl[g + 1].ctg != t.ctg}
    assert len([f for f in found if f[0] == "hi"]) == len(asked) == 4 + 6 - 1    # (tile 127 is both)
    assert (tl[63].ctg, tl[63].t0) == (2, T) and (tl[191].ctg, tl[191].t0) == (4, 40 * T)
    probes = [TS.step_back_probes(c, TS.tile_at(c, 0, k * T)) for k in range(1, 6)]
    back = [int(np.searchsorted(c.get(0).pos, k * T)) - TS.tile_at(c, 0, k * T).lo_search for k in range(1, 6)]
    assert back == list(TS.STEP_BACKS) and probes == [1, 2, 2, 3, 4], (back, probes)   # the 64, 256, 1024 and 4096 step-back
    ctgs = [t.ctg for t in tl]
    assert sum(a != b for a, b in zip(ctgs, ctgs[1:])) == 5                      # contigs' last tiles next to others' first


def edge_a_pairs(c):
    t = marked(c)
    a = TS.fast_phase_a(c, t)
    assert t.ordinary and a["multi"] == 0 and a["inline"] == t.nrd == c.get(0).n
    r = c.get(0)
    off = r.cigar_off.astype(np.int64)
    ops = r.cigar.astype(np.int64)
    pairs = {(int(ops[off[i]] & 15), int(ops[off[i] + 1] & 15)) for i in range(r.n) if off[i + 1] - off[i] == 2}
    singles = {int(ops[off[i]] & 15) for i in range(r.n) if off[i + 1] - off[i] == 1}
    assert {(x, y) for x in range(9) for y in range(9)} <= pairs and set(range(9)) <= singles
    assert {x for x, _ in pairs} >= set(range(9, 16))
    lens = {(int(ops[off[i]] >> 4), int(ops[off[i] + 1] >> 4)) for i in range(r.n) if off[i + 1] - off[i] == 2}
    assert set(TS.PAIR_LENS) <= lens
    assert (r.pos < t.t0 - T).any() and ((r.pos >= t.t0 - T) & (r.pos < t.t0)).any() and (r.pos >= t.t0).any()
    assert TS.lookback_of(c)[1] == 0 and TS.lookback_of(c)[2] > T


def edge_a_edges(c):
    t = marked(c)
    r = c.get(0)
    ends = r.pos.astype(np.int64) + H.ref_span(r)
    single = np.diff(r.cigar_off.astype(np.int64)) == 1
    for e in (t.t0 - 1, t.t0, t.t0 + 1, t.t0 + T - 1, t.t0 + T, t.t0 + T + 1):
        assert (single & (ends == e)).any(), e
    starts = {int(p) + int(cg >> 4) for p, cg, n2 in zip(r.pos, r.cigar[r.cigar_off[:-1].astype(np.int64)], np.diff(r.cigar_off.astype(np.int64)))
              if n2 == 2 and cg & 15 == 3}
    assert {t.t0 + T - 1, t.t0 + T} <= starts                                  # the N-led starts: s4 == T4 - 4 and s4 == T4
    L = c.lengths[0]
    assert (r.pos == t.t0 - 1).any() and (r.pos == 0).any() and (r.pos == L - 1).any() and (ends > L).any() and L % T == 0
    assert t.ordinary and TS.n_slow(c) == 0
    neighbours_ordinary(c)


def edge_a_queue(c):
    t = marked(c)
    a = TS.fast_phase_a(c, t)
    n = c.mark["n"]
    assert t.ordinary and a["multi"] == n and a["queued"] == min(n, 120) and a["walked"] == max(0, n - 120), (c.name, a)
    assert all(a["by_wave"]) and a["inline"] > 100 and a["dropped_multi"] > 0
    assert a["slots"] == {0, 1, 2, 3}
    neighbours_ordinary(c)


def edge_a_walked_span(c):
    t = marked(c)
    a = TS.fast_phase_a(c, t)
    assert t.ordinary and a["by_wave"] == [124, 0, 0, 0] and a["walked"] == 4
    order = TS.wave_rank_order(c, t, 0)
    span = H.ref_span(c.get(0))
    assert int(np.argmax(span)) == order[123] and order.index(int(np.argmax(span))) >= TS.QCAP      # walked in place
    assert TS.lookback_of(c) == (640, 1, 609)
    assert np.sort(span)[-2] <= 512                                            # no other read asks for the re-run


def edge_a_depth(c):
    t = marked(c)
    assert t.ordinary and t.nrd == 1024
    assert int(TS.reference(c.name)[0][0].max()) == 1024 and c.W == T          # `depth <= 1024 reads` of an ordinary tile
    assert TS.lookback_of(c)[1] == 0


def edge_lookback(c):
    if c.name == "lb-tighten":
        assert c.hint == 0 and not c.index
        assert TS.lookback_of(c, 1) == (512, 0, 150) and TS.lookback_of(c, 2) == (192, 0, 150)
        assert TS.n_slow(c) == 0 and max(t.nrd for t in TS.tiles(c)) < 300     # ordinary under either look-back
        return
    lb, reruns, span = TS.lookback_of(c)
    want = {"lb-exact": (512, 0, 512), "lb-exact-500": (500, 0, 500), "lb-over": (576, 1, 513), "lb-filtered-flag": (512, 0, 150),
            "lb-filtered-mapq": (512, 0, 150), "lb-queued": (576, 1, 513)}[c.name]
    assert (lb, reruns, span) == want
    r = c.get(0)
    i = int(np.argmax(H.ref_span(r)))
    t0 = c.mark["t0"]
    assert int(r.pos[i]) == t0 - int(H.ref_span(r)[i]) and int(H.ref_span(r)[i]) in (500, 512, 513)       # ends on t0 - 1
    assert (r.cigar_off[i + 1] - r.cigar_off[i] == 3) == (c.name == "lb-queued")
    assert TS.n_slow(c) == 0


def window_paths(c):
    paths, ones = set(), []
    for t, w, q in TS.quarters(c):
        for r, row in enumerate(q.rows):
            paths.add(row[0])
            if row[0] == "one":
                ones.append((row[1] & 3, row[1] >> 2, r))
    return paths, ones


def edge_window(c):
    W = c.W
    paths, ones = window_paths(c)
    want = {"several"} if W <= 128 else {"none", "one"} if W >= 256 else {"one", "several"} if W == 200 else {"one"}
    if W > max(c.lengths) or W % TS.CHUNK == 0:           # (every boundary on a quarter start: wleft == W)
        want = {"none"}
    assert paths == want, (c.name, paths)       # (W = 255 has two boundaries in a row only from position 65 280 on)
    qs = TS.quarters(c)
    assert all(1 <= q.wleft <= W or q.wleft == TS.FAST_BIG for _, _, q in qs)
    assert (W > TS.FAST_FAR) == all(q.wleft == TS.FAST_BIG for _, _, q in qs)
    d = TS.reference(c.name)[0][0]
    assert len(np.unique(np.diff(d[:T]))) > 2                                                      # a ramp
    ends = [p for p in c.mark["dips"] if int(d[p]) < int(d[p - 1]) and int(d[p]) < int(d[p + 1])]
    assert len(ends) >= 2, ends                           # single-position dips on a tile's and a quarter's last / first position
    if W in (4096, 1024, 256, 64, 32, 4, 2, 1):
        assert any(q.wleft == W for _, _, q in qs)                                                 # a boundary on a quarter / tile start


def test_window_family_covers_every_path_and_straddle():
    paths, ones = set(), []
    for name in TS.names("windows"):
        p, o = window_paths(TS.case(name))
        paths |= p
        ones += o
    assert paths == {"none", "one", "several"}
    for k in range(4):
        assert any(o[0] == k and o[1] == 0 for o in ones), "rel & 3 == %d in lane 0" % k
        assert any(o[0] == k and o[1] == 63 for o in ones), "rel & 3 == %d in lane 63" % k
        assert any(o[0] == k and o[2] == 0 for o in ones), "rel & 3 == %d in the first row" % k
        assert any(o[0] == k and o[2] == 3 for o in ones), "rel & 3 == %d in the last row" % k
    assert any(o == (2, 63, 3) for o in ones)                                                      # rel & 3 == 2 in lane 63 of row 3


def edge_classes(c):
    d = TS.reference(c.name)[0][0]
    at = set(TS.reference(c.name)[0][3].tolist())
    q = TS.CHUNK
    if c.max_mean_depth != 4:
        for p in (0, T, T + q, T + 2 * q + 256, 2 * T - 1, 2 * T + q):
            assert p in at, (c.name, p)
        lane = T + 2 * q + 512
        assert {lane + 81, lane + 86, lane + 91} <= at and lane % 256 == 0 and (lane + 81) % 4 == 1 and (lane + 86) % 4 == 2 and (lane + 91) % 4 == 3
    if c.max_mean_depth == 6:
        assert {T + 2 * q + 512 + 40, T + 2 * q + 512 + 44} <= at                # a lane's first position
        assert 3 * T + 100 in at and int(d[3 * T + 100]) == 6 and int(d[3 * T + 99]) == 5
    t1 = TS.tile_at(c, 0, T)
    qs = [TS.quarter(c, t1, w, d) for w in range(4)]
    if c.step == 0 and c.max_mean_depth != 4:
        # the quarter after T + q: every position CALLABLE, only the carry raises any_noisy
        assert [k for k, v in qs[1].noisy.items() if v] == ["carry_low"], qs[1].noisy
        t2 = TS.tile_at(c, 0, 4 * T)
        q2 = [TS.quarter(c, t2, w, d) for w in range(4)]
        assert q2[0].any_noisy and not q2[1].any_noisy and q2[2].any_noisy      # a CALLABLE quarter between two that are not
    if c.step in (1024, 4096):
        t4 = TS.tile_at(c, 0, 5 * T)
        q4 = TS.quarter(c, t4, 0, d)
        assert q4.sleft == 0 and [k for k, v in q4.noisy.items() if v] == ["forced"]               # a forced break on a quarter start
    if c.step == 3:
        assert TS.boundaries(c)[0] > TS.SPEC
    if c.step > TS.FAST_FAR:
        assert all(q.sleft in (0, TS.FAST_BIG) for _, _, q in TS.quarters(c))
    assert TS.n_slow(c) == 1


def edge_bounds(c):
    assert TS.boundaries(c)[0] == c.mark["target"] and c.mark["target"] in (TS.SPEC - 1, TS.SPEC, TS.SPEC + 1)
    assert TS.capacity_reruns(c) == 0


def edge_cap_grow(c):
    assert c.fresh and TS.boundaries(c)[0] == 17 * T > TS.CAP_RUNS0 and TS.capacity_reruns(c) == 1
    assert TS.n_slow(c) == 0 and all(t.nrd <= 1024 for t in TS.tiles(c))       # every position a forced break, ordinary tiles
    d = TS.reference(c.name)[0][0]
    assert int(d[300:-300].min()) == int(d[300:-300].max()) == 5


def edge_alternating(c):
    t = marked(c)
    at = TS.reference(c.name)[0][3]
    assert not t.ordinary and t.nrd >= 2048 and ((at >= T) & (at < 2 * T)).sum() == T
    neighbours_ordinary(c)


def edge_super(c):
    total, groups = TS.boundaries(c)
    assert c.n_tiles == 1030 and len(groups) == 2 and min(groups) > 5
    at0 = TS.reference(c.name)[0][3]
    assert ((at0 >= 1023 * T) & (at0 < 1024 * T)).sum() >= 2 and ((at0 >= 1024 * T) & (at0 < 1025 * T)).sum() >= 3
    assert len(TS.reference(c.name)[1][3]) == 1 and len(TS.reference(c.name)[2][3]) > 5           # a contig without class changes between
    assert TS.tile_at(c, 0, 1023 * T).ordinary and TS.tile_at(c, 0, 1024 * T).ordinary


def edge_generic(c):
    tf, tg = marked(c), marked(c, fast=False)
    g = TS.generic_phase_a(c, tg)
    name = c.name
    if name.startswith("g-reads-"):
        n = int(name.rsplit("-", 1)[1])
        assert tg.nrd == n and g["batches"] == (n + 1023) // 1024 and tf.ordinary == (n <= 1024 and tf.nst <= 1280)
    elif name.startswith("g-ops-"):
        n = int(name.rsplit("-", 1)[1])
        assert tg.nst == n and g["staged"] == (n <= 1536)
    elif name == "g-wave-64":
        assert g["waves"][0] == [("queue", 64)] and not any(g["waves"][1:])
    elif name == "g-wave-65":
        assert g["waves"][0] == [("slots", (64, 1, 0, 0))] and not any(g["waves"][1:])
    elif name == "g-wave-256":
        assert g["waves"][0] == [("slots", (64, 64, 64, 64))] and not any(g["waves"][1:])
    elif name == "g-cross-64":
        assert g["waves"][0] == [("queue", 32), ("queue", 64)] and g["batches"] == 2
    elif name == "g-cross-65":
        assert g["waves"][0] == [("queue", 32), ("drain+queue", 33)] and g["batches"] == 2
    elif name == "g-not-m":
        a = TS.fast_phase_a(c, tf)
        assert tf.ordinary and a["multi"] == 0 and g["queued"] == 400           # inline there, queued here
    else:
        raise AssertionError("no edge for " + name)
    assert tg.lo == tf.lo == 120                                                # nothing reaches the tile from the one before
    neighbours_ordinary(c)


EDGES = {"prep-empty-filtered-zero-ops": edge_prep_empty, "prep-contigs-9": edge_prep_contigs, "prep-contigs-17": edge_prep_contigs,
         "prep-index-edges": edge_prep_index, "noindex-search": edge_noindex, "a-pairs": edge_a_pairs, "a-edges": edge_a_edges,
         "a-walked-span": edge_a_walked_span, "a-depth-1024": edge_a_depth, "c-cap-grow": edge_cap_grow,
         "c-alternating": edge_alternating, "c-super-1030": edge_super}
PREFIXES = (("prep-", edge_prep_exact), ("a-queue-", edge_a_queue), ("lb-", edge_lookback), ("w-", edge_window),
            ("cls-", edge_classes), ("c-bounds-", edge_bounds), ("g-", edge_generic))


def edge_of(name):
    return EDGES.get(name) or next((f for p, f in PREFIXES if name.startswith(p)), None)


def test_every_case_has_an_edge_assertion():
    assert all(edge_of(n) for n in TS.names())
    assert sorted({TS.case(n).family for n in TS.names()}) == sorted(TS.FAMILIES)


@pytest.mark.parametrize("name", TS.names())
def test_case_reaches_its_edge(name):
    c = TS.case(name)
    assert c.edge
    edge_of(name)(c)
    # what the device test asserts from the model is defined for every case
    assert TS.lookback_of(c)[0] % 64 == 0 or TS.lookback_of(c)[1] == 0
    assert 0 <= TS.n_slow(c) <= c.n_tiles
