"""The shapes of tests/long_shapes.py, on the CPU: the interval reference (built from the routing model's own deletion
lists and read ends) equals the C oracle on every one of them, and the model shows that each case reaches the edge of
the long-read kernels it is named for.  A case that does not demonstrably hit its edge fails here -- a device test on
these shapes would pass for the wrong reason otherwise.  Every case has an entry in EDGES (by name or by family):
test_every_case_has_an_edge_assertion holds that."""
import importlib

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import helpers as H
from tests import long_shapes as LS

T, NW = LS.T, LS.NW


def test_model_constants_are_the_kernels():
    """The routing model restates the kernels' constants; the sources' are read from their text."""
    k = LS.kernel_constants()
    assert (k["DL_CHUNK"], k["PT_SHIFT"], k["WAVE_DELS_MIN"], k["LQ_CAP"]) == (LS.DL_CHUNK, LS.PT_SHIFT, LS.WAVE_DELS_MIN, LS.LQ_CAP)
    assert (k["OP_MAX"], k["POS_CAP"], k["WIDE"]) == (LS.OP_MAX, LS.POS_CAP, LS.WIDE)
    assert LS.POS_CAP - (1 << k["plain_pos_cap_shift"]) == LS.PLAIN_POS_CAP
    assert LS.POS_CAP - (1 << k["merged_pos_cap_shift"]) == LS.MERGED_POS_CAP
    assert (k["BATCH"], k["BATCH_AHEAD"], k["BATCH_LOAD"]) == (LS.BATCH, LS.BATCH_AHEAD, LS.BATCH_AHEAD)
    assert LS.BATCH == 4 * LS.WAVE and LS.BATCH_AHEAD == 3 * LS.BATCH          # four ops per lane, three load slots
    assert (k["T"], k["NT"], k["WAVE"]) == (LS.T, LS.NT, LS.WAVE) and k["NW_is_NT_over_WAVE"] and LS.NW == LS.NT // LS.WAVE
    assert LS.T % (1 << LS.PT_SHIFT) == 0 and LS.WAVE <= LS.LQ_CAP


@pytest.mark.parametrize("family", LS.FAMILIES)
def test_interval_reference_equals_oracle(family):
    for name in LS.names(family):
        c = LS.case(name)
        ref, orc = LS.reference(name), LS.oracle(name)
        for t, L in enumerate(c.lengths):
            ws, wm, runs, d = ref[t]
            ows, owm, oruns, od = orc[t]
            assert ws.dtype == np.int64 and wm.dtype == np.int32 and runs.dtype == np.int32
            if d is not None:
                bad = np.flatnonzero(d != od)
                assert not len(bad), "%s contig %d position %d: reference %d, oracle %d" % (name, t, bad[0], d[bad[0]], od[bad[0]])
            assert np.array_equal(ws, ows) and np.array_equal(wm, owm), (name, t)
            assert np.array_equal(runs, oruns), (name, t)
            assert len(ws) == (L + c.W - 1) // c.W and (not L or (runs[0, 0] == 0 and runs[-1, 1] == L))


def test_sparse_form_equals_the_dense_one():
    """The sparse window sums, minima and runs on cases small enough for a per-base vector."""
    for name in ("dl-op-counts", "dl-merged", "lt-clipped", "lt-deletions-index"):
        c = LS.case(name)
        for t, L in enumerate(c.lengths):
            dense = LS.reference(name)[t]
            st, va = LS.segments(*LS.interval_events(c, t), L)
            for step in (c.step_used, 300):
                ws, wm, runs = LS.sparse_results(st, va, L, c.W, c.min_cov, c.max_mean_depth, step)
                assert np.array_equal(ws, dense[0]) and np.array_equal(wm, dense[1]), (name, t)
                assert np.array_equal(runs, H.oracle_runs(dense[3], c.min_cov, c.max_mean_depth, step)), (name, t, step)
            st2, va2 = LS.segments_of_depth(dense[3][100:L - 1], 100, L) if L > 200 and not dense[3][:100].any() and not dense[3][L - 1] else (st, va)
            assert np.array_equal(st, st2) and np.array_equal(va, va2), (name, t)


def identity_holds(r, L, Q=1, flag_mask=0x704):
    """depth = sum over kept reads [pos <= x < end] - sum over list entries [x in entry], with the model's nd and end."""
    ms = LS.model_of_reads(r)
    kept = LS.kept_mask(r, Q, flag_mask)
    diff = np.zeros(L + 1, np.int64)
    for i, m in enumerate(ms):
        assert m.nd == len(m.starts) == len(m.lens)
        if kept[i]:
            np.add.at(diff, np.minimum([m.pos, m.end], L), [1, -1])
            np.add.at(diff, np.minimum(m.starts, L), -1)
            np.add.at(diff, np.minimum(m.starts + m.lens, L), 1)
    want = po.perbase_c(r, Q, 0, L, flag_mask)
    bad = np.flatnonzero(np.cumsum(diff[:L]) != want)
    assert not len(bad), int(bad[0])
    return ms


def test_identity_on_random_cigars():
    """A few hundred random CIGARs: every op code, zero-length ops, D/N floods that pass the slots, long skips."""
    rng = np.random.default_rng(11)
    walks = set()
    for seed in range(6):
        r = H.long_cigar_reads(rng, 200_000, [int(x) for x in rng.integers(0, 900, 40)], skip_every=5)
        walks |= {m.walk for m in identity_holds(r, 200_000)}
        n = 60
        pos = np.sort(rng.integers(0, 50_000, n))
        cig = []
        for _ in range(n):
            k = int(rng.integers(1, 700))
            ops = rng.choice(16, k, p=[.2, .05, .3, .2, .05, .02, .02, .04, .04] + [.08 / 7] * 7)
            cig.append([(int(l) << 4) | int(o) for o, l in zip(ops, rng.integers(0, 12, k))])
        walks |= {m.walk for m in identity_holds(LS.reads_of(list(zip(pos.tolist(), cig))), 80_000)}
    assert walks >= {"serial_dels_plain", "wave_dels_plain", "wave_dels", "serial_dels"}, walks


def test_identity_on_the_longread_tests_cases():
    """The hand-written cases of tests/test_gpu_longread.py: that module's `check` is replaced by the identity."""
    mod = importlib.import_module("tests.test_gpu_longread")
    seen = []
    def check(r, L, W=100, **params):
        seen.append(identity_holds(r, L, params.get("min_mapq", 1)))
    orig, mod.check = mod.check, check
    try:
        for fn in (mod.test_deletions_that_outnumber_their_slots, mod.test_slots_that_overflow_late_in_the_wave_walk,
                   mod.test_a_skip_too_long_for_the_wave_walk, mod.test_tile_index_at_its_boundaries,
                   mod.test_reads_whose_index_slots_are_too_few):
            fn()
        mod.test_random_long_reads(0)
    finally:
        mod.check = orig
    assert len(seen) == 6
    assert any(m.walk == "wave_dels" and m.batches >= 3 for m in seen[1])        # "late": the slots run out behind the third batch
    assert any(m.why_serial == "big" for m in seen[2])
    assert any(m.index == "search" and m.walk.endswith("plain") for m in seen[4])


# ---- every case reaches its edge -------------------------------------------------------------------------------------

def rm(c, key, tid=0):
    return LS.reads_model(c, tid)[c.mark["idx"][key]]


def plain_dn(c, i, tid=0):
    """D/N ops of at least one base of read i: what the plain walks count."""
    r = c.get(tid)
    ln, cons, dn = LS._split(r.cigar[int(r.cigar_off[i]):int(r.cigar_off[i + 1])])
    return int(dn.sum())


def edge_op_counts(c):
    for (n, a), i in c.mark["idx"].items():
        m = LS.reads_model(c)[i]
        assert m.n == n and m.o0 % 4 == a
        want = "none" if n == 0 else "serial_dels_plain" if n <= LS.WAVE_DELS_MIN else "wave_dels_plain"
        assert m.walk == want and m.batches == (-(-n // LS.BATCH) if n > LS.WAVE_DELS_MIN else -1), (n, a, m.walk, m.batches)
        if n:
            r = c.get(0)
            ops = r.cigar[m.o0:m.o0 + n] & 15
            assert ops[-1] in (LS.D, LS.N) and all(ops[b] in (LS.D, LS.N) for b in range(0, n, LS.BATCH))
            assert all(ops[b + LS.BATCH - 1] in (LS.D, LS.N) for b in range(0, n - LS.BATCH + 1, LS.BATCH))
            assert m.nd <= m.cap and m.nd == plain_dn(c, i)
    assert {n % 4 for n, _ in c.mark["idx"]} == {0, 1, 2, 3}
    # the three load slots: reads of up to one, two, three batches and one that reloads slot A and slot B
    assert {min(-(-n // LS.BATCH), 6) for n, _ in c.mark["idx"] if n > 24} >= {1, 2, 3, 4, 6}


def edge_boundary(c):
    ms = LS.reads_model(c)
    r = c.get(0)
    on, inside = set(), set()
    for m in ms:
        assert m.walk == "wave_dels_plain" and m.batches == 2 and m.index == "slot"
        ln, cons, dn = LS._split(r.cigar[m.o0:m.o0 + m.n])
        start = m.pos + np.cumsum(ln) - ln
        for k in range(LS.BATCH):
            if start[k] % T == 0:
                on.add(k)
            elif start[k] // T != (start[k] + ln[k] - 1) // T:
                inside.add(k)
    assert on == set(range(LS.BATCH)) and len(inside) >= 50
    assert {k % 4 for k in inside} == {0, 1, 2, 3}


def edge_nothing(c):
    ms = LS.reads_model(c)
    nothing = [m for m in ms if m.end == m.pos]
    assert len(nothing) == c.mark["n_nothing"]
    assert {m.walk for m in nothing} == {"none", "serial_dels_plain", "wave_dels_plain"}
    assert all(m.nd == 0 and m.index == "none" for m in nothing)
    for a, b in zip(ms, ms[1:]):                           # each between ordinary reads
        assert (a.end == a.pos) != (b.end == b.pos) or b is ms[-1]


def edge_slots(c):
    n, late = c.mark["n"], c.mark["late"]
    ms = LS.reads_model(c)
    for (parity, d), i in c.mark["idx"].items():
        m = ms[i]
        assert m.n == n and m.o0 % 2 == parity and plain_dn(c, i) == m.cap + d
        for nb in (ms[i - 1], ms[i + 1]):                  # the neighbours fill their slots exactly, on a plain walk
            assert nb.walk.endswith("plain") and nb.nd == nb.cap, (nb.nd, nb.cap)
        if d <= 0:
            assert m.walk == ("serial_dels_plain" if n <= LS.WAVE_DELS_MIN else "wave_dels_plain") and m.nd == m.cap + d
        else:
            assert m.walk == ("serial_dels" if n <= LS.WAVE_DELS_MIN else "wave_dels") and m.nd != m.cap + d and m.nd <= m.cap
            if n > LS.WAVE_DELS_MIN:
                assert m.why_again == "slots" and m.batches == (late or 0)
    # neighbouring D/N ops from cap on: had the read at cap been merged, n_deletions would differ
    i = c.mark["idx"][(0, 0)]
    r = c.get(0)
    ln, cons, dn = LS._split(r.cigar[ms[i].o0:ms[i].o0 + n])
    assert len(LS._merged_lists(ms[i].pos, ln, cons, dn)[0]) < ms[i].nd


def edge_index_slots(c):
    ms = LS.reads_model(c)
    for (a, d), i in c.mark["idx"].items():
        m = ms[i]
        assert m.o0 % 64 == a and m.K == m.pcap + d and m.walk == "wave_dels_plain"
        assert m.index == ("slot" if d <= 0 else "search")
        nxt = ms[i + 1]
        # the next read's index begins directly behind this read's slots (or inside them: slots never overlap by the rule)
        assert nxt.index == "slot" and LS.tile_at(c, 0, (nxt.pos >> 12) << 12).hit_reads
    assert {m.pcap for m in (ms[i] for i in c.mark["idx"].values())} == {3, 4}


def edge_index_clamp(c):
    m = rm(c, "3op")
    assert m.n == 3 and m.walk == "serial_dels_plain" and m.index == "search" and m.K > m.pcap + 20
    for where, batch in (("first", 0), ("middle", 0), ("last", 1)):
        m = rm(c, where)
        assert m.n == 300 and m.walk == "wave_dels_plain" and m.index == "search" and m.K > m.pcap + 60
    r = c.get(0)
    at = [int(np.flatnonzero((r.cigar[m.o0:m.o0 + m.n] >> 4) == 300000)[0]) for m in (rm(c, k) for k in ("first", "middle", "last"))]
    assert at[0] < 64 and 64 <= at[1] < 256 and at[2] >= 256


def edge_merged(c):
    ms = LS.reads_model(c)
    for key, i in c.mark["idx"].items():
        m = ms[i]
        assert m.walk == ("serial_dels" if key == "only-dn-short" else "wave_dels") and plain_dn(c, i) > m.cap, key
        assert ms[i - 1].walk == "wave_dels_plain"
        r = c.get(0)
        ln, cons, dn = LS._split(r.cigar[m.o0:m.o0 + m.n])
        groups = [dn[g:g + 64] for g in range(0, m.n, 64)]
        kinds = [set(g.tolist()) for g in groups]
        if key.startswith("run-"):                          # whole groups of D/N ops only, inside one run
            k = int(key[4:])
            assert any(all(kinds[j] == {True} for j in range(s, s + k)) and not dn[64 * s - 2] and dn[64 * s - 1] for s in range(1, len(groups) - k))
        if key == "head-0":
            assert dn[64] and not dn[63] and not dn[65]
        if key == "head-63":
            assert dn[63] and not dn[62] and not dn[64]
        if key == "close-next-batch":
            assert dn[200:256].all() and not dn[256]
        if key == "trailing":
            assert dn[-33:].all() and not dn[-34] and m.end == m.starts[-1] + m.lens[-1] + 7
        if key == "leading":
            assert dn[:37].all() and m.starts[0] == m.pos
        if key.startswith("only-dn"):
            assert dn.all() and m.nd == 0 and m.end == m.pos and m.index == "none"


def edge_op_max(c):
    for (over, merged), i in c.mark["idx"].items():
        m = LS.reads_model(c)[i]
        assert m.n > LS.WAVE_DELS_MIN
        if not over:
            assert m.walk == ("wave_dels" if merged else "wave_dels_plain") and m.why_serial == ""
        else:
            assert m.why_again == "big" and m.why_serial == "big" and m.walk == ("serial_dels" if merged else "serial_dels_plain")


def edge_units(c):
    if "counts" in c.mark:
        assert tuple(c.get(t).n for t in range(len(c.lengths))) == c.mark["counts"]
    if c.name == "dl-units":
        for t, lanes in enumerate(c.mark["lanes"]):
            ms = LS.reads_model(c, t)
            assert {i % 64 for i, m in enumerate(ms) if m.walk == "wave_dels_plain"} == set(lanes)
            assert all(m.walk in ("wave_dels_plain", "serial_dels_plain") for m in ms)
    if c.name == "dl-contigs-5":
        assert c.get(0).n == 0 and c.get(4).n == 0 and len(c.lengths) == 5
    if c.blocks > 1:
        cuts = LS.block_cuts(c.get(0).n, c.blocks)
        assert len(set(np.diff(cuts).tolist())) == c.blocks and all(x % 64 for x in cuts[1:-1])


def edge_poscap(c):
    want = [("wave_dels", 1, "pos", ""), ("wave_dels", 0, "pos", ""), ("wave_dels", 0, "pos", ""), ("serial_dels_plain", 0, "pos", "pos")]
    for t, p in enumerate(c.mark["starts"]):
        m = next(m for m in LS.reads_model(c, t) if m.pos == p)
        assert m.n > LS.WAVE_DELS_MIN and m.nd > 0
        assert (m.walk, m.batches, m.why_again, m.why_serial) == want[t], (t, m.walk, m.batches, m.why_again, m.why_serial)
        assert c.lengths[t] > m.end and c.lengths[t] <= 0x7fff0000
    m = LS.reads_model(c, 3)[0]
    assert (m.n, m.pos, m.walk, m.why_again, m.why_serial) == (300, LS.MERGED_POS_CAP - 1, "serial_dels_plain", "pos", "pos")
    assert c.sparse and c.W == 65536


def edge_candidates(c):
    t = LS.tile_at(c, 0, c.mark["t0"])
    n, which = c.mark["n"], c.mark["which"]
    assert t.lo == 0 and t.nrd == n
    r = c.get(0)
    assert abs(int((~LS.kept_mask(r, c.Q, c.flag_mask)).sum()) - n // 3) <= 1
    hits = [w.hits for w in t.waves]
    if which == "all":
        assert all(h > 0 for h in hits)
    else:
        k = 0 if which == "wave0" else 3
        assert hits[k] > 0 and sum(hits) == hits[k]
    assert sum(w.candidates for w in t.waves) == n and sum(w.pieces for w in t.waves) == sum(hits)


def edge_read_edges(c):
    t0 = c.mark["t0"]
    ms = LS.reads_model(c)
    assert {m.end for m in ms} >= {t0 - 1, t0, t0 + 1, t0 + T - 1, t0 + T, t0 + T + 1}
    assert {m.pos for m in ms} >= {t0 - 1, t0, t0 + T - 1, t0 + T}
    t = LS.tile_at(c, 0, t0)
    hit = {ms[h[0]].end for h in t.hit_reads}
    assert t0 in hit and t0 - 1 not in hit                                      # end == t0 still marks index -1; t0 - 1 does not reach


def edge_lookback(c):
    t0, span, de = c.mark["t0"], c.mark["span"], c.mark["de"]
    jm = LS.job_model(c)
    assert jm["max_span_seen"] == span and jm["lookback"] == (span + 63) // 64 * 64
    ms = LS.reads_model(c)
    i = next(i for i, m in enumerate(ms) if m.end - m.pos == span)
    assert ms[i].end == t0 + de
    t = LS.tile_at(c, 0, t0)
    assert (i in {h[0] for h in t.hit_reads}) == (de >= 0) and (de < 0 or t.lo <= i)
    # the read starts at most 64 positions inside the look-back, or one before it (and then ends before the tile)
    assert -1 <= ms[i].pos - (t0 - jm["lookback"]) <= 64 and (ms[i].pos >= t0 - jm["lookback"] or de < 0)


def edge_deletions(c):
    search = c.mark["search"]
    ms = LS.reads_model(c)
    assert all(m.index == ("search" if search else "slot") for m in ms if m.nd)
    if c.name == "lt-search-lists":
        assert sorted(m.nd for m in ms) == [1, 2, 200]
        for i in range(3):
            abs_ = [(h[2], h[3]) for t in LS.tile_models(c) for h in t.hit_reads if h[0] == i]
            assert (0, 0) in abs_ and (ms[i].nd, ms[i].nd) in abs_ and any(0 < a < ms[i].nd or a < b for a, b in abs_)
        return
    t0 = c.mark["t0"]
    tend = t0 + T
    dels = [(int(s), int(s + l)) for m in ms for s, l in zip(m.starts, m.lens)]
    for e in (t0 - 1, t0, t0 + 1):
        assert any(s < t0 and en == e for s, en in dels), e
    for s0 in (t0 - 1, t0, tend - 1, tend):
        assert any(s == s0 for s, _ in dels), s0
    assert any(s < t0 and en > tend for s, en in dels)
    t = LS.tile_at(c, 0, t0)
    a_j0 = {(h[2], h[4]) for h in t.hit_reads}
    assert (1, 0) in a_j0 and (0, 0) in a_j0                                    # the reach-in deletion is the read's first; none reaches in
    assert any(h[5] == 0 and ms[h[0]].nd > 0 for tt in LS.tile_models(c) for h in tt.hit_reads)      # rem = 0
    assert any(h[6] == 0 for h in t.hit_reads) and any(h[7] == h[8] - 1 for h in t.hit_reads)         # k0 = 0; k1 clamped
    assert any(h[7] < h[8] - 1 for h in t.hit_reads)


def edge_pieces(c):
    t = LS.tile_at(c, 0, c.mark["t0"])
    nd = c.mark["nd"]
    m = max(LS.reads_model(c), key=lambda m: m.nd)
    assert m.nd == nd and m.index == "slot"
    w = max(t.waves, key=lambda w: w.pieces)
    big = max(h[5] for h in t.hit_reads)
    assert big == nd and w.pieces == -(-nd // LS.DL_CHUNK)
    assert min(m.starts) >= t.t0 and max(m.starts) < t.tend


def edge_queue(c):
    t = LS.tile_at(c, 0, c.mark["t0"])
    for k, w in enumerate(t.waves):
        if k not in c.mark["waves"]:
            assert w.pieces == 0
        elif c.mark["extra"] == 0:
            assert w.hits == 64 and w.pieces == 128 and w.drains == [128] and w.rounds == [64, 64]
        else:
            assert w.hits == 65 and w.pieces == 129 and w.drains == [128, 1] and w.rounds == [64, 64, 1]


def edge_rounds(c):
    t = LS.tile_at(c, 0, c.mark["t0"])
    k = c.mark["k"]
    w = t.waves[0]
    assert w.rounds == [k, 1, 1, 1] and w.drains == [k + 3] and all(x.pieces == 0 for x in t.waves[1:])


def edge_clipped(c):
    tl = LS.tile_models(c)
    assert c.lengths[:3] == [T - 1, T + 1, 1]
    assert [t.rows for t in tl] == [True, False, True, True, False, False, True]
    assert all(sum(w.hits for w in t.waves) > 0 for t in tl)


def edge_wide(c):
    n = c.mark["n"]
    lo, hi, rows = LS.tile_range(c, 0, c.mark["t0"])
    r = c.get(0)
    assert hi - lo == n == r.n and rows == (n >= LS.WIDE) and n in (LS.WIDE - 1, LS.WIDE)
    assert int(r.pos.max()) - int(r.pos.min()) == 63 and (np.diff(r.cigar_off) == 1).all() and ((r.cigar & 15) == 0).all()
    assert [LS.tile_range(c, 0, t0)[1] - LS.tile_range(c, 0, t0)[0] for t0 in (0, 2 * T)] == [0, 0]
    d = LS.reference(c.name)[0][3]
    assert (d[T + 1024:T + 2048] == n).all() and c.W == T                     # the second quarter's sum: n * 1024, 2^32 from 2^22 reads on
    assert (n * 1024 >= 1 << 32) == (n >= LS.WIDE)
    assert d.max() >= c.max_mean_depth > c.min_cov > d[T] > 0                   # the classes' thresholds are crossed


EDGES = {"dl-op-counts": edge_op_counts, "dl-boundary-in-batch": edge_boundary, "dl-nothing": edge_nothing,
         "dl-index-slots": edge_index_slots, "dl-index-clamp": edge_index_clamp, "dl-merged": edge_merged,
         "dl-op-2^22": edge_op_max, "dl-pos-caps": edge_poscap, "lt-read-edges": edge_read_edges, "lt-clipped": edge_clipped}
PREFIXES = (("dl-slots-", edge_slots), ("dl-units", edge_units), ("dl-contigs-", edge_units), ("dl-blocks-", edge_units),
            ("lt-cand-", edge_candidates), ("lt-lookback-", edge_lookback), ("lt-deletions-", edge_deletions),
            ("lt-search-", edge_deletions), ("lt-pieces-", edge_pieces), ("lt-queue-", edge_queue), ("lt-rounds-", edge_rounds), ("lt-wide-", edge_wide))


def edge_of(name):
    return EDGES.get(name) or next((fn for p, fn in PREFIXES if name.startswith(p)), None)


def test_every_case_has_an_edge_assertion():
    assert all(edge_of(n) for n in LS.names()), [n for n in LS.names() if not edge_of(n)]
    assert set(LS.FAMILIES) == {LS.case(n).family for n in LS.names()}


@pytest.mark.parametrize("family", LS.FAMILIES)
def test_cases_reach_their_edges(family):
    for name in LS.names(family):
        edge_of(name)(LS.case(name))


def test_job_model_counts():
    """n_deletions and max_span_seen of a job: the plain and the merged count differ where the case says so."""
    c = LS.case("dl-slots-wave")
    plain = sum(plain_dn(c, i) for i in range(c.get(0).n))
    assert LS.job_model(c)["n_deletions"] < plain
    c = LS.case("dl-merged")
    m = LS.reads_model(c)[c.mark["idx"]["trailing"]]
    r = c.get(0)
    assert m.end < m.pos + int(H.ref_span(r)[c.mark["idx"]["trailing"]])       # a merged read ends after its last M
    f = LS.case("lt-cand-255-all")
    assert LS.job_model(f)["max_span_seen"] == max(m.end - m.pos for m in LS.reads_model(f))   # filtered reads count
