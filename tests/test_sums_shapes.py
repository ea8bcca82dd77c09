"""The shapes of tests/sums_shapes.py, on the CPU: the interval reference equals the C oracle on every one of them, and
the routing model shows that each case reaches the edge of gd_sums_stream_kernel it is named for.  A case that does
not demonstrably hit its edge fails here -- a device test on these shapes would pass for the wrong reason otherwise."""
import numpy as np
import pytest

from oracle import pyoracle as po
from tests import helpers as H
from tests import sums_shapes as S


@pytest.fixture(scope="module")
def routed():
    cache = {}

    def get(name, tid):
        if (name, tid) not in cache:
            c = S.case(name)
            cache[name, tid] = S.classify(c.get(tid), c.Q, c.flag_mask, c.lengths[tid], c.W)
        return cache[name, tid]
    return get


def counted_bases(r, Q, flag_mask, length):
    """Counted bases inside the contig, one read and one op at a time."""
    total = 0
    for i in range(r.n):
        if (int(r.flag[i]) & flag_mask) or int(r.mapq[i]) < Q:
            continue
        x = int(r.pos[i])
        for c in r.cigar[int(r.cigar_off[i]):int(r.cigar_off[i + 1])].tolist():
            l, o = c >> 4, c & 15
            if o in S.COUNTED:
                total += max(0, min(x + l, length) - max(x, 0))
            if o in S.CONSUMING:
                x += l
    return total


@pytest.mark.parametrize("name", S.NAMES)
def test_interval_reference_equals_oracle(name):
    c = S.case(name)
    want = S.oracle_sums(name)
    for t, L in enumerate(c.lengths):
        got = S.interval_window_sums(c.get(t), c.Q, c.flag_mask, L, c.W)
        assert got.dtype == np.int64 and got.shape == want[t].shape, (name, t)
        bad = np.flatnonzero(got != want[t])
        assert not len(bad), "%s contig %d window %d: intervals %d, oracle %d" % (
            name, t, bad[0], got[bad[0]], want[t][bad[0]])
        if t in c.huge:
            assert int(got.sum()) == counted_bases(c.get(t), c.Q, c.flag_mask, L) > 0


@pytest.mark.parametrize("seed,L,n,W,Q,mask", [(1, 150_001, 12_000, 100, 1, 0x704), (2, 9_001, 2_500, 32, 0, 0),
                                                 (3, 40_000, 5_000, 4096, 128, 0x8000)])
def test_interval_reference_equals_oracle_on_edge_reads(seed, L, n, W, Q, mask):
    r = H.edge_reads(np.random.default_rng(seed), L, n)
    got = S.interval_window_sums(r, Q, mask, L, W)
    want = H.oracle_windows(po.perbase_c(r, Q, 0, L, flag_mask=mask), W)[0]
    assert np.array_equal(got, want)
    assert int(got.sum()) == counted_bases(r, Q, mask, L)


def test_model_constants_are_the_kernels():
    """The routing model restates the kernel's constants; the header's are read from its text."""
    k = S.kernel_constants()
    assert (k["reads_per_lane"], k["group"], k["wave"]) == (4, S.GROUP_READS, S.WAVE_READS)
    assert k["queue"] == k["drain_at"] == S.QUEUE_SLOTS                # (the product build sets no -DGD_SUMS_DRAIN_AT)
    assert k["accumulators"] == S.N_ACC and k["fit_bases"] == S.FIT_BASES


def ballot_contig(n_reads, unit, local=False):
    """The kernel's contig search as its comments state it: the last contig whose first unit is <= unit, found 64 table
    entries per round, a round counting its entries that qualify and the search ending at the first round that is not
    all of them.  local=True forgets the round's base (the index within the round only)."""
    first, u = [], 0
    for n in n_reads:
        first.append(u)
        u += (n + S.WAVE_READS - 1) // S.WAVE_READS
    ci = 0
    for base in range(0, len(n_reads), 64):
        cnt = sum(f <= unit for f in first[base:base + 64])
        ci = (0 if local else base) + cnt - 1
        if cnt < 64:
            break
    return ci


# ---- each case reaches its edge -------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_ctgs", [131, 64, 65])
def test_case_a_read_counts_and_contig_table(routed, n_ctgs):
    c = S.case("a%d" % n_ctgs)
    assert len(c.lengths) == n_ctgs and all(0 < L <= 1 << 24 for L in c.lengths)
    n = {t: c.get(t).n for t in range(n_ctgs)}
    want = set((1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 511, 512, 513, 767, 768, 769, 1023, 1024, 1025, 4095, 4096, 4097,
                4351, 4353, 8191, 8192, 8193, 12289))
    if n_ctgs == 131:
        assert want <= set(n.values())
        assert all(n[t] == 0 for t in (0, 62, 66, 126, 129, 130))
        assert all(n[t] > 0 for t in (63, 64, 65, 127, 128))
        assert c.lengths[S.A_UNIT] == 1 and n[S.A_UNIT] == 1 and c.get(S.A_UNIT).cigar.tolist() == [1 << 4]
    assert n[63] == 4097 and n[0] == n[62] == 0                      # the last contig of the first ballot round has two units
    owner = S.unit_contigs(c)
    counts = [n[t] for t in range(n_ctgs)]
    assert [ballot_contig(counts, u) for u in range(len(owner))] == owner      # the search as stated finds every unit's contig
    assert owner.count(63) == 2                                      # both need a full first round: 64 of 64 entries qualify
    if n_ctgs == 64:
        assert max(owner) == 63 and owner[-2:] == [63, 63]
    else:
        # units 0 to 3 of contig 64 exist, and only the second ballot round tells them from contig 63's; a search that
        # forgot the round's base would give every unit from contig 64 on to another contig
        assert n[64] == 12289 and owner.count(64) == 4 and len(routed(c.name, 64).waves) == 4
        beyond = [u for u, t in enumerate(owner) if t >= 64]
        assert len(beyond) >= 4 and all(ballot_contig(counts, u, local=True) != owner[u] for u in beyond)
    if n_ctgs == 131:
        assert {65, 127, 128} <= set(owner) and owner.count(65) == 3 and owner.count(127) == 2
    for t in (t for t in range(n_ctgs) if n[t] in want and t != S.A_UNIT and c.lengths[t] > 1):
        r = c.get(t)
        lens = (r.cigar >> 4)
        assert len(r.cigar) == r.n and len(set(lens.tolist())) == r.n, "lengths are unique within contig %d" % t
        rt = routed(c.name, t)
        i = np.arange(r.n)
        must = (i % 256 == 0) | (i == r.n - 1) | (i % 3 != 2)
        assert np.array_equal(rt.kept, must), t
        drop = np.flatnonzero(~rt.kept)
        reasons = [(int(r.flag[k]), int(r.mapq[k])) for k in drop]
        assert all((f in (0x4, 0x100, 0x200, 0x400)) != (q == 0) for f, q in reasons)       # exactly one reason each
        if r.n >= 64:
            assert len(set(reasons)) == 5
    # both paths are taken in the large contigs: reads that fit and reads that are queued and drained
    big = routed(c.name, 63)
    assert big.waves[0].n_fit > 0 and big.waves[0].n_odd > 256 and len(big.waves[0].drains) > 1
    assert big.waves[1].n_fit + big.waves[1].n_odd == 1


def test_case_b_every_short_cigar(routed):
    c = S.case("b")
    assert c.W == 64
    for t, n_ops, n in ((0, 1, 48), (1, 2, 2304), (2, 3, 4096)):
        r = c.get(t)
        assert r.n == n and np.all(np.diff(r.cigar_off.astype(np.int64)) == n_ops)
        assert np.all(np.diff(r.pos) == 29)
        ops = (r.cigar & 15).reshape(n, n_ops)
        assert len({tuple(x) for x in ops.tolist()}) == 16 ** n_ops
        assert set((r.cigar >> 4).tolist()) == {0, 1, 37}
        both = set(map(tuple, np.concatenate([ops, (r.cigar >> 4).reshape(n, n_ops)], 1).tolist()))
        if n_ops < 3:                                               # every op combination with every length combination
            assert len(both) == 16 ** n_ops * 3 ** n_ops - (3 if n_ops == 2 else 0)   # (`0S <n>N`)
    r = c.get(1)
    two = r.cigar.reshape(-1, 2)
    assert not np.any((two[:, 0] == 4) & ((two[:, 1] & 15) == 3)), "no `0S <n>N`"
    rt = routed("b", 1)
    assert {"fit", "odd", "none"} <= set(rt.route)
    w = routed("b", 2).waves
    assert len(w) == 1 and w[0].refused and w[0].n_three == 256 and w[0].n_odd == 4096 - 256
    assert max(w[0].occupancy) == 256


def test_case_c_queue_occupancy(routed):
    c = S.case("c")
    assert c.W == 250
    w = [routed("c", t).waves for t in range(7)]
    assert all(len(x) == 1 for x in w)
    w = [x[0] for x in w]
    # 256 three-op reads in the first group: the queue is exactly full, nothing is refused, one final drain
    assert w[0].occupancy == [64, 128, 192, 256] and not w[0].refused and w[0].drains == [(256, 0)]
    # 257: the last one is refused, becomes an odd read and forces a drain of the full queue
    assert w[1].refused and w[1].n_three == 256 and w[1].n_odd == 1 and w[1].drains == [(256, 0), (0, 1)]
    # 256 five-op reads, 64 per group: exactly full, no drain before the end
    assert w[2].occupancy == [64, 128, 192, 256] and w[2].drains == [(0, 256)] and w[2].n_odd == 256
    # 257: one past full
    assert w[3].n_odd == 257 and w[3].drains == [(0, 256), (0, 1)]
    # every group queues 256 reads: the queue fills to the brim and is drained 16 times
    assert w[4].n_odd == 4096 and w[4].drains == [(0, 256)] * 16 and max(w[4].occupancy) == 256
    # alternating: both kinds of item in the queue at every drain but the first (the three-op reads of groups 0 and 1:
    # the ops of a group are fetched before the group before it is worked on) and the final one (the odd reads of groups 14 and 15)
    assert w[5].n_three == w[5].n_odd == 2048 and not w[5].refused
    assert w[5].drains == [(256, 0)] + [(128, 128)] * 14 + [(0, 256)]
    assert max(w[5].occupancy) == 256
    # only the final drain
    assert w[6].drains == [(0, 1)] and w[6].n_fit == 4095 and routed("c", 6).route[4095] == "odd"
    for x in w:
        assert max(x.occupancy) <= 256


@pytest.mark.parametrize("W", [32, 100, 4096])
def test_case_d_three_window_fit(routed, W):
    c = S.case("d%d" % W)
    r, L = c.get(0), c.lengths[0]
    rt = routed(c.name, 0)
    assert L <= 1 << 24 and r.n > S.WAVE_READS
    first = r.pos[0::4].astype(np.int64)                             # the lanes' first reads
    assert {0, 1, W - 1} <= set((first % W).tolist())
    i = np.arange(r.n)
    later = i % 4 != 0
    form = lambda k: "".join(S.OPS[o & 15] for o in r.cigar[int(r.cigar_off[k]):int(r.cigar_off[k + 1])].tolist())
    forms = {"M", "SM", "MS", "MI", "MD", "HM"}
    for over, route in ((-1, "fit"), (0, "fit"), (1, "odd")):
        hit = np.flatnonzero(later & rt.kept & (rt.end == rt.nb2 + over) & (rt.end < L) & (r.pos >= 10 * W))
        # every form (plain and the five two-op ones) for every start offset of the lane, each exactly once
        pairs = sorted((form(k), int(r.pos[k - k % 4]) % W) for k in hit)
        assert pairs == sorted((f, d) for f in forms for d in {0, 1, W - 1}), (W, over, pairs)
        assert all(rt.route[k] == route for k in hit), (W, over)
    span = po.read_ends(r) - r.pos
    assert np.any((r.pos % W == 0) & (span == W) & (i % 4 != 0)), "boundary to boundary"
    # every form at position 0 and, with 77 counted bases, at the contig's last position
    assert {form(k) for k in np.flatnonzero(r.pos == 0)} == forms
    assert {form(k) for k in np.flatnonzero((r.pos == L - 1) & (r.cigar[r.cigar_off[:-1]] >> 4 != 1)
                                            & ((rt.end == L) & rt.kept))} == forms
    assert np.any((r.pos == L - 1) & (span == 77))
    # `150M` (and its five two-op forms) to the contig's last base, and one base past it (clipped)
    assert np.sum((r.pos == L - 150) & (rt.end == L)) >= 6 and np.sum((r.pos == L - 149) & (rt.end == L)) >= 6
    assert all(rt.route[k] in ("fit", "odd") for k in range(r.n))


def test_case_e_accumulator_range(routed):
    c = S.case("e")
    assert c.W == 32
    w = [routed("e", t).waves for t in range(6)]
    assert all(len(x) == 1 for x in w)
    w = [x[0] for x in w]
    for t in (0, 4):
        assert (w[t].first_window, w[t].lo_window, w[t].hi_window) == (S.E_KW0, S.E_KW0, S.E_KW0 + 255), t
    for t in (1, 5):
        assert (w[t].first_window, w[t].lo_window, w[t].hi_window) == (S.E_KW0, S.E_KW0, S.E_KW0 + 256), t
    assert w[0].n_fit == w[1].n_fit == 0 and w[4].n_odd == w[5].n_odd == 0     # the queue's way and the lanes' way
    r = c.get(2)
    assert np.all(np.diff(r.pos.astype(np.int64)) == 300 * 32) and w[2].hi_window > S.E_KW0 + 255 * 300
    assert w[3].hi_window >= S.E_KW0 + 10_000 and w[3].lo_window == S.E_KW0
    s = S.case("e-short")
    assert s.lengths[0] < s.W == 4096 and s.get(0).n == 4097
    ws = routed("e-short", 0).waves
    assert len(ws) == 2 and ws[0].hi_window == ws[1].hi_window == 0


def test_case_f_length_and_magnitude(routed):
    for name, routes in (("f-len-4096", ["odd", "odd", "odd"]), ("f-len-2m", ["fit", "odd", "odd"])):
        c = S.case(name)
        r = c.get(0)
        assert (r.cigar[:3] >> 4).tolist() == [(1 << 22) - 1, 1 << 22, (1 << 22) + 1] and c.lengths[0] == 1 << 24
        assert routed(name, 0).route[:3] == routes
    assert S.case("f-len-2m").W == 1 << 21
    c = S.case("f-sum")
    rt = routed("f-sum", 0)
    assert rt.route == ["fit"] * 4096
    per_group = 256 * ((1 << 22) - 1)
    assert (1 << 29) < per_group < (1 << 32) and S.oracle_sums("f-sum")[0][0] == 16 * per_group > (1 << 32)
    # 4096 reads that the 2^22 bound keeps out of the lanes: folded there, a group would sum to 2^32 exactly
    wide = S.case("f-sum-wide")
    assert routed("f-sum-wide", 0).route == ["odd"] * 4096 and wide.W == wide.lengths[0] == 1 << 24
    assert S.oracle_sums("f-sum-wide")[0].tolist() == [4096 << 24] and 256 << 24 == 1 << 32
    assert S.case("f-w-max").W == (1 << 31) - 1 and S.case("f-w-2^30+1").W == (1 << 30) + 1
    h = S.case("f-huge")
    r = h.get(0)
    assert h.lengths[0] == 0x7fff0000 and h.W == (1 << 30) + 1
    assert np.sum(r.pos >= 0x7fff0000 - 70_000) == 20 and po.read_ends(r)[-1] > 0x7fff0000
    assert np.all(po.read_ends(r) - r.pos < 1 << 27)
    sums = S.oracle_sums("f-huge")[0]
    assert len(sums) == 2 and sums[0] > 0 and sums[1] > 0


def test_guard_case_read_counts():
    """Every remainder of the read count by 4 that makes the rounded-up flag / MAPQ loads reach past the records, in a
    first wave and in a second one."""
    c = S.case("guard")
    n = [c.get(t).n for t in range(len(c.lengths))]
    assert c.guarded and {1, 2, 3} == {x % 4 for x in n if x < S.WAVE_READS} == {x % 4 for x in n if x > S.WAVE_READS}
    assert all(c.get(t).flag.max() == 0 and c.get(t).mapq.min() == 60 for t in range(len(n)))    # the last reads are kept
