"""CPU: the shapes of tests/indexcov_shapes.py reach the edges they are named for, and the restatement
(tests/indexcov_ref.py) agrees on exactly these inputs with a second model that shares no code with it: sorted() and
Python integers for the median and the copy number, fractions.Fraction with an explicit round-to-nearest-even after
every float32 step for the depths, slots, pca8 bytes and counters (the rational model takes 30 us a value: it runs on
every slot and counter boundary and on a fixed tenth of the pca8 boundaries, 43 000 of the 460 000 threshold depths).
tests/test_gpu_indexcov_edges.py holds the device to the restatement on the same inputs."""
from fractions import Fraction

import numpy as np

from tests import indexcov_ref as R
from tests import indexcov_shapes as S

F32 = np.float32


# ---- medians --------------------------------------------------------------------------------------------------------------
def test_median_shapes_reach_their_edges_and_both_models_agree():
    shapes = dict(S.median_shapes())
    assert len(shapes) == len(S.median_shapes())                     # the names are distinct
    facts = {}
    for name, v in shapes.items():
        want, facts[name] = S.median_model(v)
        assert R.median_size([v]) == want, name
        assert R.median_size(np.array_split(v, 3)) == want, name     # however the sizes lie on the references
        assert (np.diff(v) < 0).any() or len(set(v.tolist())) <= 1 or len(v) < 20, name   # not handed over sorted
    n_of = {len(v) for v in shapes.values()}
    assert {1, 2, 3, 255, 256, 257, 1025} <= n_of and set(range(1, 301)) <= n_of
    assert {int(0.98 * n) for n in n_of} >= set(range(0, 294))
    med = {name: S.median_model(v)[0] for name, v in shapes.items()}
    # total == 0 with a non-zero size: no cumulative sum exceeds total / 2, the median is the largest size
    for name in ("zeros-99-one-5000", "zeros-981-and-19"):
        assert facts[name]["total"] == 0 and facts[name]["max"] > 0 and med[name] == facts[name]["max"], name
    assert med["zeros-99-one-5000"] == 5000
    # int(0.98 * 1000) == 980 is the rank of the smallest non-zero size of 980 zeros and 20 sizes: the cap is that size
    assert facts["zeros-980-and-20"]["n98"] == 100 and facts["zeros-980-and-20"]["total"] == 2000
    # a cumulative sum equal to total // 2: `>` and `>=` select different sizes
    for name, m in (("cum-equals-half", 2), ("cum-equals-half-shuffled", 2), ("odd-total", 4), ("half-at-run-end", 20),
                    ("run-to-half", 300), ("half-inside-run", 500)):
        assert facts[name]["cum_hits_half"] and med[name] == m, name
    assert facts["odd-total"]["odd"] and sum(f["odd"] for f in facts.values()) > 100
    # a median of 0
    zero = [name for name, m in med.items() if m == 0]
    assert {"zeros-10", "zeros-300", "zeros-3000", "one-zero"} <= set(zero) and med["one-size"] == 7 and med["zero-and-one"] == med["zeros-and-one"] == 1
    # ... and the sample with the most tiles is one of them: its tiles must not count towards `longest`
    assert max(shapes, key=lambda n: len(shapes[n])) == "zeros-3000"
    # runs of equal sizes across the 98th-percentile rank and across the median
    s = np.sort(shapes["run-over-k98"])
    k = int(0.98 * len(s))
    assert (s[k - 250:k + 20] == 5000).all() and (s == 5000).sum() >= 300 and facts["run-over-k98"]["n98"] == 5000
    for name, first, last in (("run-starts-at-k98", True, False), ("run-ends-at-k98", False, True)):
        s = np.sort(shapes[name])
        k = int(0.98 * len(s))
        assert s[k] == 5000 and (s[k - 1] < 5000) == first and (s[k + 1] > 5000) == last, name
    s = np.sort(shapes["run-ends-before-k98"])
    k = int(0.98 * len(s))
    assert s[k - 1] == 5000 and s[k] == 10000
    assert med["run-over-median"] == 1000
    # one rank lower in the first select changes the median of every tail sweep of three sizes or more: the sizes at the two ranks differ and
    # so do the medians they lead to
    for n in range(3, 301):
        s = sorted(shapes["tail-%d" % n].tolist())
        k = int(0.98 * n)
        capped = [min(x, s[k - 1]) for x in s]
        cum = np.cumsum(capped)
        other = s[min(int(np.searchsorted(cum, int(cum[-1]) // 2, side="right")), n - 1)]
        assert s[k - 1] < s[k] and other != med["tail-%d" % n], n
    # more than 40 and more than 53 bits
    assert med["big-40"] == 2 ** 40 + 1 and med["big-53"] == 2 ** 53 + 1 and med["big-61"] == 2 ** 61
    assert med["big-53-run"] == 2 ** 53 + 1 and 100 < med["big-capped"] < 400
    assert max(int(v.max()).bit_length() for v in shapes.values()) == 62


def test_depths_of_the_median_shapes_and_the_50000_cap():
    shapes = dict(S.median_shapes())
    for name in [n for n in shapes if n.startswith(("cap-", "big-", "n3", "odd", "run-to"))]:
        v = shapes[name]
        m = S.median_model(v)[0]
        d = R.normalized_depth([v], 0, m)
        assert [Fraction(float(x)) for x in d] == [S.depth_model(x, m) for x in v.tolist()], name
    for m, above in ((1, True), (7, True), (3000, False)):
        v = shapes["cap-m%d" % m]
        assert S.median_model(v)[0] == m
        d = dict(zip(v.tolist(), R.normalized_depth([v], 0, m).tolist()))
        assert d[m * 50000] == 50000 and d[m * 50000 + 1] == 50000 and d[10 ** 12] == 50000
        # one size lower is below 50 000, one higher is cut by the cap -- unless 1 / m is too small for a float32 at
        # 50 000 and both round to 50 000 itself
        assert (d[m * 50000 - 1] < 50000) == above
        assert (F32(float(m * 50000 + 1) / float(m)) > F32(50000)) == above
    assert R.normalized_depth([shapes["zeros-10"]], 0, 0).size == 0  # a median of 0: no depths at all


# ---- copy numbers ---------------------------------------------------------------------------------------------------------
def test_cn_shapes_reach_their_edges_and_both_models_agree():
    shapes = dict(S.cn_shapes())
    assert len(shapes) == len(S.cn_shapes())
    got = dict(zip(shapes, R.get_cn(list(shapes.values()))))
    facts = {}
    for name, d in shapes.items():
        want, facts[name] = S.cn_model(d)
        assert got[name] == want, name
    assert got["no-tiles"] == got["zeros"] == got["one-zero"] == -0.1
    assert got["all-low"] == got["all-low-no-zeros"] == got["one-low"] == 0.0 and facts["all-low"]["left"] == 0
    # the share of lows is exactly 0.3 and stays; its sibling's is above and is dropped; the answers differ
    for keep, drop in (("lows-3-of-10", "lows-4-of-10"), ("lows-3-of-10-zeros-count", "lows-4-of-10-zeros-count"),
                       ("lows-30-of-100", "lows-31-of-100"), ("around-0.02-3-lows", "around-0.02-4-lows")):
        assert facts[keep]["share_is_0.3"] and not facts[keep]["dropped"], keep
        assert facts[drop]["dropped"] and not facts[drop]["share_is_0.3"], drop
        d = shapes[keep]
        # had the lows of the 0.3 shape been dropped, another value would have been selected
        t = np.sort(d[d != 0])[facts[keep]["lows"]:]
        assert float(F32(2) * t[int(len(t) * 0.4)]) != got[keep], keep
    # the share counts the zero tiles: 3 lows of 8 non-zero values would be above 0.3
    assert facts["lows-3-of-10-zeros-count"]["nonzero"] == 8
    # one float32 either side of float32(0.02): only the lower one is low
    assert (facts["below-0.02"]["lows"], facts["at-0.02"]["lows"], facts["above-0.02"]["lows"]) == (4, 0, 0)
    assert facts["below-0.02"]["dropped"] and got["below-0.02"] != got["at-0.02"]
    assert {len(shapes["n%d" % n]) for n in (255, 256, 257)} == {255, 256, 257}
    assert facts["interleaved"]["n"] == 81 and facts["interleaved"]["nonzero"] == 40
    # every `left` from 1 to 300, with the selected value alone, repeated below, above, and on both sides
    for left in range(1, 301):
        k = int(float(left) * 0.4)
        for dup, below, above in (("", False, False), ("-lo", True, False), ("-hi", False, True), ("-both", True, True)):
            f = facts["left-%d%s" % (left, dup)]
            assert f["left"] == left and f["rank"] == k and f["dropped"] == (left % 5 == 0), (left, dup)
            assert f["dup_below"] == (below and k >= 1) and f["dup_above"] == (above and k + 1 < left), (left, dup)
        d = np.sort(shapes["left-%d" % left])
        d = d[d >= 0.1]
        if k >= 1:
            assert d[k - 1] < d[k]                                   # one rank lower is another value


# ---- cells ----------------------------------------------------------------------------------------------------------------
def test_cell_values_hold_ties_subnormals_and_the_cap():
    v = S.cell_values()
    assert len(v) > 27000 and (v >= 0).all()
    tie = S.tie_neighbourhood()
    exact = [x for x in tie.tolist() if "%.3g" % x != "%.3g" % float(np.nextafter(F32(x), F32(np.inf)))]
    assert len(exact) > 1000                                         # the grid crosses rounding boundaries
    assert ((v > 0) & (v < F32(1.17549435e-38))).sum() >= 2 and F32(1.4e-45) in v and (v == 0).any()
    assert {49999.996, 50000.0, 50000.004} <= {round(float(x), 3) for x in v[-3:]}


# ---- thresholds -----------------------------------------------------------------------------------------------------------
def _adjacent(v):
    """The sorted distinct values and a mask: element i + 1 is the float32 right above element i."""
    u = np.unique(v)
    return u, np.nextafter(u[:-1], F32(np.inf)) == u[1:]


def test_threshold_depths_have_both_sides_of_every_boundary():
    v = S.threshold_depths()
    assert v.dtype == F32 and len(v) == 7 * (70 + 65536 + 4) and (v > 0).all()
    u, adj = _adjacent(v)
    # slots: the unclamped integer changes k - 1 -> k between two adjacent float32, for every k = 1 .. 70
    raw = ((u * R.SLOT_C).astype(F32) + F32(0.5)).astype(np.int64)
    step = adj & (np.diff(raw) == 1)
    assert set(raw[1:][step].tolist()) >= set(range(1, 71))
    assert (R.slots_of(u) > 0).all() and raw.min() == 0              # so both sides of every slot 0 .. 69 are there
    assert (raw >= 70).any() and R.slots_of(u[raw >= 70])[69] == (raw >= 70).sum()    # the clamp at slot 69
    # pca8: the integer changes k - 1 -> k for every k = 1 .. 65 535 (65 536 is past MaxCN: the byte of 8 is 255), so
    # every byte value is entered 256 times, 255 -> 0 at every multiple of 256
    b = R.pca8_bytes(np.minimum(u, F32(8))).astype(np.int64)
    full = ((F32(8191.875) * np.minimum(u, F32(8))).astype(F32) + F32(0.5)).astype(np.int64)
    step = adj & (np.diff(full) == 1)
    assert set(full[1:][step].tolist()) == set(range(1, 65536))
    entered = np.bincount(b[1:][step], minlength=256)
    assert entered[0] == 255 and (entered[1:] == 256).all()
    assert (u > 8).sum() >= 6 and (b[u >= 8] == 255).all() and full.max() == 65535
    # uncapped, the depths above 8 would give other bytes: the order "cap, then byte" is visible
    assert (R.pca8_bytes(u[u > 8]) != 255).any()
    # the four counters: out / low / hi / in change between adjacent float32 at 0.15, 0.85, 1.15; nothing changes at 8
    dp = np.minimum(u, F32(8))
    out = (dp < F32(0.85)) | (dp > F32(1.15))
    hi = dp > F32(1.15)
    low = out & ~hi & (dp < F32(0.15))
    for edge, col in ((0.15, low), (0.85, out), (1.15, out), (1.15, hi)):
        i = int(np.searchsorted(u, F32(edge)))
        assert u[i] == F32(edge) and adj[i - 3:i + 3].all()
        flips = np.flatnonzero(col[i - 3:i + 4][1:] != col[i - 3:i + 4][:-1])
        assert len(flips) == 1, edge
    i = int(np.searchsorted(u, F32(8)))
    assert u[i] == 8 and adj[i - 3:i + 3].all() and hi[i - 3:i + 4].all()


def test_slots_bytes_and_counters_against_the_rational_model():
    v = S.threshold_depths()
    u = np.unique(v)
    # every slot boundary and counter edge, every pca8 boundary up to 1024, each byte wrap, the last 600 before MaxCN and
    # every 16th boundary in between
    k = np.arange(1, 65537)
    pick = (k <= 1024) | (k % 256 <= 1) | (k >= 64936) | (k % 16 == 5)
    some = np.concatenate([v[:7 * 70], v[7 * 70:7 * (70 + 65536)].reshape(-1, 7)[pick].ravel(), v[-28:]])
    assert len(some) > 40000
    slots = np.array([S.slot_model(x) for x in some.tolist()])
    assert np.array_equal(np.bincount(slots, minlength=70), R.slots_of(some))
    for i in range(0, len(some), 4099):                              # (and value by value, on a few)
        assert R.slots_of(some[i:i + 1])[slots[i]] == 1
    assert np.array_equal(np.array([S.byte_model(x) for x in some.tolist()], np.uint8), R.pca8_bytes(np.minimum(some, F32(8))))
    dp = np.minimum(some, F32(8))
    out = (dp < F32(0.85)) | (dp > F32(1.15))
    hi = dp > F32(1.15)
    want = np.stack([out, out & ~hi & (dp < F32(0.15)), hi, ~out], axis=1).astype(np.int64)
    assert np.array_equal(np.array([S.counter_model(x) for x in some.tolist()]), want)
    assert len(u) > 400000
