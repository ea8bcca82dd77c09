"""Crafted inputs for indexcov's device kernels (goleft_amd/csrc/gd_indexcov.hpp, gd_round3g.hpp) at the places where a
selection or a rounding can be off by one: duplicates across the selected rank, a cumulative sum equal to total / 2, the
`tot == 0` branch, a median of 0, the 0.3 share of GetCN, three-digit ties of the cells, and every float32 next to a
slot, pca8 or counter threshold -- with a second model of each operation that shares no code with
tests/indexcov_ref.py (sorted() and Python integers for the selections, fractions.Fraction for the float32 steps).

Test infrastructure only, plain numpy, no pytest marks: tests/test_indexcov_shapes.py (CPU) shows that every shape
reaches its edge and that both models agree; tests/test_gpu_indexcov_edges.py feeds them to the device."""
from fractions import Fraction
from functools import lru_cache

import numpy as np

F32 = np.float32
INF32 = F32(np.inf)
ZERO32 = F32(0)


def _shuffled(rng, v):
    """The kernels select from unsorted sizes: no shape hands them a sorted array."""
    return rng.permutation(np.asarray(v, np.int64))


# ---- median shapes --------------------------------------------------------------------------------------------------------
def tail_sweep(n):
    """n sizes on which the median depends on the 98th-percentile cap: 1, 2, 3, ... (their sum S) below rank
    k - 1 = int(0.98 n) - 1, a size A at that rank and sizes from B = 4 S on behind it, c = n - k + 1 in all, with
    A c < S.  Capped at sorted[k] = B the tail outweighs S and the median lies in the tail; capped at sorted[k - 1] = A,
    one rank too low, it would not, and the median would be one of the small sizes.  (Where n is too small for such an A,
    10^6 and 2 * 10^6 stand at the two last ranks: the cap decides between them.)"""
    k = int(0.98 * float(n))
    start = max(k - 1, 0)
    c, S = n - start, start * (start + 1) // 2
    A, B = S // c - 1, 4 * S
    if A <= start:
        A, B = 10 ** 6, 2 * 10 ** 6
    v = np.arange(1, n + 1, dtype=np.int64)
    v[start] = A
    v[start + 1:] = B + np.arange(n - start - 1)
    return v


@lru_cache(maxsize=None)
def median_shapes():
    """(name, int64 sizes) per sample; every sum is below 2^62, so the kernel's sums and numpy's cumsum are exact."""
    rng = np.random.default_rng(98)
    out = []
    for n in (1, 2, 3, 255, 256, 257, 1025):
        out.append(("n%d" % n, _shuffled(rng, np.arange(n) * 7 + 3)))
        out.append(("n%d-dup" % n, _shuffled(rng, np.arange(n) // 3 + 1)))
    out += [("equal-10", np.full(10, 500)), ("equal-256", np.full(256, 12345)), ("equal-257", np.full(257, 1)),
            ("zeros-10", np.zeros(10)), ("zeros-300", np.zeros(300)), ("zeros-3000", np.zeros(3000)),   # (the sample with the most tiles)
            ("one-zero", [0]), ("one-size", [7]),
            ("cum-equals-half", [1, 1, 2]), ("cum-equals-half-shuffled", [2, 1, 1]),
            ("odd-total", [4, 1, 2]),                       # total 7, half 3 = the cumulative sum at the 2: the answer is 4
            ("half-at-run-end", [5, 20, 5, 5, 5]),          # cumsum 5 10 15 20 40, half 20: the answer is 20
            ("zero-and-one", [0, 1]), ("zeros-and-one", [0, 0, 0, 1])]
    # a run of 300 equal sizes across rank int(0.98 n): n = 1305, rank 1278, the run at ranks 1000 .. 1299
    out.append(("run-over-k98", _shuffled(rng, np.r_[np.arange(1, 1001), np.full(300, 5000), 10 ** 4 + np.arange(5)])))
    # the rank is the first / the last of the run, and the first size behind it
    out.append(("run-starts-at-k98", _shuffled(rng, np.r_[np.arange(1, 981), np.full(15, 5000), 10 ** 4 + np.arange(5)])))
    out.append(("run-ends-at-k98", _shuffled(rng, np.r_[np.arange(1, 671), np.full(311, 5000), 10 ** 4 + np.arange(19)])))
    out.append(("run-ends-before-k98", _shuffled(rng, np.r_[np.arange(1, 671), np.full(310, 5000), 10 ** 4 + np.arange(20)])))
    # a run across the median rank, and one that the cumulative sum leaves exactly at total / 2
    out.append(("run-over-median", _shuffled(rng, np.r_[np.arange(1, 101), np.full(400, 1000), 2000 + np.arange(100)])))
    out.append(("run-to-half", _shuffled(rng, np.r_[np.full(30, 10), 300])))                 # cumsum 300 = half after the run
    out.append(("half-inside-run", _shuffled(rng, np.r_[np.full(300, 10), np.full(8, 500)])))   # 3500 = half after one 500
    # total == 0 and a non-zero tail: nothing exceeds total / 2 = 0, the index falls back to the largest size
    out.append(("zeros-99-one-5000", _shuffled(rng, np.r_[np.zeros(99), 5000])))
    out.append(("zeros-981-and-19", _shuffled(rng, np.r_[np.zeros(981), 100 + 13 * np.arange(19)])))
    # (int(0.98 * 1000) is 980: with 980 zeros the cap is the smallest non-zero size and the total is not 0)
    out.append(("zeros-980-and-20", _shuffled(rng, np.r_[np.zeros(980), 100 + 13 * np.arange(20)])))
    # sizes above 2^40 and 2^53
    big = [2 ** 40 + 1, 2 ** 53 + 1, 2 ** 61]
    out += [("big-40", [2 ** 40 + 1, 1, 2 ** 40 + 1, 2, 2 ** 40 + 1]), ("big-53", [5, 2 ** 53 + 1, 2 ** 53 + 1, 2 ** 53 + 1]),
            ("big-61", [3, 2 ** 61, 3, 2 ** 53 + 1, 7, 2 ** 40 + 1, 3]),
            ("big-capped", _shuffled(rng, big + list(range(100, 400)))),
            ("big-53-run", _shuffled(rng, [2 ** 53 + 1] * 300 + [2 ** 53] * 20 + [2 ** 53 + 2] * 3))]
    for n in range(1, 301):
        out.append(("sweep-%d" % n, _shuffled(rng, np.arange(1, n + 1))))
        out.append(("tail-%d" % n, _shuffled(rng, tail_sweep(n))))
    out += depth_shapes()
    out = [(name, np.asarray(v, np.int64)) for name, v in out]
    for _, v in out:
        assert (v >= 0).all() and sum(int(x) for x in v) < 2 ** 62
        v.setflags(write=False)
    return tuple(out)


def depth_shapes():
    """The 50 000 cap of the depth: 250 tiles of m fix the median at m (four outliers stay above the 98th percentile);
    (50 000 m + 1) / m rounds above 50 000 for m = 1 and 7 and to 50 000 itself for m = 3000."""
    rng = np.random.default_rng(50000)
    return [("cap-m%d" % m, _shuffled(rng, [m] * 250 + [m * 50000 - 1, m * 50000, m * 50000 + 1, 10 ** 12])) for m in (1, 7, 3000)]


def median_model(sizes):
    """Index.init (indexcov.go:104-124) with sorted() and Python integers; returns (median, facts)."""
    s = sorted(int(x) for x in sizes)
    n98 = s[int(0.98 * float(len(s)))]
    total, cumsum = 0, []
    for v in s:
        total += min(v, n98)
        cumsum.append(total)
    idx = 0
    while idx < len(cumsum) and not cumsum[idx] > total // 2:
        idx += 1
    while idx >= len(s):
        idx -= 1
    return s[idx], {"total": total, "max": s[-1], "n98": n98, "cum_hits_half": total // 2 in cumsum, "odd": total % 2 == 1}


def depth_model(size, median):
    """float32(float64(size) / float64(median)) capped at 50 000, as an exact rational (NormalizedDepth :144-148): every
    conversion and the division are one correct rounding each."""
    q = _rne(_rne(Fraction(int(size)), 53) / _rne(Fraction(int(median)), 53), 53)
    return min(_rne(q, 24), Fraction(50000))


# ---- CN shapes ------------------------------------------------------------------------------------------------------------
LOW = F32(0.02)


@lru_cache(maxsize=None)
def cn_shapes():
    """(name, float32 depths of one sex reference) per sample."""
    rng = np.random.default_rng(40)
    below, above = np.nextafter(LOW, ZERO32), np.nextafter(LOW, INF32)
    rest = lambda k: 0.25 + 0.125 * np.arange(k)                     # k distinct values well above 0.02
    out = [("no-tiles", []), ("zeros", np.zeros(10)), ("one-zero", [0]), ("one-value", [0.75]), ("one-low", [0.01]),
           ("lows-3-of-10", np.r_[[0.01, 0.005, 0.015], rest(7)]), ("lows-4-of-10", np.r_[[0.01, 0.005, 0.015, 0.012], rest(6)]),
           ("lows-3-of-10-zeros-count", np.r_[[0.01, 0.005, 0.015], rest(5), [0, 0]]),
           ("lows-4-of-10-zeros-count", np.r_[[0.01, 0.005, 0.015, 0.012], rest(4), [0, 0]]),
           ("lows-30-of-100", np.r_[0.001 + 0.0005 * np.arange(30), rest(70)]),
           ("lows-31-of-100", np.r_[0.001 + 0.0005 * np.arange(31), rest(69)]),
           ("all-low", np.r_[np.full(5, 0.01), np.zeros(5)]), ("all-low-no-zeros", 0.001 * np.arange(1, 8)),
           ("below-0.02", np.r_[[below] * 4, rest(6)]), ("at-0.02", np.r_[[LOW] * 4, rest(6)]),
           ("above-0.02", np.r_[[above] * 4, rest(6)]),
           ("around-0.02-3-lows", np.r_[[below, below, below, LOW, above], rest(5)]),
           ("around-0.02-4-lows", np.r_[[below, below, below, below, LOW, above], rest(4)]),
           ("interleaved", np.r_[np.c_[np.zeros(40), rest(40)].ravel(), 0]),
           ("interleaved-lows", np.c_[np.zeros(30), np.full(30, 0.01), rest(30)].ravel())]
    for n in (255, 256, 257):
        v = rng.uniform(0.03, 3, n)
        v[rng.integers(0, n, n // 10)] = 0
        out.append(("n%d" % n, v))
        v = v.copy()
        v[rng.permutation(n)[:n * 2 // 5]] = rng.uniform(0.001, 0.0199, n * 2 // 5)
        out.append(("n%d-lows" % n, v))
    # left = 1 .. 300 values behind the (possibly dropped) lows: rank int(left * 0.4) among distinct values, and with
    # the value at that rank repeated below it, above it, or on both sides
    for left in range(1, 301):
        k = int(float(left) * 0.4)
        for dup in ("", "-lo", "-hi", "-both"):
            v = (0.125 + np.arange(left) / 64).astype(F32)
            if dup in ("-lo", "-both") and k >= 1:
                v[k - 1] = v[k]
            if dup in ("-hi", "-both") and k + 1 < left:
                v[k + 1] = v[k]
            zeros = np.zeros(left % 3)
            lows = np.full(left if left % 5 == 0 else 0, 0.0078125)  # every fifth: as many lows again, dropped
            out.append(("left-%d%s" % (left, dup), rng.permutation(np.r_[v, zeros, lows])))
    out = [(name, np.asarray(v, np.float64).astype(F32)) for name, v in out]
    for _, v in out:
        v.setflags(write=False)
    return tuple(out)


def cn_model(d):
    """GetCN (indexcov.go:962-988) of one sample with sorted() and integers; returns (cn, facts).  The share
    lows / len(d) > 0.3 is Go's float64 comparison: both sides are taken as the exact values of their doubles."""
    tmp = sorted(float(x) for x in d if x != 0)
    lows = sum(1 for x in tmp if Fraction(x) < Fraction(float(LOW)))
    facts = {"n": len(d), "nonzero": len(tmp), "lows": lows, "dropped": False}
    if not tmp:
        return -0.1, facts
    share = _rne(Fraction(lows, len(d)), 53)
    facts["share_is_0.3"] = share == Fraction(0.3)
    if share > Fraction(0.3):
        tmp = tmp[lows:]
        facts["dropped"] = True
    facts["left"] = len(tmp)
    if not tmp:
        return 0.0, facts
    k = int(float(len(tmp)) * 0.4)
    facts["rank"], facts["dup_below"], facts["dup_above"] = k, k >= 1 and tmp[k - 1] == tmp[k], k + 1 < len(tmp) and tmp[k + 1] == tmp[k]
    return float(_rne(2 * Fraction(tmp[k]), 24)), facts


# ---- cell ties ------------------------------------------------------------------------------------------------------------
def tie_neighbourhood():
    """Every float32 in 1e-5 .. 5e4 that is a three-digit tie (d.dd5 x 10^e exactly) or the float32 next to one."""
    out = []
    for e in range(-5, 5):
        for d in range(100, 1000):
            tie = Fraction(2 * d + 1, 2) * Fraction(10) ** (e - 2)
            if tie > 50000:
                continue
            f = np.float32(float(tie))                       # a float32 beside the tie (or the tie itself)
            lo, hi = np.nextafter(f, np.float32(0)), np.nextafter(f, np.float32(np.inf))
            out += [lo, f, hi]
            if Fraction(float(f)) == tie:                    # representable: one more on each side
                out += [np.nextafter(lo, np.float32(0)), np.nextafter(hi, np.float32(np.inf))]
    return np.array(out, np.float32)


def notation_edges():
    """Where %.3g changes notation or the number of digits, with the float32 on each side (negative neighbours of 0
    left out)."""
    edge = [9.995e-5, 0.0001, 999.5, 1000, 50000, 0, 0.00099951, 0.001, 9.99e-5, 1e-5, 99.95, 100, 0.5, 1, 8, 1.15, 12.25,
            10.25, 122.5, 123.5, 1005, 10050, 49950, 999.49994, 999.50006]
    for x in list(edge):
        f = np.float32(x)
        edge += [np.nextafter(f, np.float32(0)), np.nextafter(f, np.float32(np.inf))]
    return [x for x in edge if x >= 0]


def tiny_quotients():
    """Small quotients down to the subnormals (the 134-bit product of gd3_scale_up) and a double that rounds to 0."""
    return [np.float32(1) / np.float32(3e30), np.float32(1e-38), np.float32(1.4e-45), np.float32(7e-45), np.float32(1.17549435e-38),
            np.float32(3.3e-33), np.float32(9.995e-31), np.float32(5e-324), np.float32(1e-20), np.float32(2.5e-12)]


@lru_cache(maxsize=None)
def cell_values():
    """float32: every tie with its neighbours, the notation edges, the tiny quotients, 50 000 with its two neighbours."""
    cap = F32(50000)
    v = np.concatenate([tie_neighbourhood(), np.array(notation_edges(), F32), np.array(tiny_quotients(), F32),
                        np.array([np.nextafter(cap, ZERO32), cap, np.nextafter(cap, INF32)], F32)])
    v.setflags(write=False)
    return v


# ---- threshold depths -----------------------------------------------------------------------------------------------------
SLOTS = 70
SLOT_C = Fraction(float(F32(F32(70) * F32(2.0 / 3.0))))             # slots * float32(slotsMid), one rounding
PCA_C = Fraction(float(F32(65535) / F32(8)))                        # 65535 / MaxCN = 8191.875
COUNTER_EDGES = (0.15, 0.85, 1.15, 8)                                # low, the band, MaxCN


def around(x, side=3):
    """The float32 nearest to each x and `side` float32 on each side of it."""
    c = np.asarray(x, np.float64).astype(F32)
    cols, lo, hi = [c], c, c
    for _ in range(side):
        lo, hi = np.nextafter(lo, ZERO32), np.nextafter(hi, INF32)
        cols += [lo, hi]
    return np.stack(cols, axis=1).ravel()


@lru_cache(maxsize=None)
def threshold_depths():
    """float32: seven values around every depth at which a slot (k - 0.5) / c, k = 1 .. 70, or a pca8 value
    (k - 0.5) / 8191.875, k = 1 .. 65 536, turns into the next, and around 0.15, 0.85, 1.15 and 8."""
    slot = [float((Fraction(2 * k - 1, 2)) / SLOT_C) for k in range(1, SLOTS + 1)]
    pca = (np.arange(1, 65537, dtype=np.float64) - 0.5) / float(PCA_C)
    v = np.concatenate([around(slot), around(pca), around(COUNTER_EDGES)])
    v.setflags(write=False)
    return v


def _rne(x, bits):
    """The non-negative rational x rounded to the nearest number of `bits` significant bits, ties to even (float32
    with bits = 24, float64 with 53; the values here are far from either format's subnormals)."""
    if x == 0:
        return Fraction(0)
    n, d = x.numerator, x.denominator
    e = n.bit_length() - d.bit_length()                              # floor(log2 x) is e or e - 1
    if (n << max(-e, 0)) < (d << max(e, 0)):
        e -= 1
    sh = e - (bits - 1)                                              # the unit in the last place is 2^sh
    num, den = (n, d << sh) if sh >= 0 else (n << -sh, d)
    q, r = divmod(num, den)
    if 2 * r > den or (2 * r == den and q & 1):
        q += 1
    return Fraction(q) * Fraction(2) ** sh


def _mul_add_int(d, c):
    """int(float32(float32(d * c) + 0.5)): the product and the sum rounded to float32 one after the other."""
    return int(_rne(_rne(Fraction(float(d)) * c, 24) + Fraction(1, 2), 24))


def slot_model(d):
    """tint(d * (slots * float32(slotsMid)) + 0.5) (indexcov.go:159-176)."""
    return min(_mul_add_int(d, SLOT_C), SLOTS - 1)


def byte_model(d):
    """uint8(65535 / MaxCN * min(d, MaxCN) + 0.5): the integer's low 8 bits (indexcov.go:694-698)."""
    return _mul_add_int(min(float(d), 8.0), PCA_C) & 0xff


def counter_model(d):
    """counter.count (indexcov.go:1064-1075) of one depth after the MaxCN cap: the index of out-low / out-only / hi / in
    as (out, low, hi, in) increments."""
    x = Fraction(min(float(d), 8.0))
    lo, a, b = (Fraction(float(F32(t))) for t in COUNTER_EDGES[:3])
    if x < a or x > b:
        return (1, 0, 1, 0) if x > b else (1, 1, 0, 0) if x < lo else (1, 0, 0, 0)
    return (0, 0, 0, 1)
