"""A plain restatement of the reference's emdepth.EMDepth, for the tests alone (nothing under goleft_amd/ imports it).

Written from reading emdepth/emdepth.go and emdepth/stats.go of goleft; the line numbers below are that file's.  Python
floats are IEEE float64 and nothing here is fused, so the arithmetic on the centres is the reference's operation by
operation; numpy.float32 does the narrowing.  Kept quirk for quirk:

  * median32 (:18-29) of an even row is (b[N/2] + b[N/2 + 1]) / 2 -- one place to the right of the middle pair -- and
    indexes past the end for N = 2 (Go panics; em_row raises);
  * sort.SearchFloat64s (:161, :274) is a binary search over centres that are not always ascending;
  * the fallback (:181-192) clamps lambda[i] to eps for i = 1 .. 7 in order, lambda[2] included, before adding to it;
  * Type (:278-279) answers 9 = len(Lambda) above lambda[8]; the reference's own unit test expects 8 there
    (emdepth_test.go:31).  No Go toolchain was at hand: the code as written is followed.

Besides the results, em_row returns what decides how far a device result may be compared: the smallest relative gap
|a - b| / max(|a|, |b|) over every strict comparison the row took (classification, lambda[2] == 0, the two convergence
tests, Type's search), and per adjusted cell the pair (0.9 * pmf(k, lambda[cn]), pmf(k, lambda[2]))."""
import math

import numpy as np

EPS = 0.01
MAX_CN = 8
MAXITER = 10
INF = float("inf")


class Gap:
    """The smallest relative gap of the comparisons seen; a comparison of two equal values counts as 0."""

    def __init__(self):
        self.min = INF

    def see(self, a, b):
        m = max(abs(a), abs(b))
        g = abs(a - b) / m if m > 0 else 0.0
        if g < self.min:
            self.min = g

    def lt(self, a, b):
        self.see(a, b)
        return a < b

    def gt(self, a, b):
        self.see(a, b)
        return a > b

    def ge(self, a, b):
        self.see(a, b)
        return a >= b


def median32(a):
    """:18-29"""
    b = sorted(float(v) for v in a)
    n = len(b)
    if n % 2 == 1:
        return b[n // 2]
    return (b[n // 2] + b[n // 2 + 1]) / 2        # IndexError for N = 2, as Go panics


def search(lam, d, gap):
    """sort.SearchFloat64s: the smallest index the binary search reaches with lam[h] >= d"""
    i, j = 0, len(lam)
    while i < j:
        h = (i + j) >> 1
        if gap.ge(lam[h], d):
            j = h
        else:
            i = h + 1
    return i


def mean64(total, n):
    return total / n if n else 0.0


def bin_of(lam, d, gap):
    """:152-176"""
    if gap.gt(d, lam[1]) and gap.lt(d, lam[3]):
        a2 = abs(d - lam[2])
        if gap.lt(a2, abs(d - lam[1])) and gap.lt(a2, abs(d - lam[3])):
            return 2
    idx = search(lam, d, gap)
    if idx == 0:
        return 0
    if idx == len(lam):
        return idx - 1
    return idx if gap.lt(abs(d - lam[idx]), abs(d - lam[idx - 1])) else idx - 1


def em_lambda(depths, gap):
    """EMDepth (:117-206): (lambda, passes run).  depths: float32 values as Python floats."""
    m = median32(depths)
    lam = [0.0] * (MAX_CN + 1)
    last = [0.0] * (MAX_CN + 1)
    lam[0], lam[2] = EPS * m, m
    last[0] = lam[0]
    for i in range(1, len(lam)):
        if i != 2:
            lam[i] = lam[2] * math.pow(i / 2, 1.1)
    sumd, maxd = 100.0, 100.0
    it = 0
    while it < MAXITER and gap.gt(sumd, EPS) and gap.gt(maxd, 0.5):
        for i in range(1, len(lam)):
            last[i] = lam[i]
        sums = [0.0] * len(lam)
        cnts = [0] * len(lam)
        for d in depths:                         # (in the reference's order: bin by bin, sample by sample)
            b = bin_of(lam, d, gap)
            sums[b] += d
            cnts[b] += 1
        lam[2] = mean64(sums[2], cnts[2])
        if lam[2] == 0:
            n = float(len(depths))
            for i in range(1, len(lam) - 1):
                pdepth = cnts[i] / n
                if lam[i] < EPS:
                    lam[i] = EPS
                lam[2] += mean64(sums[i], cnts[i]) * (2 / float(i)) * pdepth
        else:
            gap.see(lam[2], 0.0)
        for i in range(1, len(lam)):
            lam[i] = lam[2] * (float(i) / 2)
        span = lam[2] - lam[1]
        lam[1] -= span / 1.5
        lam[3] += span / 1.5
        sumd, maxd = 0.0, 0.0
        for i in range(len(lam)):
            d = abs(lam[i] - last[i])
            sumd += d
            if d > maxd:
                maxd = d
        it += 1
    return lam, it


def pmf(k, mu):
    """stats.go:14-23 (the table of the first 1000 values holds what Lgamma returns)"""
    lg = math.lgamma(k + 1.0)
    log_mu = math.log(mu) if mu > 0 else -INF    # (Go: Log(0) = -Inf)
    return math.exp(k * log_mu - lg - mu)        # 0 * -inf = NaN, and exp(NaN) = NaN


def type_of(lam, d, gap):
    """Type + adjustCN (:272-304): (cn, None) or (cn, (0.9 * pmf_cn, pmf_2)) when the comparison was taken"""
    idx = search(lam, d, gap)
    if idx == 0:
        cn = 0
    elif idx == len(lam):
        cn = len(lam)                            # 9
    else:
        cn = idx if gap.lt(abs(d - lam[idx]), abs(d - lam[idx - 1])) else idx - 1
    if cn != 2 and cn < len(lam):
        k = int(0.5 + d)
        o, o2 = pmf(k, lam[cn]), pmf(k, lam[2])
        a = o * 0.9
        if a < o2:
            cn = 2
        return cn, (a, o2)
    return cn, None


def log2fc(lam, d):
    """:256, narrowed to float32"""
    if d == 0:
        return np.float32(-INF)                  # (Go: Log2(0) = -Inf; lambda[2] is never 0 after a pass)
    return np.float32(math.log2(d / lam[2]))


class Row:
    __slots__ = ("lam", "iters", "cn", "log2fc", "gap", "pairs")


def em_row(depths):
    """One row: depths are narrowed to float32 first.  Returns a Row: lam (list of 9 floats), iters, cn (list),
    log2fc (float32 array), gap (smallest relative comparison gap), pairs ({sample: (0.9 * pmf_cn, pmf_2)})."""
    d32 = np.asarray(depths, dtype=np.float32)
    if d32.ndim != 1 or d32.size == 0 or d32.size == 2:
        raise ValueError("emdepth: the reference cannot take the median of %d values" % d32.size)
    ds = [float(v) for v in d32]
    gap = Gap()
    r = Row()
    r.lam, r.iters = em_lambda(ds, gap)
    r.cn, r.pairs = [], {}
    for s, d in enumerate(ds):
        cn, pair = type_of(r.lam, d, gap)
        r.cn.append(cn)
        if pair is not None:
            r.pairs[s] = pair
    r.log2fc = np.array([log2fc(r.lam, d) for d in ds], dtype=np.float32)
    r.gap = gap.min
    return r


def em_matrix(depths):
    """Rows of a [rows][samples] matrix."""
    return [em_row(row) for row in np.asarray(depths, dtype=np.float32)]


def cells_to_depths(cells, scale=None):
    """What gd_emdepth_cells makes of int64 cells: (float32)cell, then * scale[s] in float32: one rounding each."""
    d = np.asarray(cells, dtype=np.int64).astype(np.float32)
    if scale is not None:
        d = d * np.asarray(scale, dtype=np.float32)[None, :]
    return d.astype(np.float32)


def pair_excluded(a, b):
    """A cell whose adjustCN comparison a device may decide the other way: the two sides within 1e-9 relative, or next to
    the underflow edge.  Both exactly 0, or a NaN, compare the same everywhere."""
    if math.isnan(a) or math.isnan(b) or (a == 0 and b == 0):
        return False
    m = max(a, b)
    return m < 1e-290 or abs(a - b) <= 1e-9 * m
