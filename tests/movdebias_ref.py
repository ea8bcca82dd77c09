"""The moving-median debias gd_moving_debias serves, restated from dcnv's GeneralDebiaser
(dcnv/debiaser/debiaser.go:98-123 of the reference) in numpy.  Two forms: `debias`, the closed form the kernel is built
on, and `literal_column`, a transcription of the Go loop push by push; tests/test_movdebias_ref.py holds one to the other.

What the Go code fixes, kept (line numbers of debiaser.go):
  :105      mid = (W - 1) / 2 + 1
  :106-108  the first mid values of the sorted column are pushed, :109-111 the first mid rows divided by one median
  :114-117  row i in [mid, R - mid) pushes col[i + mid] and is divided by the median after that push: the values of rows
            mid .. 2 mid - 1 are never pushed, the window of row i is not centred on it, and R - mid values are pushed in all
  :118-120  the last mid rows share the last median
  :110      the divisor is max(median, 1)
What it does not fix, defined here:
  the order  ascending covariate, tied covariates by row index (floats.Argsort, :60, is unstable there)
  the median of fewer than W values (the moving-median library is not part of the reference: its answer before the window
             is full is unread): (sorted[(m - 1) / 2] + sorted[m / 2]) / 2 in float64.  A full window of an odd W has one
             middle value, whatever the library does.
The pushed values count as keys: -0.0 is 0.0 there (a median is never -0.0); the dividend keeps its sign bit."""
import numpy as np

E_INVALID, E_RANGE = -1, -5
MAX_WINDOW = 255
MAX_SAMPLES = 4096


class Refused(Exception):
    def __init__(self, code, why):
        super().__init__(why)
        self.code = code


def mid_of(window):
    return (window - 1) // 2 + 1


def order_of(vals):
    """the rows in ascending covariate order, ties by row index"""
    return np.argsort(np.asarray(vals, np.float64), kind="stable")


def pushed(c, window):
    """P: c[0 .. mid), then c[2 mid ..) (debiaser.go:106-108, :115)"""
    mid = mid_of(window)
    return np.concatenate([c[:mid], c[2 * mid:]])


def window_of(i, rows, window):
    """(lo, hi): row i of the sorted column is divided by the median of P[lo .. hi)"""
    mid = mid_of(window)
    hi = mid if i < mid else min(i + 1, max(mid, rows - mid))
    return max(0, hi - window), hi


def median_of(w, window):
    """the median of the values of one window (of every column, when w is [m][n]), float64"""
    s = np.sort(np.asarray(w, np.float64), axis=0)
    m = len(s)
    if m == window:
        return s[(window - 1) // 2]
    return (s[(m - 1) // 2] + s[m // 2]) / 2.0


def check(depths, vals, window):
    d = np.asarray(depths)
    if d.ndim != 2:
        raise Refused(E_INVALID, "a matrix")
    rows, n = d.shape
    if n < 1 or n > MAX_SAMPLES:
        raise Refused(E_RANGE, "1 .. 4096 samples")
    if window < 1 or window > MAX_WINDOW or window % 2 == 0:
        raise Refused(E_RANGE, "an odd window of 1 .. 255")
    if rows < mid_of(window) or rows > 2 ** 31 - 1:
        raise Refused(E_RANGE, "at least (W - 1) / 2 + 1 rows (debiaser.go:107 indexes past the column otherwise)")
    if not np.all(np.isfinite(vals)):
        raise Refused(E_INVALID, "a covariate is not finite")
    if not (np.all(np.isfinite(d)) and np.all(d >= 0)):
        raise Refused(E_INVALID, "a depth is not a finite number >= 0")


def debias_column(c, window):
    """one sorted column, float32 (or [rows][n]: every column) -> (out float32, med float64: the divisors before the max)"""
    c = np.asarray(c, np.float32)
    rows = len(c)
    P = np.abs(pushed(c, window)).astype(np.float64)             # (abs: -0.0 as the key 0.0; nothing else is negative)
    med = np.empty(c.shape, np.float64)
    last = None
    for i in range(rows):
        w = window_of(i, rows, window)
        if w != last:
            m = median_of(P[w[0]:w[1]], window)
            last = w
        med[i] = m
    with np.errstate(over="ignore"):
        out = (c.astype(np.float64) / np.maximum(med, 1.0)).astype(np.float32)
    return out, med


def debias(depths, vals, window):
    """-> (out float32 [rows][n], med float64 [rows][n]), both at the rows' original places"""
    check(depths, vals, window)
    d = np.ascontiguousarray(depths, np.float32)
    order = order_of(vals)
    out = np.empty(d.shape, np.float32)
    med = np.empty(d.shape, np.float64)
    out[order], med[order] = debias_column(d[order], window)
    return out, med


def literal_column(c, window):
    """debiaser.go:104-120 line by line on one sorted column: a ring of W values fed push by push, the median of whatever
    it holds.  -> (out float32, med float64)"""
    col = np.asarray(c, np.float32).astype(np.float64)
    rows = len(col)
    ring, at = [], 0

    def push(v):
        nonlocal at
        v = abs(v)
        if len(ring) < window:
            ring.append(v)
        else:
            ring[at] = v
            at = (at + 1) % window

    def median():
        return median_of(ring, window)

    out = col.copy()
    med = np.empty(rows, np.float64)
    mid = (window - 1) // 2 + 1                                   # :105
    for i in range(mid):                                          # :106
        push(col[i])
    for i in range(mid):                                          # :109
        med[i] = median()
        out[i] = col[i] / max(med[i], 1.0)
    i = mid
    while i < rows - mid:                                         # :114
        push(col[i + mid])
        med[i] = median()
        out[i] = col[i] / max(med[i], 1.0)
        i += 1
    while i < rows:                                               # :118
        med[i] = median()
        out[i] = col[i] / max(med[i], 1.0)
        i += 1
    with np.errstate(over="ignore"):
        return out.astype(np.float32), med


def text(out):
    """the cells as the command line prints them: %.9g of the float32"""
    return [["%.9g" % float(x) for x in row] for row in out]
