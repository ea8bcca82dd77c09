"""A restatement of dcnv's SampleMedians (dcnv/dcnv.go:108-125 of the reference) and of the scale factors this project
derives from them, in plain Python: what gd_sample_medians, `goleft-depth scales` and
`emdepth --normalize` are held to, bit for bit.

For one sample over all R rows: sort the column ascending; k is the number of leading zeros (-0.0 compares equal to 0
and counts); n = R - k; the "median" is sorted[k + int(0.65 * float64(n))] -- the 0.65 quantile of the non-zero depths.
The product is taken in float64 and truncated.  n = 0 (Go indexes an empty slice and panics) gives 0 here.

The factors are a definition of this project's, not the reference's: scale[s] = float32(float64(T) / float64(med[s])),
T = sorted(med)[N // 2] (the centre the reference's scalers use) unless a level is given."""
import numpy as np

QUANTILE = 0.65


def rank(k, n):
    """index into the sorted column"""
    return k + int(QUANTILE * float(n))


def column_median(col):
    """(median, non-zero count) of one column; the median keeps the column's type (a value of the column, or 0)"""
    col = np.asarray(col)
    s = np.sort(col, kind="stable")
    k = int(np.count_nonzero(s == 0))            # (depths are >= 0, so the zeros lead; -0.0 == 0)
    n = len(s) - k
    if n == 0:
        return col.dtype.type(0), 0
    return s[rank(k, n)], n


def sample_medians(matrix):
    """(med [N] of the matrix's dtype, nonzero uint64 [N]) of a [rows][N] matrix"""
    m = np.asarray(matrix)
    assert m.ndim == 2 and m.shape[0] >= 1
    med = np.zeros(m.shape[1], m.dtype)
    nz = np.zeros(m.shape[1], np.uint64)
    for s in range(m.shape[1]):
        med[s], nz[s] = column_median(m[:, s])
    return med, nz


def level_of(med):
    """T: the middle median"""
    return sorted(float(v) for v in med)[len(med) // 2]


def scales(med, level=None):
    """float32 [N]: float32(T / med[s]), the division in float64"""
    T = level_of(med) if level is None else float(level)
    assert all(float(v) > 0 for v in med)
    return np.array([np.float32(T / float(v)) for v in med], np.float32)


def scale_lines(scale):
    """what `goleft-depth scales` writes: %.9g of each float32"""
    return "".join("%.9g\n" % float(v) for v in scale)
