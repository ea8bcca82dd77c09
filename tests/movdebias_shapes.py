"""The shapes tests/test_gpu_movdebias.py runs gd_moving_debias on: the smallest that reach each structural edge of the
kernel as built (goleft_amd/csrc/gd_movdebias.hpp).

  columns    a workgroup (one wave) owns 64 columns, one per lane (MD_COLS): 1, 63, 64, 65, 200 samples, and 4096 with few rows
  segments   a workgroup owns SEGMENT sorted positions and starts by loading the at most W pushed rows before its first:
             256 of them for W <= 63, 1024 above.  Rows one fewer and one more than a segment put a seam inside a window;
             two segments and a bit put a whole segment behind a seam
  batches    rows are loaded eight steps at a time (MD_BATCH), the window before a segment too: rows and windows of 7, 8, 9
  windows    the ring has room for 15, 63 or 255 values (three instances): W = 15 | 17 and 63 | 65 are the boundaries;
             W = 1 (mid = 1: a row is divided by the next row's value), 3, 9 (what dcnv runs), 255 (the largest)
  rows       mid (the fewest; one partial window), 2 mid - 1 (nothing is pushed after the first mid), 2 mid, 2 mid + 1 (the
             first push of the second loop), W - 1, W, W + 1 (the first full window, the first value to leave it)
  order      the covariate random, descending (the permutation reverses the rows), ascending, and heavily tied"""
import numpy as np

COLS, BATCH = 64, 8
CAPS = (15, 63, 255)
SEG_SMALL, SEG_BIG = 256, 1024
WINDOWS = (1, 3, 9, 15, 17, 63, 65, 255)
SAMPLE_COUNTS = (1, 63, 64, 65, 200)


def mid_of(W):
    return (W - 1) // 2 + 1


def segment_of(W):
    return SEG_SMALL if W <= CAPS[1] else SEG_BIG


def edge_rows(W):
    mid = mid_of(W)
    return sorted({r for r in (mid, 2 * mid - 1, 2 * mid, 2 * mid + 1, W - 1, W, W + 1, W + BATCH + 1) if r >= mid})


def seam_rows(W):
    s = segment_of(W)
    return (s - 1, s, s + 1, 2 * s + 3)


def float_matrix(seed, rows, n):
    """any finite float32 >= 0 as its bit pattern (denormals included), a third of the cells zero, some of them -0.0"""
    rng = np.random.default_rng(seed)
    m = rng.integers(0, 0x7f800000, size=(rows, n), dtype=np.int64).astype(np.uint32).view(np.float32).copy()
    z = rng.random((rows, n))
    m[z < 0.33] = 0.0
    m[z < 0.05] = -0.0
    return m


def depth_matrix(seed, rows, n):
    """depths as a cohort has them: integers around a sample's level (many duplicates in a window), some zero, and a
    sample whose level is below 1 (its divisor is 1)"""
    rng = np.random.default_rng(seed)
    m = rng.poisson(rng.uniform(5.0, 300.0, size=(1, n)), size=(rows, n)).astype(np.float32)
    m[rng.random((rows, n)) < 0.2] = 0.0
    m[:, 0] = (rng.random(rows) * 0.9).astype(np.float32)
    return m


def vals_of(kind, seed, rows):
    rng = np.random.default_rng(seed)
    if kind == "random":
        return rng.normal(0.41, 0.05, rows)
    if kind == "tied":
        return np.round(rng.normal(0.41, 0.05, rows), 2)
    if kind == "reversed":
        return -np.arange(rows, dtype=np.float64)
    if kind == "sorted":
        return np.arange(rows, dtype=np.float64)
    raise ValueError(kind)
