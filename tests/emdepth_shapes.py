"""The matrices the emdepth tests run, seeded, with their restatement results computed once a process.

CPU tests (tests/test_emdepth_ref.py) pin the quirks on the hand-made rows and assert the exclusion caps on every
matrix here; the GPU tests (tests/test_gpu_emdepth.py) run the same matrices through the C ABI.  Shapes follow the
kernel's structure (goleft_amd/csrc/gd_emdepth.hpp): 64 lanes a row, 4 rows a workgroup, rows of up to 256 samples
held in registers and longer ones re-read, at most 2048 workgroups a launch."""
import functools

import numpy as np

from tests import emdepth_ref as R

WAVES = 4                # rows of a workgroup (EM_WAVES)
GRID = 2048              # workgroups of a launch at most (EM_MAX_GRID)
REG_MAX = 256            # the longest row held in registers (EM_REG_MAX)
SAMPLE_COUNTS = (1, 3, 4, 5, 63, 64, 65, 127, 128, 129, 200, REG_MAX - 1, REG_MAX, REG_MAX + 1, 4096)
ROW_COUNTS = (1, WAVES - 1, WAVES, WAVES + 1)
STRIDE_ROWS = GRID * WAVES + 5                   # more rows than a launch holds at once: the stride loop turns
CHOICE = np.array([0, 0.5, 1, 1, 1, 1, 1.5, 2, 4])
GAP = 1e-9               # rows of general inputs are compared when every comparison they took is wider than this
CAP = 0.01               # ... and at most this share of rows, and of adjusted cells, may be left out


class Case:
    """kind 'f32': depths float32 [rows][n] for gd_emdepth; kind 'cells': int64 cells and a scale (or None) for
    gd_emdepth_cells ('cohort': the cells a real gd_depthwed_device must leave).  exact: bin sums are exact in any order (integers times one power of two): lambda bit for bit."""

    def __init__(self, kind, exact, depths=None, cells=None, scale=None):
        self.kind, self.exact, self.cells, self.scale = kind, exact, cells, scale
        self.depths = np.ascontiguousarray(depths if depths is not None else R.cells_to_depths(cells, scale), np.float32)


def integer_rows(seed, rows, n, lo=5.0, hi=60.0):
    """floor(Poisson(b) * choice{0, 1/2, 1, 1, 1, 1, 1 1/2, 2, 4}), b per row"""
    rng = np.random.default_rng(seed)
    b = rng.uniform(lo, hi, size=(rows, 1))
    return np.floor(rng.poisson(b, size=(rows, n)) * rng.choice(CHOICE, size=(rows, n)))


def float_rows(seed, rows, n):
    """arbitrary float32 depths: a row's level, times a copy-number factor, times 15 % noise.  Rows of fewer than 8
    samples get no factor: a bin of one value makes its centre that value, an exact tie in the next pass, and such a
    row would be left out."""
    rng = np.random.default_rng(seed)
    b = rng.uniform(5.0, 60.0, size=(rows, 1))
    f = rng.choice(CHOICE, size=(rows, n)) if n >= 8 else 1.0
    return (b * f * rng.lognormal(0.0, 0.15, size=(rows, n))).astype(np.float32)


def pow2_scales(seed, n):
    return (2.0 ** np.random.default_rng(seed).integers(-3, 4, size=n)).astype(np.float32)


def any_scales(seed, n, lo=0.5, hi=2.0):
    return np.random.default_rng(seed).uniform(lo, hi, size=n).astype(np.float32)


def _rows_for(n):
    return 2 if n > 1024 else WAVES + 1


# the hand-made rows: name -> depths
HAND = {
    "all_zero": [0.0] * 9,                                       # one pass, the fallback, NaN pmf: CN 0 everywhere
    "all_equal": [7.0] * 9,
    "above_lambda8": [0, 0, 0, 5, 0, 0, 0],                      # 5 among zeros: 9
    "on_a_centre": [30, 30, 30, 30, 30, 30, 30, 60, 15],         # lambda[2] = 30: 60 is lambda[4], 15 lambda[1] before widening
    "median_duplicates_even": [3, 3, 7, 7, 7, 7, 9, 9],          # b[4] = b[5] = 7
    "median_even_off_by_one": [5, 5, 5, 5, 9, 9],                # b[3] = 5, b[4] = 9: (5 + 9) / 2 = 7, not 5
    "median_straddle_odd": [4, 6, 6, 6, 8],
    "fallback_non_ascending": [0, 0, 1, 1000],                   # bin 2 empty twice: lambda[2] = eps, lambda[1] < lambda[0]
    "go_test_depth_1": [1, 8, 33, 34, 35, 37, 31, 22, 66],
    "go_test_big": [296.6, 16.7, 17.0, 3019.2, 14.4, 16.5, 14.2, 26, 7],
    "underflow_kept": [1e6] * 8 + [3.8e6],                       # both pmf values are exactly 0: the call is kept
    "single_sample": [12.5],
}

TEN_PASS_SEED, TEN_PASS_N = 11, 10               # see ten_pass_row()


@functools.lru_cache(maxsize=None)
def ten_pass_row():
    """The first row of the seeded even-N stream that runs all ten passes (found by the restatement itself)."""
    rows = integer_rows(TEN_PASS_SEED, 40000, TEN_PASS_N, 0.2, 30.0).astype(np.float32)
    for row in rows:
        lam, it = R.em_lambda([float(v) for v in row], R.Gap())
        if it == R.MAXITER:
            return row
    raise AssertionError("no ten-pass row in the stream")


@functools.lru_cache(maxsize=None)
def non_ascending_rows():
    """Rows of a seeded integer stream (6 samples, small depths) whose final lambda is not ascending: at least 20."""
    rows = integer_rows(7, 600, 6, 0.2, 3.0).astype(np.float32)
    keep = []
    for row in rows:
        lam, _ = R.em_lambda([float(v) for v in row], R.Gap())
        if any(lam[k] > lam[k + 1] for k in range(8)):
            keep.append(row)
    return np.array(keep, np.float32)


COHORT_W = 100                                   # window of the synthetic cohort, and the depthwed size
COHORT_LENGTHS = (2050, 1500)                    # two contigs; the first ends on a short window
COHORT_SAMPLES = (3, 5)


@functools.lru_cache(maxsize=None)
def cohort(n_samples):
    """A tiny cohort for a real gd_depthwed_device: (window sums [sample][contig], the depthwed cells [rows][samples] the
    reference's text chain gives for them).  Every sample sits at the window's level; with five samples the last one carries
    a copy-number factor (bin 2 keeps at least two values, so that no centre is a depth itself: such a row ties)."""
    from oracle import pyoracle as po
    rng = np.random.default_rng(600 + n_samples)
    sums = [[] for _ in range(n_samples)]
    for L in COHORT_LENGTHS:
        nw = (L + COHORT_W - 1) // COHORT_W
        start = np.arange(nw, dtype=np.int64) * COHORT_W
        wlen = np.minimum(start + COHORT_W, L) - start
        level = rng.poisson(rng.uniform(30.0, 60.0, size=(1, nw)), size=(n_samples, nw)).astype(np.float64)
        if n_samples >= 5:
            level[-1] = np.floor(level[-1] * rng.choice(CHOICE, size=nw))
        for s in range(n_samples):
            sums[s].append(level[s].astype(np.int64) * wlen)
    cells = np.array([np.concatenate([po.depthwed_cells_contig(sums[s][j], L, COHORT_W, COHORT_W)[0]
                                      for j, L in enumerate(COHORT_LENGTHS)]) for s in range(n_samples)]).T
    return sums, np.ascontiguousarray(cells, np.int64)


@functools.lru_cache(maxsize=None)
def cases():
    c = {}
    for name, row in HAND.items():
        c["hand_" + name] = Case("f32", name != "go_test_big", depths=np.array([row], np.float32))    # (its depths have fractions)
    c["hand_ten_passes"] = Case("f32", True, depths=ten_pass_row()[None, :])
    c["non_ascending"] = Case("f32", True, depths=non_ascending_rows())
    for n in SAMPLE_COUNTS:
        c["int_n%d" % n] = Case("f32", True, depths=integer_rows(100 + n, _rows_for(n), n))
        # (one sample: a bin of one value has no order of summation, and its centre always ties with the value)
        c["float_n%d" % n] = Case("f32", n == 1, depths=float_rows(200 + n, _rows_for(n), n))
    for rows in ROW_COUNTS:
        c["rows_%d" % rows] = Case("f32", True, depths=integer_rows(300 + rows, rows, 9))
    c["rows_stride"] = Case("f32", True, depths=integer_rows(310, STRIDE_ROWS, 3))
    c["deep_int"] = Case("f32", True, depths=integer_rows(320, 6, 65, 800.0, 850.0))         # lgamma of a large argument; no depth above 4096
    c["deep_float"] = Case("f32", False, depths=float_rows(321, 6, 65) * np.float32(12.0))
    for n in (5, 200, REG_MAX + 1):
        cells = integer_rows(400 + n, 7, n).astype(np.int64)
        c["cells_n%d" % n] = Case("cells", True, cells=cells)
        c["cells_pow2_n%d" % n] = Case("cells", True, cells=cells, scale=pow2_scales(410 + n, n))
        c["cells_scaled_n%d" % n] = Case("cells", False, cells=cells, scale=any_scales(415 + n, n))
    for n in COHORT_SAMPLES:
        cells = cohort(n)[1]
        c["cohort_n%d" % n] = Case("cohort", True, cells=cells)
        c["cohort_pow2_n%d" % n] = Case("cohort", True, cells=cells, scale=pow2_scales(610 + n, n))
        c["cohort_scaled_n%d" % n] = Case("cohort", False, cells=cells, scale=any_scales(620 + n, n, 0.9, 1.1))      # (3 samples spread further apart leave one value in bin 2)
    return c


CLI_SCALES = (1.0, 0.5, 2.0, 1.25, 0.8, 1.0, 1.5, 1.0, 0.9)      # as the --scales file spells them


def cli_cells():
    """The 9-sample, 40-row integer matrix of the command-line tests."""
    return integer_rows(500, 40, 9).astype(np.int64)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The restatement's rows of a case, computed once."""
    return R.em_matrix(cases()[name].depths)


def plan(case, rows):
    """What of a case is compared: (row mask, excluded cells {(row, sample)}, adjusted cell count).  Exact cases compare
    every row; general ones the rows whose comparisons are all wider than GAP.  A cell is left out when its adjustCN
    comparison was taken with the two sides within 1e-9 relative or next to the underflow edge."""
    keep = np.array([case.exact or r.gap > GAP for r in rows])
    out, adjusted = set(), 0
    for i, r in enumerate(rows):
        if not keep[i]:
            continue
        adjusted += len(r.pairs)
        out |= {(i, s) for s, (a, b) in r.pairs.items() if R.pair_excluded(a, b)}
    return keep, out, adjusted


def within_caps(keep, out, adjusted):
    return (~keep).sum() <= CAP * len(keep) and len(out) <= CAP * adjusted
