"""The cases of `debias --svd --log2` (tests/svdlog2_ref.py), built like tests/svddebias_shapes.py: Poisson depths whose rate
carries a few rank-one components of known strength, so that the cut of the spectrum is unambiguous, at the smallest sizes
where the device code changes path.

A case is (name, R, N, n, planted, depth): R rows, N samples, n the number of components the case wants removed, `planted`
rank-one components in the rate, `depth` the mean rate.  In log space the samples are centred, so there is no mean-depth
component: the planted ones lead.  pct is derived from the oracle's own spectrum (route (a)): half way between the shares of
s[n - 1] and s[n]; 0 when every value the cap allows is wanted.  The matrices, pct and the oracle's answer are built once
(case()) and shared.

SLAB is the rows of a Gram workgroup (gd_svddebias.hpp SV_SLAB), CS_SLAB the rows of a histogram workgroup's turn
(gd_colselect.hpp CS_SLAB: below it no whole slab is read, one row above it the tail follows a whole slab), 64 the Gram tile,
64 lanes x 1, 2, 4, 8, 16 the registers of the projection.  N covers 2, 3, 63, 64, 65, 128, 257, 1024; R covers 1, 2, 3,
CS_SLAB - 1, CS_SLAB, CS_SLAB + 1, SLAB - 1, SLAB, SLAB + 1, 3 SLAB + 7; n covers 0, 1, 3 and the cap (15, and N where that
is less).

LOW is the low-depth case (rate 1.5: most cells are 0, 1 or 2), where the projection carries zero cells above 0 and other
cells below it.  SELECT carries the columns that try the selection of the centres: SELECT_COLS.  Its half-empty column,
centred on 0, is a component of its own beside the three planted ones: n = 4 there."""
import functools

import numpy as np

from tests import svdlog2_ref as LR
from tests.svddebias_shapes import choose_pct, planted_matrix

SLAB = 1024
CS_SLAB = 64

#        name             R             N     n   planted depth
CASES = [
    ("n2_slab+1_all",     SLAB + 1,     2,    2,  1,  30),
    ("n2_two_rows",       2,            2,    1,  0,  30),
    ("n3_one_row",        1,            3,    0,  0,  30),
    ("n3_three_rows",     3,            3,    1,  0,  30),
    ("n63_slab-1",        SLAB - 1,     63,   3,  3,  30),
    ("n64_slab",          SLAB,         64,   3,  3,  30),
    ("n64_cs-1",          CS_SLAB - 1,  64,   1,  1,  100),
    ("n64_cs",            CS_SLAB,      64,   1,  1,  100),
    ("n65_cs+1",          CS_SLAB + 1,  65,   1,  1,  100),
    ("n65_slab+1",        SLAB + 1,     65,   3,  3,  30),
    ("n65_none",          500,          65,   0,  0,  30),
    ("n128_cap",          3 * SLAB + 7, 128,  15, 15, 400),
    ("n128_low",          SLAB + 1,     128,  1,  1,  1.5),
    ("n257_select",       3 * SLAB + 7, 257,  4,  3,  30),
    ("n1024",             1100,         1024, 3,  3,  30),
]
NAMES = [c[0] for c in CASES]
LOW = "n128_low"
SELECT = "n257_select"
# column -> what it tries (select_columns() writes them)
SELECT_COLS = {0: "all zeros", 64: "more than half zeros: the centre is 0", 130: "a long tie at the rank", 256: "the answer is in the last row"}


def select_columns(A, rng):
    R = A.shape[0]
    A[:, 0] = 0.0
    A[rng.permutation(R)[:R // 2 + 5], 64] = 0.0
    col = A[:, 130]
    lo, hi = np.sort(col)[[R // 4, 3 * R // 4]]
    col[(col >= lo) & (col <= hi)] = lo                                # half the column is one value, the rank in its middle
    v = np.sort(A[:-1, 256])
    v[:R // 2] = np.minimum(v[:R // 2], 30.0)
    v[R // 2:] = np.maximum(v[R // 2:], 31.0)
    A[:-1, 256] = rng.permutation(v)
    A[-1, 256] = 30.5                                                  # R // 2 cells are below it, and it is the only 30.5


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(A float32 [R][N], pct, n, out float32, out64, e, s, m): built once, never written to"""
    k = NAMES.index(name)
    _, R, N, n, planted, depth = CASES[k]
    A = planted_matrix(R, N, planted, depth, 2000 + k)
    if name == SELECT:
        select_columns(A, np.random.default_rng(77))
    s, _ = LR.SR.spectrum_svd(LR.scale(A.astype(np.float64))[0])
    pct = choose_pct(s, n, R, N) if s.any() else 50.0
    out, s, got, out64, e, m = LR.svd_log2(A, pct)
    assert got == n, (name, got, n, (100 * s / s.sum())[:17])
    if name == LOW:                              # conditions on the oracle alone
        assert (np.exp2(e) - 1.0 < 0).any(), "no cell is clamped to 0"
        assert (out64[A == 0] > 0).any(), "no zero cell comes out positive"
    for a in (A, out, out64, e, s, m):
        a.setflags(write=False)
    return dict(A=A, pct=float(pct), n=n, out=out, out64=out64, e=e, s=s, m=m)
