"""The cases of `debias --svd` (tests/svddebias_ref.py): Poisson depths whose rate carries a few rank-one components of known
strength, so that the cut of the spectrum is unambiguous, at the sizes where the device code changes path.

A case is (name, R, N, zscore, n, planted, depth): R rows, N samples, n the number of components the case wants removed,
`planted` rank-one components in the rate, `depth` the mean rate.  pct is derived from the oracle's own spectrum (route (a)):
half way between the shares of s[n - 1] and s[n]; 0 when every value the cap allows is wanted and none follows.  The
matrices, pct and the oracle's answer are built once (case()) and shared.

SLAB is the rows of a Gram workgroup (gd_svddebias.hpp SV_SLAB), 64 its tile, 64 lanes x 1, 2, 4, 8, 16 the registers of the
projection.  N covers 2, 3, 5, 63, 64, 65, 128, 257, 1024; R covers 1, N - 1, SLAB - 1, SLAB, SLAB + 1, 3 SLAB + 7."""
import functools

import numpy as np

from tests import svddebias_ref as SR

SLAB = 1024

#        name             R             N     z  n  planted depth
CASES = [
    ("n2_slab+1",         SLAB + 1,     2,    0, 1,  0,  30),
    ("n2_z",              7,            2,    1, 1,  0,  30),
    ("n3_rank",           2,            3,    0, 1,  0,  30),
    ("n3_one_row_z",      1,            3,    1, 1,  0,  30),
    ("n5_all",            300,          5,    0, 5,  2,  30),
    ("n5_rank_z",         4,            5,    1, 1,  1,  30),
    ("n16_cap_z",         SLAB,         16,   1, 15, 15, 400),
    ("n63_slab-1_z",      SLAB - 1,     63,   1, 3,  3,  30),
    ("n64_slab",          SLAB,         64,   0, 3,  2,  30),
    ("n64_none",          500,          64,   0, 0,  0,  30),
    ("n65_slab+1_z",      SLAB + 1,     65,   1, 3,  3,  30),
    ("n65_rank",          64,           65,   0, 1,  0,  30),
    ("n128_cap_z",        3 * SLAB + 7, 128,  1, 15, 15, 400),
    ("n128_rank_none_z",  127,          128,  1, 0,  0,  30),
    ("n200_z",            2000,         200,  1, 3,  3,  30),
    ("n257_3slab+7",      3 * SLAB + 7, 257,  0, 3,  2,  30),
    ("n257_rank_z",       256,          257,  1, 3,  3,  30),
    ("n1024_z",           1100,         1024, 1, 3,  3,  30),
]
NAMES = [c[0] for c in CASES]
# rows that are constants (sd == 0) and all-zero rows go into this one, at these rows
FLAT = "n200_z"
FLAT_ROWS = {0: 0.0, 5: 7.0, 6: 0.0, 1023: 31.0, 1024: 0.0, 1999: 12.0}


def planted_matrix(R, N, planted, depth, seed):
    """float32 [R][N]: Poisson counts of rate depth (1 + sum_k g u_k v_k^T), u and v uniform in [-1, 1]: the mean depth is
    the first component of the raw matrix, the planted ones follow, the counting noise is the rest"""
    rng = np.random.default_rng(seed)
    rate = np.ones((R, N))
    g = 0.9 / max(planted, 1) if planted > 3 else 0.3
    for k in range(planted):
        rate += g * (1.0 - 0.25 * k / max(planted, 1)) * np.outer(rng.uniform(-1, 1, R), rng.uniform(-1, 1, N))
    return rng.poisson(depth * rate).astype(np.float32)


def choose_pct(s, n, R, N):
    share = 100.0 * s / s.sum()
    cap = min(SR.MAX_REMOVED, R, N)
    if n == 0:
        return (share[0] + 100.0) / 2
    if n == cap and (n == len(s) or share[n] > 0.1):
        return 0.0
    return (share[n - 1] + share[n]) / 2


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(A float32 [R][N], pct, zscore, n, out float32, out64, s): built once, never written to"""
    k = NAMES.index(name)
    _, R, N, z, n, planted, depth = CASES[k]
    A = planted_matrix(R, N, planted, depth, 1000 + k)
    if name == FLAT:
        for r, v in FLAT_ROWS.items():
            A[r] = v
    A64 = A.astype(np.float64)
    s, _ = SR.spectrum_svd(SR.scale(A64)[0] if z else A64)
    pct = choose_pct(s, n, R, N)
    out, s, got, out64 = SR.svd_debias(A, pct, bool(z))
    assert got == n, (name, got, n, (100 * s / s.sum())[:17])
    for a in (A, out, out64, s):
        a.setflags(write=False)
    return dict(A=A, pct=float(pct), zscore=int(z), n=n, out=out, out64=out64, s=s)
