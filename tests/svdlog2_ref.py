"""The definition of `debias --svd --log2` in numpy float64: dcnv's SVD debiaser (dcnv/debiaser/
debiaser.go:173-200 of the reference) flanked by its Log2 scaler (dcnv/scalers/scalers.go:134-164, through
ColCentered{gmean}, :63-100 and :126-132).  The oracle of tests/test_gpu_svdlog2*.py.

A is [R][N] float32, every cell finite and >= 0, taken to float64.  2 <= N <= 1024, 1 <= R < 2^31.
  1. l_ij = log2(1 + a_ij).
  2. c_j = sorted(l_.j)[R // 2]: the upper median over ALL R cells of sample j, zeros included (gmean; its second return is
     dead code).  log2 is monotone, so c_j = log2(1 + m_j) with m_j the R // 2-th smallest raw cell: centre_cells().
  3. z_ij = l_ij - c_j.
  4. s, the cut n and the projection are steps 2-4 of tests/svddebias_ref.py on Z: the cap is min(15, R, N), an all-zero Z
     removes nothing.
  5. out_ij = max(0, 2^(z'_ij + c_j) - 1), narrowed to float32 with one rounding.

The "- 1" and the clamp of step 5 are this project's definition.  The reference's UnScale returns 2^x (:155-163), so a round
trip gives depth + 1, and the reference's own TestLog2RoundTrip (scalers_test.go:49-79), which wants the input back within
0.001, fails on it: the test's contract is served, not the code's result.  The clamp is ZScore.UnScale's max(0, .): a zero
cell can come out of the projection with a negative exponent.

Two routes to s and V, as in svddebias_ref: (a) numpy.linalg.svd(Z); (b) eigh(Z^T Z), the one the device takes."""
import numpy as np

from tests import svddebias_ref as SR


def centre_cells(A32):
    """m_j float32 [N]: the R // 2-th smallest raw cell of every column"""
    A32 = np.asarray(A32, np.float32)
    return np.sort(A32, axis=0, kind="stable")[A32.shape[0] // 2].copy()


def scale(A):
    """(Z, c) of steps 1-3; A float64 [R][N]; c by sorting the logs, as the reference does"""
    L = np.log2(1.0 + A)
    c = np.sort(L, axis=0, kind="stable")[A.shape[0] // 2]
    return L - c[None, :], c


def svd_log2(A32, pct, route="svd"):
    """(out float32 [R][N], s float64 [min(R, N)], n, out64: out before the narrowing, e: the exponent z' + c, m: centre_cells)"""
    A32 = np.asarray(A32, np.float32)
    assert A32.ndim == 2 and A32.shape[0] >= 1 and A32.shape[1] >= 2
    assert np.isfinite(A32).all() and (A32 >= 0).all()
    A = A32.astype(np.float64)
    R, N = A.shape
    Z, c = scale(A)
    s, V = (SR.spectrum_svd if route == "svd" else SR.spectrum_gram)(Z)
    n = SR.cut(s, pct, R, N)
    Vn = V[:, :n]
    e = (Z - (Z @ Vn) @ Vn.T) + c[None, :]
    out64 = np.maximum(0.0, np.exp2(e) - 1.0)
    return out64.astype(np.float32), s, n, out64, e, centre_cells(A32)
