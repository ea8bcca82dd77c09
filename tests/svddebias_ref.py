"""The definition of `debias --svd` in numpy float64: dcnv's SVD debiaser (dcnv/debiaser/
debiaser.go:173-200 of the reference) flanked by its z-score scaler (dcnv/scalers/scalers.go:24-56).  The oracle of
tests/test_gpu_svddebias*.py.

A is [R][N] float32, every cell finite and >= 0, taken to float64.
  1. zscore: m_i = sum_j a_ij / N, sd_i the sample standard deviation (N - 1, two-pass: gonum's stat.MeanStdDev),
     z_ij = (a_ij - m_i) / sd_i, and z_ij = 0 for the whole row when sd_i == 0 (the project's choice: the reference gets NaN
     there and its factorisation panics).  Without zscore Z = A.
  2. s: the singular values of Z, descending, min(R, N) of them.
  3. n: the first index where 100 s[n] / sum(s) > pct fails, at most min(15, R, N) (the reference stops at 15 and indexes
     past the end of fewer; the cap at what there is is ours).  An all-zero Z gives 0 / 0, the compare is false, n = 0.
  4. Z' = Z - (Z V_n) V_n^T, V_n the first n right singular vectors: the reference's U Sigma' V^T.
  5. zscore only: out_ij = max(0, z'_ij sd_i + m_i) (ZScore.UnScale).
  6. out is narrowed to float32 with one rounding.

Two routes to s and V: (a) numpy.linalg.svd(Z); (b) eigh(Z^T Z), s = sqrt(max(w, 0)) -- the route the device takes.
tests/test_svddebias_ref.py holds them together on every case."""
import numpy as np

MAX_REMOVED = 15


def scale(A):
    """(Z, m, sd) of step 1; A float64 [R][N], N >= 2"""
    N = A.shape[1]
    m = A.sum(axis=1) / N
    d = A - m[:, None]
    sd = np.sqrt((d * d).sum(axis=1) / (N - 1))
    Z = np.zeros_like(A)
    ok = sd > 0
    Z[ok] = d[ok] / sd[ok, None]
    return Z, m, sd


def spectrum_svd(Z):
    """route (a): (s [min(R, N)], V [N][min(R, N)])"""
    _, s, vt = np.linalg.svd(Z, full_matrices=False)
    return s, vt.T


def spectrum_gram(Z):
    """route (b): the same from the eigenpairs of Z^T Z"""
    w, v = np.linalg.eigh(Z.T @ Z)
    order = np.argsort(-w, kind="stable")
    L = min(Z.shape)
    return np.sqrt(np.maximum(w[order], 0.0))[:L], v[:, order][:, :L]


def cut(s, pct, R, N):
    """step 3"""
    total = s.sum()
    n = 0
    with np.errstate(invalid="ignore", divide="ignore"):
        while n < min(MAX_REMOVED, R, N) and 100.0 * s[n] / total > pct:
            n += 1
    return n


def svd_debias(A32, pct, zscore, route="svd"):
    """(out float32 [R][N], s float64 [min(R, N)], n, out64: out before step 6)"""
    A32 = np.asarray(A32, np.float32)
    assert A32.ndim == 2 and A32.shape[0] >= 1 and A32.shape[1] >= 2
    assert np.isfinite(A32).all() and (A32 >= 0).all()
    A = A32.astype(np.float64)
    R, N = A.shape
    Z, m, sd = scale(A) if zscore else (A, None, None)
    s, V = (spectrum_svd if route == "svd" else spectrum_gram)(Z)
    n = cut(s, pct, R, N)
    Vn = V[:, :n]
    out64 = Z - (Z @ Vn) @ Vn.T
    if zscore:
        out64 = np.maximum(0.0, out64 * sd[:, None] + m[:, None])
    return out64.astype(np.float32), s, n, out64
