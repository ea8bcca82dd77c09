"""CPU: the oracle of `debias --svd` (tests/svddebias_ref.py) against itself.  Every case of tests/svddebias_shapes.py has a
cut that no rounding moves and a removed subspace that is well conditioned, and the two routes -- numpy.linalg.svd(Z) and
eigh(Z^T Z), the one the device takes -- agree on it within 2^-42 of the row's largest depth per cell (measured between
them on planted matrices: <= 1.5e-14 of the row maximum; 2^-42 = 2.3e-13 leaves 15x).  Then the definitions the reference
does not give: the row whose sd is 0, the all-zero matrix, the cap of 15 and of N."""
import numpy as np
import pytest

from tests import svddebias_ref as SR
from tests import svddebias_shapes as SS


@pytest.mark.parametrize("name", SS.NAMES)
def test_the_cut_is_unambiguous_and_the_routes_agree(name):
    c = SS.case(name)
    A, s, n, pct = c["A"], c["s"], c["n"], c["pct"]
    share = 100.0 * s / s.sum()
    if n > 0:
        assert abs(share[n - 1] - pct) >= 0.05, (name, share[n - 1], pct)
    if n < len(s):
        assert abs(share[n] - pct) >= 0.05, (name, share[n], pct)
        if n > 0:
            assert (s[n - 1] - s[n]) / s[0] >= 0.01, (name, s[n - 1], s[n], s[0])
    out_b, s_b, n_b, out64_b = SR.svd_debias(A, pct, bool(c["zscore"]), route="gram")
    assert n_b == n
    bound = 2.0 ** -42 * A.astype(np.float64).max(axis=1, keepdims=True)
    err = np.abs(out64_b - c["out64"])
    print(name, "routes differ by", float((err / np.maximum(bound * 2.0 ** 42, 1e-300)).max()), "of the row maximum")
    assert (err <= bound).all(), (name, float((err - bound).max()))
    big = s > 2.0 ** -20 * s[0]
    assert (np.abs(s_b - s)[big] <= 2.0 ** -36 * s[0]).all() and (np.abs(s_b - s)[~big] <= 2.0 ** -20 * s[0]).all()


def test_every_size_and_kind_of_case_is_there():
    Ns = {c[2] for c in SS.CASES}
    assert Ns >= {2, 3, 5, 63, 64, 65, 128, 257, 1024}
    S = SS.SLAB
    assert sum(c[2] == 1024 for c in SS.CASES) == 1
    Rs = {c[1] for c in SS.CASES}
    assert Rs >= {1, S - 1, S, S + 1, 3 * S + 7} and any(c[1] == c[2] - 1 for c in SS.CASES)
    assert max(Rs) <= 4000
    assert {c[3] for c in SS.CASES} == {0, 1}
    assert {c[4] for c in SS.CASES} >= {0, 1, 3, 15} and any(c[4] == c[2] == 5 for c in SS.CASES)
    assert any(c[4] == 15 and c[2] >= 16 for c in SS.CASES)


def s_top_share(A):
    s = np.linalg.svd(A.astype(np.float64), compute_uv=False)
    return s[0] / s.sum()


def test_a_row_without_spread_scales_to_zero_and_comes_out_unchanged():
    c = SS.case(SS.FLAT)
    Z, m, sd = SR.scale(c["A"].astype(np.float64))
    for r, v in SS.FLAT_ROWS.items():
        assert sd[r] == 0 and m[r] == v and not Z[r].any()
        assert (c["out"][r] == np.float32(v)).all()
    assert np.isfinite(c["out"]).all() and c["n"] == 3
    # the same rows without the z-score are ordinary rows
    out, s, n, _ = SR.svd_debias(c["A"], 50.0 * s_top_share(c["A"]), False)
    assert n == 1 and np.isfinite(out).all()


def test_a_constant_row_is_unchanged_under_zscore_whatever_is_removed():
    A = SS.planted_matrix(40, 9, 2, 30, 5).copy()
    A[11] = 23.0
    for pct in (0.0, 5.0, 99.0):
        out, _, _, _ = SR.svd_debias(A, pct, True)
        assert (out[11] == np.float32(23.0)).all()


def test_an_all_zero_matrix_removes_nothing():
    for z in (False, True):
        for route in ("svd", "gram"):
            out, s, n, _ = SR.svd_debias(np.zeros((6, 4), np.float32), 0.0, z, route=route)
            assert n == 0 and not s.any() and not out.any() and len(s) == 4


def test_the_cap_of_15_and_of_what_there_is():
    rng = np.random.default_rng(3)
    A = rng.poisson(30, (40, 20)).astype(np.float32)
    assert SR.svd_debias(A, 0.0, False)[2] == 15             # the reference's 15
    A = rng.poisson(30, (40, 4)).astype(np.float32)
    out, s, n, _ = SR.svd_debias(A, 0.0, False)              # the reference indexes s[4] here
    assert n == 4 and len(s) == 4 and np.abs(out).max() < 1e-4
    A = rng.poisson(30, (3, 20)).astype(np.float32)
    out, s, n, _ = SR.svd_debias(A, 0.0, False)
    assert n == 3 and len(s) == 3
    # (z-scored rows sum to zero, so the last singular value is 0 up to rounding: a share of 0 is no unambiguous cut there,
    # and no case of tests/svddebias_shapes.py asks for one)
    s = SR.svd_debias(rng.poisson(30, (40, 4)).astype(np.float32), 50.0, True)[1]
    assert s[3] <= 1e-12 * s[0]


def test_removing_is_a_projection():
    c = SS.case("n64_slab")
    A = c["A"].astype(np.float64)
    _, V = SR.spectrum_svd(A)
    Vn = V[:, :c["n"]]
    assert np.abs(c["out64"] @ Vn).max() <= 1e-9 * np.abs(A).max()
    U, s, vt = np.linalg.svd(A, full_matrices=False)
    s2 = s.copy()
    s2[:c["n"]] = 0
    assert np.abs((U * s2) @ vt - c["out64"]).max() <= 1e-9 * np.abs(A).max()      # the reference's U Sigma' V^T
