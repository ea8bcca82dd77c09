"""CPU: the oracle of `debias --svd --log2` (tests/svdlog2_ref.py) against itself.  Every case of tests/svdlog2_shapes.py has
a cut that no rounding moves, and the two routes -- numpy.linalg.svd(Z) and eigh(Z^T Z), the one the device takes -- agree
on n and on the exponent z' + c within 2^-42 of the largest log of the case (measured between them on these cases:
<= 1.6e-14; the exponents are below 10, so 2^-42 x that leaves more than 10x).  Then the consequences of the definition: a
cut that removes nothing gives the input back, one row is all centres, and the centre is the log of the selected raw cell,
bit for bit, which is the form the device computes."""
import numpy as np
import pytest

from tests import svddebias_shapes as SS
from tests import svdlog2_ref as LR
from tests import svdlog2_shapes as LS


@pytest.mark.parametrize("name", LS.NAMES)
def test_the_cut_is_unambiguous_and_the_routes_agree(name):
    c = LS.case(name)
    A, s, n, pct = c["A"], c["s"], c["n"], c["pct"]
    if s.any():
        share = 100.0 * s / s.sum()
        if n > 0:
            assert abs(share[n - 1] - pct) >= 0.05, (name, share[n - 1], pct)
        if n < len(s):
            assert abs(share[n] - pct) >= 0.05, (name, share[n], pct)
            if n > 0:
                assert (s[n - 1] - s[n]) / s[0] >= 0.01, (name, s[n - 1], s[n], s[0])
    out_b, s_b, n_b, out64_b, e_b, m_b = LR.svd_log2(A, pct, route="gram")
    assert n_b == n
    worst = float(np.abs(e_b - c["e"]).max())
    print(name, "routes differ by", worst, "in the exponent")
    assert worst <= 2.0 ** -42 * max(1.0, float(np.log2(1.0 + A.astype(np.float64)).max())), (name, worst)
    if s.any():
        big = s > 2.0 ** -20 * s[0]
        assert (np.abs(s_b - s)[big] <= 2.0 ** -36 * s[0]).all() and (np.abs(s_b - s)[~big] <= 2.0 ** -20 * s[0]).all()


def test_every_size_and_kind_of_case_is_there():
    S, CS = LS.SLAB, LS.CS_SLAB
    assert {c[2] for c in LS.CASES} >= {2, 3, 63, 64, 65, 128, 257, 1024}
    assert sum(c[2] == 1024 for c in LS.CASES) == 1
    Rs = {c[1] for c in LS.CASES}
    assert Rs >= {1, 2, 3, CS - 1, CS, CS + 1, S - 1, S, S + 1, 3 * S + 7}
    assert max(Rs) <= 4000
    assert {c[3] for c in LS.CASES} >= {0, 1, 3, 15}
    assert any(c[3] == c[2] == 2 for c in LS.CASES)                                   # the cap of N
    low = LS.CASES[LS.NAMES.index(LS.LOW)]
    assert low[5] == 1.5 and LS.case(LS.LOW)["n"] >= 1


def test_the_low_depth_case_clamps_and_lifts():
    c = LS.case(LS.LOW)
    raw = np.exp2(c["e"]) - 1.0
    assert (raw < 0).any() and (c["out64"][raw < 0] == 0).all() and (c["out64"] >= 0).all()
    assert (c["out64"][c["A"] == 0] > 0).any()


def test_the_columns_that_try_the_selection():
    c = LS.case(LS.SELECT)
    A, m = c["A"], c["m"]
    R = A.shape[0]
    assert sorted(LS.SELECT_COLS) == [0, 64, 130, 256]
    assert not A[:, 0].any() and m[0] == 0
    assert (A[:, 64] == 0).sum() > R // 2 and A[:, 64].any() and m[64] == 0
    tie = A[:, 130] == m[130]
    assert tie.sum() >= R // 3 and (A[:, 130] < m[130]).sum() < R // 2 < (A[:, 130] <= m[130]).sum() - 100
    assert m[256] == np.float32(30.5) and A[-1, 256] == m[256] and (A[:, 256] == m[256]).sum() == 1
    assert np.isfinite(c["out"]).all()


def test_the_centre_is_the_log_of_the_selected_cell_bit_for_bit():
    mats = [LS.case(n)["A"] for n in LS.NAMES] + [SS.case(n)["A"] for n in SS.NAMES]
    for A in mats:
        _, c = LR.scale(A.astype(np.float64))
        m = LR.centre_cells(A)
        assert m.dtype == np.float32
        assert np.log2(1.0 + m.astype(np.float64)).tobytes() == c.tobytes()


def test_a_cut_above_the_first_share_gives_the_input_back():
    for name in ("n64_slab", LS.LOW, LS.SELECT):
        c = LS.case(name)
        s = c["s"]
        out, _, n, out64, _, _ = LR.svd_log2(c["A"], (100.0 * s[0] / s.sum() + 100.0) / 2)
        assert n == 0
        A = c["A"].astype(np.float64)
        assert (np.abs(out64 - A) <= 2.0 ** -48 * (1.0 + A)).all()                    # log2, exp2 and two roundings of the sum
        assert (np.abs(out.astype(np.float64) - A) <= 2.0 ** -24 * A).all()


def test_one_row_is_all_centres():
    c = LS.case("n3_one_row")
    A = c["A"]
    assert A.shape[0] == 1
    Z, ce = LR.scale(A.astype(np.float64))
    assert not Z.any() and c["n"] == 0 and not c["s"].any()
    assert c["m"].tobytes() == A[0].tobytes()
    assert (np.abs(c["out"].astype(np.float64) - A) <= 2.0 ** -24 * A).all()
    for pct in (0.0, 50.0):
        assert LR.svd_log2(A, pct)[2] == 0
        assert LR.svd_log2(A, pct, route="gram")[2] == 0
