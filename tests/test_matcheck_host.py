"""CPU: goleft_amd/csrc/gd_matcheck.hpp -- the host-side decisions of the entry points that take a depth matrix -- compiled
as it is (tests/emul/matcheck_emul.cpp) and compared with the restatements: the argsort with tests/movdebias_ref.py's order
and numpy's stable one, the chunk walk with tests/debias_ref.chunks, slices and chunk_of_row exactly."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import debias_ref as DR
from tests import helpers as H
from tests import movdebias_ref as MR

EMUL_DIR = os.path.join(H.ROOT, "tests", "emul")
CLANG = next((p for p in ("/opt/rocm/lib/llvm/bin/clang++", shutil.which("clang++") or "") if p and os.path.exists(p)), None)

pytestmark = pytest.mark.skipif(CLANG is None, reason="the header is compiled for the host with clang")

SIZE_MAX = 2 ** 64 - 1
FLT_MAX = np.finfo(np.float32).max


@pytest.fixture(scope="module")
def lib():
    src = os.path.join(EMUL_DIR, "matcheck_emul.cpp")
    so = os.path.join(EMUL_DIR, "matcheck_emul.so")
    deps = [src, os.path.join(H.ROOT, "goleft_amd", "csrc", "gd_matcheck.hpp")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call([CLANG, "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, src])
    lib = C.CDLL(so)
    lib.mc_first_bad.argtypes, lib.mc_first_bad.restype = [C.c_void_p, C.c_size_t], C.c_longlong
    lib.mc_fits.argtypes, lib.mc_fits.restype = [C.c_size_t] * 3, C.c_int
    lib.mc_overlap.argtypes, lib.mc_overlap.restype = [C.c_size_t] * 4, C.c_int
    lib.mc_chunks.argtypes = [C.c_void_p, C.c_size_t, C.c_double] + [C.c_void_p] * 3 + [C.POINTER(C.c_size_t)]
    lib.mc_chunks.restype = C.c_size_t
    return lib


def walk(lib, vals, window):
    """(order, slices, chunk_of_row, largest) as the header has them"""
    v = np.ascontiguousarray(vals, np.float64)
    n = len(v)
    order, slices, cor = np.full(n, 0xffffffff, np.uint32), np.full(n + 1, 0xffffffff, np.uint32), np.full(n, 0xffffffff, np.uint32)
    largest = C.c_size_t(0)
    count = lib.mc_chunks(v.ctypes.data, n, float(window), order.ctypes.data, slices.ctypes.data, cor.ctypes.data, C.byref(largest))
    assert (slices[count + 1:] == 0xffffffff).all()
    return order, slices[:count + 1], cor, largest.value


def check_walk(lib, vals, window):
    vals = np.asarray(vals, np.float64)
    order, slices, cor, largest = walk(lib, vals, window)
    assert np.array_equal(order, np.argsort(vals, kind="stable"))
    assert np.array_equal(order, MR.order_of(vals))
    _, want_slices, want_cor = DR.chunks(vals, window)
    assert np.array_equal(slices, want_slices)
    assert cor.dtype == want_cor.dtype and np.array_equal(cor, want_cor)
    assert largest == np.diff(want_slices).max()
    return order, slices, cor


def test_one_row(lib):
    order, slices, cor = check_walk(lib, [0.3], 0.1)
    assert order.tolist() == [0] and slices.tolist() == [0, 1] and cor.tolist() == [0]


def test_all_values_equal(lib):
    _, slices, cor = check_walk(lib, [0.5] * 7, 1e-300)
    assert slices.tolist() == [0, 7] and not cor.any()


def test_a_chunk_per_row(lib):
    _, slices, cor = check_walk(lib, [3.0, 0.0, 2.0, 5.0, 1.0, 4.0], 0.5)
    assert slices.tolist() == list(range(7)) and cor.tolist() == [3, 0, 2, 5, 1, 4]


def test_a_difference_equal_to_the_window_is_no_boundary_and_an_ulp_more_is(lib):
    assert 0.75 - 0.25 == 0.5
    assert check_walk(lib, [0.75, 0.25], 0.5)[1].tolist() == [0, 2]
    above = np.nextafter(0.75, np.inf)
    assert above - 0.25 == np.nextafter(0.5, np.inf)         # the next float64 after the window
    assert check_walk(lib, [above, 0.25], 0.5)[1].tolist() == [0, 1, 2]
    # the difference is taken from the value that opened the chunk, not from the neighbour
    assert check_walk(lib, [0.25, 0.5, 0.75, above], 0.5)[1].tolist() == [0, 3, 4]


def test_minus_zero_ties_with_zero_and_the_row_decides(lib):
    order, slices, _ = check_walk(lib, [0.0, -0.0, 0.0, -0.0, -1.0], 0.5)
    assert order.tolist() == [4, 0, 1, 2, 3] and slices.tolist() == [0, 1, 5]


def test_denormals(lib):
    tiny = 5e-324
    order, slices, cor = check_walk(lib, [tiny, 0.0, 2 * tiny, tiny, 3 * tiny], tiny)
    assert order.tolist() == [1, 0, 3, 2, 4] and slices.tolist() == [0, 3, 5] and cor.tolist() == [0, 0, 1, 0, 1]


def test_a_descending_input(lib):
    order, slices, _ = check_walk(lib, np.arange(10)[::-1] * 0.25, 0.5)
    assert order.tolist() == list(range(9, -1, -1)) and slices.tolist() == [0, 3, 6, 9, 10]


@pytest.mark.parametrize("seed", range(8))
def test_random_inputs_with_heavy_ties(lib, seed):
    rng = np.random.default_rng(seed)
    for rows in sorted(set([1, 2, 300] + rng.integers(1, 301, 12).tolist())):
        vals = np.round(rng.normal(0.41, 0.05, rows), 2)
        for window in (0.03, 0.01, 1e-9, 10.0):
            check_walk(lib, vals, window)
        check_walk(lib, rng.integers(0, 3, rows).astype(np.float64), 0.5)


@pytest.mark.parametrize("at", (0, 7, 14))
def test_the_first_cell_that_is_not_a_depth(lib, at):
    good = (np.arange(15, dtype=np.float32) + 1).reshape(3, 5)
    first = lambda m: lib.mc_first_bad(np.ascontiguousarray(m).ctypes.data, m.size)
    assert first(good) == -1
    for bad in (np.nan, np.inf, -np.inf, -1e-45):
        m = good.copy()
        m.flat[at] = bad
        assert np.isnan(m.flat[at]) or m.flat[at] < 0 or np.isinf(m.flat[at])
        assert first(m) == at, bad
        m.flat[14] = np.nan                              # the first of two
        assert first(m) == at
    for fine in (-0.0, FLT_MAX, 1e-45, 0.0):
        m = good.copy()
        m.flat[at] = fine
        assert first(m) == -1, fine
    assert lib.mc_first_bad(good.ctypes.data, 0) == -1


def test_overlap(lib):
    a = 1 << 20
    assert not lib.mc_overlap(a, 64, a + 64, 64) and not lib.mc_overlap(a + 64, 64, a, 64)      # they touch
    assert lib.mc_overlap(a, 65, a + 64, 64) and lib.mc_overlap(a + 64, 64, a, 65)              # one byte
    assert lib.mc_overlap(a, 64, a + 63, 1) and lib.mc_overlap(a + 63, 1, a, 64)
    assert lib.mc_overlap(a, 64, a + 8, 16) and lib.mc_overlap(a + 8, 16, a, 64)                # one inside the other
    assert lib.mc_overlap(a, 64, a, 64)
    assert not lib.mc_overlap(a, 64, a + 4096, 64)


@pytest.mark.parametrize("n", (1, 9, 10, 4096))
def test_fits_up_to_the_first_row_count_that_overflows(lib, n):
    cols = max(n, 9)
    rows = SIZE_MAX // 8 // cols + 1
    assert (rows - 1) * cols * 8 <= SIZE_MAX < rows * cols * 8
    assert lib.mc_fits(rows - 1, n, 9) and not lib.mc_fits(rows, n, 9)
    assert lib.mc_fits(0, n, 9) and lib.mc_fits(1, n, 9) and not lib.mc_fits(SIZE_MAX, n, 9)
