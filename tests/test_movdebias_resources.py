"""CPU: the moving-median debias kernels (goleft_amd/csrc/gd_movdebias.hpp) as hipcc compiles them for gfx950, and the
symbols the library exports for them.

One kernel, three instances by the window it has room for.  A workgroup is one wave; its window is
an LDS ring of one key (4 bytes) and one rank (1 byte) per slot and lane: CAP x 64 x 5 bytes -- 4 800 for CAP 15, 20 160
for CAP 63, 81 600 for CAP 255, two workgroups of which fit a CU's 160 KB.  The rows in flight (eight cells to divide, eight
to push, their addresses, and the eight slots a push has in flight) are unrolled arrays and the ring is LDS: no scratch;
at most 128 registers a lane, four waves per SIMD (LDS holds the largest instance to two workgroups a CU whatever it
uses).  Metadata only."""
import re

import pytest

from tests import helpers as H

LDS_PER_CU = 160 * 1024
CAPS = (15, 63, 255)                             # MD_CAP_SMALL, MD_CAP_MID, MD_CAP_BIG
WG = 64                                          # MD_COLS: one wave
MAX_VGPR = 128

pytestmark = pytest.mark.skipif(H.HIPCC is None, reason="needs hipcc")


@pytest.fixture(scope="module")
def kernels():
    return {k: r for k, r in H.kernel_metadata(H.api_asm()).items() if "gd_movdebias_" in k}


def cap_of(name):
    return int(re.search(r"gd_movdebias_kernelILi(\d+)E", name).group(1))


def test_three_instances(kernels):
    assert sorted(cap_of(k) for k in kernels) == list(CAPS), sorted(kernels)


def test_no_scratch_and_the_lds_of_the_ring(kernels):
    assert kernels
    for name, r in kernels.items():
        cap = cap_of(name)
        assert r["scratch"] == 0 and r["spill"] == 0, (name, r)
        assert r["wg"] == WG, (name, r)
        assert r["lds"] == cap * 64 * 5, (name, r)
        assert r["vgpr"] <= MAX_VGPR, (name, r)
    big = next(r for k, r in kernels.items() if cap_of(k) == 255)
    assert big["lds"] == 81600 and 2 * big["lds"] <= LDS_PER_CU


def test_the_library_exports_the_symbols():
    from goleft_amd import _lib
    lib = _lib.load()                            # (resolves every symbol of _lib.SYMBOLS, or raises)
    for name in ("gd_moving_debias", "gd_moving_debias_cells", "gd_moving_debias_timing"):
        assert name in _lib.SYMBOLS and getattr(lib, name) is not None
