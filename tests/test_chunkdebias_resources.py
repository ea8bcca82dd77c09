"""CPU: the chunk-debias kernels (goleft_amd/csrc/gd_chunkdebias.hpp) as hipcc compiles them for gfx950, and the two
symbols the library exports for them.

The median kernel keeps one counter per (digit, column) of its 64 columns in LDS, laid out [bin][column], plus the eight
partial sums of a column's scan and three words of state per column: 256 x 64 x 4 + 8 x 64 x 4 + 3 x 64 x 4 = 68 352 bytes a
workgroup.  It is designed for TWO workgroups of 512 threads per CU (136 704 of the 160 KB; sixteen waves, four per SIMD,
so at most 128 registers a lane).  The cells a wave has in flight and the 32 bins it scans are unrolled arrays and nothing
is indexed by a runtime value: no scratch.  The divide kernel is a wave a row, four rows a workgroup, and uses no LDS.
Metadata only."""
import pytest

from tests import helpers as H

LDS_PER_CU = 160 * 1024
WORKGROUPS_PER_CU = 2                            # CD_WG_PER_CU
MEDIAN_WG, DIVIDE_WG = 512, 256                  # CD_WG, CD_DIV_WAVES * 64
MEDIAN_LDS = (256 * 64 + 8 * 64 + 3 * 64) * 4    # CD_BINS * CD_COLS counters, CD_WAVES * CD_COLS sums, prefix / rank / zeros

pytestmark = pytest.mark.skipif(H.HIPCC is None, reason="needs hipcc")


@pytest.fixture(scope="module")
def kernels():
    return {k: r for k, r in H.kernel_metadata(H.api_asm()).items() if "gd_chunkdebias_" in k}


def test_two_kernels(kernels):
    assert len([k for k in kernels if "median_kernel" in k]) == 1, sorted(kernels)
    assert len([k for k in kernels if "divide_kernel" in k]) == 1, sorted(kernels)
    assert len(kernels) == 2, sorted(kernels)


def test_no_scratch_and_two_workgroups_per_cu(kernels):
    assert kernels
    for name, r in kernels.items():
        assert r["scratch"] == 0 and r["spill"] == 0, (name, r)
        if "median_kernel" in name:
            assert r["wg"] == MEDIAN_WG, (name, r)
            assert r["lds"] == MEDIAN_LDS == 68352, (name, r)
            assert r["lds"] * WORKGROUPS_PER_CU <= LDS_PER_CU, (name, r)
            assert r["vgpr"] <= 512 // (WORKGROUPS_PER_CU * MEDIAN_WG // 256), (name, r)     # 2 x 8 waves = 4 per SIMD
        else:
            assert r["wg"] == DIVIDE_WG and r["lds"] == 0, (name, r)


def test_the_library_exports_the_two_symbols():
    from goleft_amd import _lib
    lib = _lib.load()                            # (resolves every symbol of _lib.SYMBOLS, or raises)
    for name in ("gd_chunk_debias", "gd_chunk_debias_timing"):
        assert name in _lib.SYMBOLS and getattr(lib, name) is not None
