"""CPU: the SVD debias kernels (goleft_amd/csrc/gd_svddebias.hpp) as hipcc compiles them for gfx950 with the policy of the
linear scalers (SvLinear: none and the z-score), and the symbols the library exports for them.  Metadata only.

DESIGN.md section 3.16 claims: no kernel uses scratch; every workgroup is 256 threads, a wave on each SIMD, so a
workgroup fits a CU as often as a wave's registers fit a SIMD's 512 and its LDS the CU's 160 KB.  The Gram kernel holds two
16 x 64 float64 chunks in LDS (16 384 bytes: ten workgroups by LDS) and 16 float64 accumulators a thread, at most 80
registers a lane: six workgroups a CU.  The other kernels use no LDS.  The projection holds the row, its
correction and a vector in 3 x NV float64 a lane: at most 64 registers up to NV = 8 (eight workgroups a CU) and at most 128
at NV = 16 (four)."""
import re

import pytest

from tests import helpers as H

VGPR_PER_SIMD = 512
WAVES_PER_SIMD = 8
LDS_PER_CU = 160 * 1024
WG = 256                                         # SV_WG: one wave a SIMD
PROJECT = "gd_svd_project_kernelINS_8SvLinearELi%sE"        # gd::gd_svd_project_kernel<gd::SvLinear, NV>

pytestmark = pytest.mark.skipif(H.HIPCC is None, reason="needs hipcc")


@pytest.fixture(scope="module")
def kernels():
    return {k: r for k, r in H.kernel_metadata(H.api_asm()).items() if "gd_svd_" in k and "SvLog2" not in k}


def workgroups_per_cu(r):
    """a workgroup puts one wave on each SIMD: as many as a SIMD holds waves of this many registers (allocated in eights),
    and as the LDS allows"""
    by_regs = min(WAVES_PER_SIMD, VGPR_PER_SIMD // (-(-r["vgpr"] // 8) * 8))
    return by_regs if r["lds"] == 0 else min(by_regs, LDS_PER_CU // r["lds"])


def one(kernels, part):
    hits = [r for k, r in kernels.items() if part in k]
    assert len(hits) == 1, (part, sorted(kernels))
    return hits[0]


def test_the_kernels_are_there(kernels):
    assert len(kernels) == 8, sorted(kernels)
    for part in ("gd_svd_rowstats_kernel", "gd_svd_gram_kernel", "gd_svd_gram_sum_kernel"):
        one(kernels, part)
    nv = sorted(int(re.search(PROJECT % r"(\d+)", k).group(1)) for k in kernels if "project" in k)
    assert nv == [1, 2, 4, 8, 16]


def test_no_scratch_one_wave_a_simd_lds_in_the_gram_kernel_only(kernels):
    for name, r in kernels.items():
        assert r["scratch"] == 0 and r["spill"] == 0, (name, r)
        assert r["lds"] == (2 * 16 * 64 * 8 if "gd_svd_gram_kernel" in name else 0), (name, r)
        assert r["wg"] == WG, (name, r)


def test_the_workgroups_a_cu_the_design_claims(kernels):
    gram = one(kernels, "gd_svd_gram_kernel")
    assert gram["vgpr"] <= 80 and gram["lds"] == 16384 and workgroups_per_cu(gram) == 6, gram
    for nv in (1, 2, 4, 8):
        r = one(kernels, PROJECT % nv)
        assert r["vgpr"] <= 64 and workgroups_per_cu(r) == 8, (nv, r)
    r = one(kernels, PROJECT % 16)
    assert r["vgpr"] <= 128 and workgroups_per_cu(r) >= 4, r
    for part in ("gd_svd_rowstats_kernel", "gd_svd_gram_sum_kernel"):
        assert workgroups_per_cu(one(kernels, part)) == 8


def test_the_library_exports_the_symbols():
    from goleft_amd import _lib
    lib = _lib.load()                            # (resolves every symbol of _lib.SYMBOLS, or raises)
    for name in ("gd_svd_debias", "gd_svd_debias_cells", "gd_svd_debias_device", "gd_svd_debias_timing"):
        assert name in _lib.SYMBOLS and getattr(lib, name) is not None
