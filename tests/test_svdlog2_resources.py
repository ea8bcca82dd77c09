"""CPU: the SVD debias kernels as hipcc compiles them for gfx950 with the Log2 scaler's policy (SvLog2,
goleft_amd/csrc/gd_svdlog2.hpp), its centre kernel and the centre pick it adds to gd_colselect.hpp, and the symbols the
library exports for them.  Metadata only.

DESIGN.md section 3.17 claims: no kernel uses scratch; every workgroup is 256 threads, a wave on each SIMD.  The Gram kernel
is the linear scalers' with another conversion in its loader: the same two 16 x 64 float64 chunks in LDS (16 384 bytes), the
same 16 accumulators, and log2's temporaries for the two cells a thread converts: at most 104 registers a lane, four
workgroups a CU where the z-score's kernel has six.  The other kernels use no LDS.  The projection holds the row, its
correction and a vector in 3 x NV float64 a lane, as it does for the linear scalers, beside log2's and exp2's temporaries: at
most 64 registers at NV = 1 (eight workgroups a CU), 80 at NV = 2 and 4 (six), 104 at NV = 8 (four), 168 at NV = 16
(three)."""
import re

import pytest

from tests import helpers as H
from tests import test_svddebias_resources as SRS

pytestmark = pytest.mark.skipif(H.HIPCC is None, reason="needs hipcc")

workgroups_per_cu, one = SRS.workgroups_per_cu, SRS.one
GRAM = "gd_svd_gram_kernelINS_6SvLog2E"                     # gd::gd_svd_gram_kernel<gd::SvLog2>
PROJECT = "gd_svd_project_kernelINS_6SvLog2ELi%sE"          # gd::gd_svd_project_kernel<gd::SvLog2, NV>


@pytest.fixture(scope="module")
def kernels():
    return {k: r for k, r in H.kernel_metadata(H.api_asm()).items() if "SvLog2" in k or "gd_svl_" in k or "gd_colmid_" in k}


def test_the_kernels_are_there(kernels):
    assert len(kernels) == 8, sorted(kernels)
    for part in ("gd_svl_centre_kernel", GRAM, "gd_colmid_pick_kernel"):
        one(kernels, part)
    nv = sorted(int(re.search(PROJECT % r"(\d+)", k).group(1)) for k in kernels if "project" in k)
    assert nv == [1, 2, 4, 8, 16]


def test_no_scratch_one_wave_a_simd_lds_in_the_gram_kernel_only(kernels):
    for name, r in kernels.items():
        assert r["scratch"] == 0 and r["spill"] == 0, (name, r)
        assert r["lds"] == (2 * 16 * 64 * 8 if GRAM in name else 0), (name, r)
        assert r["wg"] == SRS.WG, (name, r)


def test_the_workgroups_a_cu_the_design_claims(kernels):
    gram = one(kernels, GRAM)
    assert gram["vgpr"] <= 104 and gram["lds"] == 16384 and workgroups_per_cu(gram) == 4, gram
    for nv, regs, wgs in ((1, 64, 8), (2, 80, 6), (4, 80, 6), (8, 104, 4), (16, 168, 3)):
        r = one(kernels, PROJECT % nv)
        assert r["vgpr"] <= regs and workgroups_per_cu(r) >= wgs, (nv, r)
    for part in ("gd_svl_centre_kernel", "gd_colmid_pick_kernel"):
        assert workgroups_per_cu(one(kernels, part)) == 8


def test_the_library_exports_the_symbols():
    from goleft_amd import _lib
    lib = _lib.load()                            # (resolves every symbol of _lib.SYMBOLS, or raises)
    for name in ("gd_svd_debias_scaled", "gd_svd_debias_scaled_cells", "gd_svd_debias_scaled_device"):
        assert name in _lib.SYMBOLS and getattr(lib, name) is not None
