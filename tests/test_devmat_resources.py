"""CPU: the resident-matrix kernels (goleft_amd/csrc/gd_devmat.hpp) as hipcc compiles them for gfx950, and the symbols the
library exports for a matrix that stays in HBM.

Three streaming kernels -- int64 cells to float32, the finite-and->=-0 check, the per-sample scale in place -- a wave a
row, four rows a workgroup, four rows of a wave in flight as an unrolled array: no LDS (the header states none), no scratch,
no spills.  Metadata only."""
import os
import re

import pytest

from tests import helpers as H

WG = 256                                         # DM_WG = DM_WAVES * 64
KERNELS = ("gd_devmat_from_cells_kernel", "gd_devmat_check_kernel", "gd_devmat_scale_kernel")
NEW_SYMBOLS = ("gd_chunk_debias_cells", "gd_device_scale", "gd_sample_medians_device", "gd_emdepth_device",
               "gd_emcnv_add_device")

pytestmark = pytest.mark.skipif(H.HIPCC is None, reason="needs hipcc")


@pytest.fixture(scope="module")
def kernels():
    return {k: r for k, r in H.kernel_metadata(H.api_asm()).items() if "gd_devmat_" in k}


def test_three_kernels(kernels):
    assert len(kernels) == 3, sorted(kernels)
    for want in KERNELS:
        assert len([k for k in kernels if want in k]) == 1, (want, sorted(kernels))


def test_no_scratch_no_spills_no_lds(kernels):
    assert kernels
    for name, r in kernels.items():
        assert r["scratch"] == 0 and r["spill"] == 0 and r["sgpr_spill"] == 0, (name, r)
        assert r["lds"] == 0 and r["wg"] == WG, (name, r)
        assert r["vgpr"] <= 64, (name, r)        # eight waves a SIMD are not held back by registers


def test_the_library_exports_the_new_symbols():
    from goleft_amd import _lib
    lib = _lib.load()                            # (resolves every symbol of _lib.SYMBOLS, or raises)
    for name in NEW_SYMBOLS:
        assert name in _lib.SYMBOLS and getattr(lib, name) is not None
    header = open(os.path.join(H.ROOT, "include", "goleft_depth.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % name, header), name
