"""CPU: the resident-matrix kernels (goleft_amd/csrc/gd_devmat.hpp) as hipcc compiles them for gfx950, and the symbols the
library exports for a matrix that stays in HBM.

Three streaming kernels -- int64 cells to float32, the finite-and->=-0 check, the per-sample scale in place -- a wave a
row, four rows a workgroup, four rows of a wave in flight as an unrolled array: no LDS (the header states none), no scratch,
no spills.  Metadata only."""
import os
import re
import shutil
import subprocess

import pytest

from tests import helpers as H

HIPCC = next((p for p in ("/opt/rocm/bin/hipcc", shutil.which("hipcc") or "") if p and os.path.exists(p)), None)
WG = 256                                         # DM_WG = DM_WAVES * 64
KERNELS = ("gd_devmat_from_cells_kernel", "gd_devmat_check_kernel", "gd_devmat_scale_kernel")
NEW_SYMBOLS = ("gd_chunk_debias_cells", "gd_device_scale", "gd_sample_medians_device", "gd_emdepth_device",
               "gd_emcnv_add_device")

pytestmark = pytest.mark.skipif(HIPCC is None, reason="needs hipcc")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    path = tmp_path_factory.mktemp("isa") / "api.s"
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                           "-I", os.path.join(H.ROOT, "include"), "-o", str(path),
                           os.path.join(H.ROOT, "goleft_amd", "csrc", "gd_api.hip")], stderr=subprocess.DEVNULL)
    asm = path.read_text()
    meta = asm[asm.index("amdhsa.kernels:"):]
    out = {}
    for k in re.split(r"\n  - \.", meta)[1:]:
        g = lambda key: re.search(r"\.%s:\s+(\S+)" % key, "." + k).group(1)
        if "gd_devmat_" in g("name"):
            out[g("name")] = dict(lds=int(g("group_segment_fixed_size")), scratch=int(g("private_segment_fixed_size")),
                                  vgpr=int(g("vgpr_count")), spill=int(g("vgpr_spill_count")),
                                  sgpr_spill=int(g("sgpr_spill_count")), wg=int(g("max_flat_workgroup_size")))
    return out


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
