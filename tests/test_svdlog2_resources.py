"""CPU: the Log2-scaler kernels of the SVD debiaser (goleft_amd/csrc/gd_svdlog2.hpp) and the centre pick they add to
gd_colselect.hpp, as hipcc compiles them for gfx950, and the symbols the library exports for them.  Metadata only.

DESIGN.md section 3.17 claims: no kernel uses scratch; every workgroup is 256 threads, a wave on each SIMD.  The Gram kernel
is gd_svd_gram_kernel with another conversion in its loader: the same two 16 x 64 float64 chunks in LDS (16 384 bytes), the
same 16 accumulators, and log2's temporaries for the two cells a thread converts: at most 104 registers a lane, four
workgroups a CU where the z-score's kernel has six.  The other kernels use no LDS.  The projection holds the row, its
correction and a vector in 3 x NV float64 a lane, as gd_svd_project_kernel does, beside log2's and exp2's temporaries: at
most 64 registers at NV = 1 (eight workgroups a CU), 80 at NV = 2 and 4 (six), 104 at NV = 8 (four), 168 at NV = 16
(three)."""
import re
import subprocess

import pytest

from tests import helpers as H
from tests import test_svddebias_resources as SRS

pytestmark = pytest.mark.skipif(SRS.HIPCC is None, reason="needs hipcc")

workgroups_per_cu = SRS.workgroups_per_cu


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    import os
    path = tmp_path_factory.mktemp("isa") / "api.s"
    subprocess.check_call([SRS.HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                           "-I", os.path.join(H.ROOT, "include"), "-o", str(path),
                           os.path.join(H.ROOT, "goleft_amd", "csrc", "gd_api.hip")], stderr=subprocess.DEVNULL)
    asm = path.read_text()
    meta = asm[asm.index("amdhsa.kernels:"):]
    out = {}
    for k in re.split(r"\n  - \.", meta)[1:]:
        g = lambda key: re.search(r"\.%s:\s+(\S+)" % key, "." + k).group(1)
        if "gd_svl_" in g("name") or "gd_colmid_" in g("name"):
            out[g("name")] = dict(lds=int(g("group_segment_fixed_size")), scratch=int(g("private_segment_fixed_size")),
                                  vgpr=int(g("vgpr_count")), spill=int(g("vgpr_spill_count")),
                                  wg=int(g("max_flat_workgroup_size")))
    return out


def one(kernels, part):
    hits = [r for k, r in kernels.items() if part in k]
    assert len(hits) == 1, (part, sorted(kernels))
    return hits[0]


def test_the_kernels_are_there(kernels):
    assert len(kernels) == 8, sorted(kernels)
    for part in ("gd_svl_centre_kernel", "gd_svl_gram_kernel", "gd_colmid_pick_kernel"):
        one(kernels, part)
    nv = sorted(int(re.search(r"gd_svl_project_kernelILi(\d+)E", k).group(1)) for k in kernels if "project" in k)
    assert nv == [1, 2, 4, 8, 16]


def test_no_scratch_one_wave_a_simd_lds_in_the_gram_kernel_only(kernels):
    for name, r in kernels.items():
        assert r["scratch"] == 0 and r["spill"] == 0, (name, r)
        assert r["lds"] == (2 * 16 * 64 * 8 if "gd_svl_gram_kernel" in name else 0), (name, r)
        assert r["wg"] == SRS.WG, (name, r)


def test_the_workgroups_a_cu_the_design_claims(kernels):
    gram = one(kernels, "gd_svl_gram_kernel")
    assert gram["vgpr"] <= 104 and gram["lds"] == 16384 and workgroups_per_cu(gram) == 4, gram
    for nv, regs, wgs in ((1, 64, 8), (2, 80, 6), (4, 80, 6), (8, 104, 4), (16, 168, 3)):
        r = one(kernels, "gd_svl_project_kernelILi%dE" % nv)
        assert r["vgpr"] <= regs and workgroups_per_cu(r) >= wgs, (nv, r)
    for part in ("gd_svl_centre_kernel", "gd_colmid_pick_kernel"):
        assert workgroups_per_cu(one(kernels, part)) == 8


def test_the_library_exports_the_symbols():
    from goleft_amd import _lib
    lib = _lib.load()                            # (resolves every symbol of _lib.SYMBOLS, or raises)
    for name in ("gd_svd_debias_scaled", "gd_svd_debias_scaled_cells", "gd_svd_debias_scaled_device"):
        assert name in _lib.SYMBOLS and getattr(lib, name) is not None
