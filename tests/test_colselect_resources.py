"""CPU: the column-select kernels (goleft_amd/csrc/gd_colselect.hpp) as hipcc compiles them for gfx950.

The histogram kernel keeps one counter per (digit, column) of its 64 columns in LDS, laid out [bin][column] so that lane l
only touches words that are l mod 64: 256 x 64 x 4 bytes = 64 KB a workgroup.  It is designed for TWO workgroups of 512
threads per CU (128 KB of the 160 KB; sixteen waves, four per SIMD, so at most 128 registers a lane), and the launch is
capped at two workgroups per CU accordingly.  The rows a wave has in flight are an unrolled array and nothing is indexed
by a runtime value: no scratch.  The pick kernel is one wavefront a column, four columns a workgroup, and uses no LDS.
Metadata only."""
import pytest

from tests import helpers as H

LDS_PER_CU = 160 * 1024
WORKGROUPS_PER_CU = 2                            # CS_WG_PER_CU
HIST_WG, PICK_WG = 512, 256                      # CS_WG, CS_PICK_WAVES * 64
HIST_LDS = 256 * 64 * 4                          # CS_BINS * CS_COLS counters

pytestmark = pytest.mark.skipif(H.HIPCC is None, reason="needs hipcc")


@pytest.fixture(scope="module")
def kernels():
    return {k: r for k, r in H.kernel_metadata(H.api_asm()).items() if "gd_colselect_" in k}


def test_seven_instances(kernels):
    # histogram: float / int64 cells x first / later pass; pick: float first, int64 lengths, a digit
    assert len([k for k in kernels if "hist_kernel" in k]) == 4, sorted(kernels)
    assert len([k for k in kernels if "pick_kernel" in k]) == 3, sorted(kernels)


def test_no_scratch_and_two_workgroups_per_cu(kernels):
    for name, r in kernels.items():
        assert r["scratch"] == 0 and r["spill"] == 0, (name, r)
        if "hist_kernel" in name:
            assert r["wg"] == HIST_WG, (name, r)
            assert r["lds"] == HIST_LDS, (name, r)
            assert r["lds"] * WORKGROUPS_PER_CU <= LDS_PER_CU, (name, r)
            assert r["vgpr"] <= 512 // (WORKGROUPS_PER_CU * HIST_WG // 256), (name, r)       # 2 x 8 waves = 4 per SIMD
        else:
            assert r["wg"] == PICK_WG and r["lds"] == 0, (name, r)
