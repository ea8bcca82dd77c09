"""CPU: the emcnv kernels (goleft_amd/csrc/gd_emcnv.hpp) as hipcc compiles them for gfx950, from the kernel metadata
alone (vector registers, LDS and scratch sizes, workgroup size).

They are short integer kernels that wait on memory: a broadcast load of one member word per row of a chunk, a gather
of F at the members.  What hides that latency is waves in flight, so they are designed for EIGHT workgroups of four
waves per CU -- eight waves a SIMD, the most gfx950 schedules -- which takes at most 64 vector registers a lane and,
for the three scan kernels, their 2 KB of LDS eight times over.  The two per-block kernels call the float64 log2 and
carry a row's cells: they are held to the same 64.  Nothing is indexed by a runtime register index and nothing may
spill: no scratch."""
import pytest

from tests import helpers as H

LDS_PER_CU = 160 * 1024
WORKGROUPS_PER_CU = 8
EXPECTED = ("gd_emcnv_member_kernel", "gd_emcnv_gather_kernel", "gd_emcnv_scan_tile_kernel", "gd_emcnv_scan_top_kernel",
            "gd_emcnv_scan_apply_kernel", "gd_emcnv_span_kernel", "gd_emcnv_gap_kernel", "gd_emcnv_chunk_kernel",
            "gd_emcnv_carry_kernel", "gd_emcnv_emit_kernel", "gd_emcnv_members_kernel")

pytestmark = pytest.mark.skipif(H.HIPCC is None, reason="needs hipcc")


@pytest.fixture(scope="module")
def kernels():
    return {k: r for k, r in H.kernel_metadata(H.api_asm()).items() if "gd_emcnv_" in k}


def test_the_kernels_are_there(kernels):
    # member and gather for float and int64 cells, span for its two levels, emit for its two phases: 15 in all
    for stem in EXPECTED:
        assert any(stem in name for name in kernels), stem
    assert len(kernels) == 15, sorted(kernels)


def test_no_scratch_and_eight_workgroups_per_cu(kernels):
    for name, r in kernels.items():
        print(name, r)
        assert r["scratch"] == 0, (name, r)
        assert r["wg"] == 256, (name, r)
        assert r["lds"] * WORKGROUPS_PER_CU <= LDS_PER_CU, (name, r)
        assert r["vgpr"] <= 512 // WORKGROUPS_PER_CU, (name, r)          # 8 workgroups x 4 waves = 8 waves per SIMD
