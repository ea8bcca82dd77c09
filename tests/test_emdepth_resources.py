"""CPU: the emdepth kernels (goleft_amd/csrc/gd_emdepth.hpp) as hipcc compiles them for gfx950.

The mapping is one wavefront a row, four rows a workgroup, and no LDS at all: every cross-lane step is a wave-wide
shuffle.  What bounds the waves of a CU is therefore the vector registers alone.  The kernels are designed for FOUR
workgroups per CU (sixteen waves, four per SIMD, 128 registers a lane): a row is a chain of dependent float64 compares,
shuffles and library calls, and four waves a SIMD is what keeps its issue slots filled while one of them waits.  With
the Poisson term (log, lgamma, exp) inlined into the calls of a row's four registers the kernels took 221 - 234
registers -- two waves a SIMD -- and held to 128 by the compiler they spilled; with that term out of line they take
99 - 114.  So: no scratch (nothing is indexed by a runtime value, nothing spills), at most 128 registers, and LDS
(none) that lets four workgroups in."""
import pytest

from tests import helpers as H

LDS_PER_CU = 160 * 1024
WORKGROUPS_PER_CU = 4

pytestmark = pytest.mark.skipif(H.HIPCC is None, reason="needs hipcc")


@pytest.fixture(scope="module")
def asm():
    return H.api_asm()


@pytest.fixture(scope="module")
def kernels(asm):
    return {k: r for k, r in H.kernel_metadata(asm).items() if "gd_emdepth_kernel" in k}


def test_four_instances(kernels):
    # float / int64 cells x row in registers / row re-read
    assert len(kernels) == 4, sorted(kernels)


def test_no_scratch_and_four_workgroups_per_cu(asm, kernels):
    for name, r in kernels.items():
        assert r["scratch"] == 0, (name, r)
        assert r["wg"] == 256, (name, r)
        assert r["lds"] * WORKGROUPS_PER_CU <= LDS_PER_CU, (name, r)
        assert r["vgpr"] <= 512 // WORKGROUPS_PER_CU, (name, r)          # 4 workgroups x 4 waves = 4 waves per SIMD
        body = asm[asm.index("\n%s:" % name):]
        body = body[:body.index("s_endpgm")]
        assert "scratch_" not in body, name
