"""CPU: the covstats kernels (gd_covstats.hpp) as hipcc compiles them for gfx950 -- no scratch, and the walk's LDS
no larger than that of the depth walk it sits beside."""
import pytest

from tests import helpers as H

pytestmark = pytest.mark.skipif(H.HIPCC is None, reason="needs hipcc")

KERNELS = ("gd_cs_walk_kernel", "gd_cs_compact_kernel", "gd_cs_tile_kernel", "gd_cs_tscan_kernel", "gd_cs_select_kernel",
           "gd_cs_hist_kernel")


@pytest.fixture(scope="module")
def kernels():
    return H.kernel_metadata(H.api_asm())


@pytest.mark.parametrize("name", KERNELS)
def test_covstats_kernels_use_no_scratch(kernels, name):
    got = {k: v for k, v in kernels.items() if name in k}
    assert len(got) == 1, (name, sorted(got))
    (k, r), = got.items()
    assert r["scratch"] == 0, (k, r)
    assert r["lds"] <= 4608, (k, r)                       # (beside the inflate workgroups of the next range)


def test_covstats_walk_stages_no_more_than_the_depth_walk(kernels):
    (_, cs), = {k: v for k, v in kernels.items() if "gd_cs_walk_kernel" in k}.items()
    depth = [v for k, v in kernels.items() if "gd_bam_walk_kernel" in k]
    assert depth and cs["lds"] <= max(v["lds"] for v in depth), (cs, depth)
