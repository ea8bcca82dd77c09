"""CPU: the covstats kernels (gd_covstats.hpp) as hipcc compiles them for gfx950 -- no scratch, and the walk's LDS
no larger than that of the depth walk it sits beside."""
import os
import re
import shutil
import subprocess

import pytest

from tests import helpers as H

HIPCC = next((p for p in ("/opt/rocm/bin/hipcc", shutil.which("hipcc") or "") if p and os.path.exists(p)), None)

pytestmark = pytest.mark.skipif(HIPCC is None, reason="needs hipcc")

KERNELS = ("gd_cs_walk_kernel", "gd_cs_compact_kernel", "gd_cs_tile_kernel", "gd_cs_tscan_kernel", "gd_cs_select_kernel",
           "gd_cs_hist_kernel")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    asm = tmp_path_factory.mktemp("isa") / "api.s"
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                           "-I", os.path.join(H.ROOT, "include"), "-o", str(asm),
                           os.path.join(H.ROOT, "goleft_amd", "csrc", "gd_api.hip")], stderr=subprocess.DEVNULL)
    text = asm.read_text()
    meta = text[text.index("amdhsa.kernels:"):]
    out = {}
    for k in re.split(r"\n  - \.", meta)[1:]:
        g = lambda key: re.search(r"\.%s:\s+(\S+)" % key, "." + k).group(1)
        out[g("name")] = dict(lds=int(g("group_segment_fixed_size")), scratch=int(g("private_segment_fixed_size")),
                              vgpr=int(g("vgpr_count")))
    return out


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
