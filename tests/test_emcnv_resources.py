"""CPU: the emcnv kernels (goleft_amd/csrc/gd_emcnv.hpp) as hipcc compiles them for gfx950, from the kernel metadata
alone (vector registers, LDS and scratch sizes, workgroup size).

They are short integer kernels that wait on memory: a broadcast load of one member word per row of a chunk, a gather
of F at the members.  What hides that latency is waves in flight, so they are designed for EIGHT workgroups of four
waves per CU -- eight waves a SIMD, the most gfx950 schedules -- which takes at most 64 vector registers a lane and,
for the three scan kernels, their 2 KB of LDS eight times over.  The two per-block kernels call the float64 log2 and
carry a row's cells: they are held to the same 64.  Nothing is indexed by a runtime register index and nothing may
spill: no scratch."""
import os
import re
import shutil
import subprocess

import pytest

from tests import helpers as H

HIPCC = next((p for p in ("/opt/rocm/bin/hipcc", shutil.which("hipcc") or "") if p and os.path.exists(p)), None)
LDS_PER_CU = 160 * 1024
WORKGROUPS_PER_CU = 8
EXPECTED = ("gd_emcnv_member_kernel", "gd_emcnv_gather_kernel", "gd_emcnv_scan_tile_kernel", "gd_emcnv_scan_top_kernel",
            "gd_emcnv_scan_apply_kernel", "gd_emcnv_span_kernel", "gd_emcnv_gap_kernel", "gd_emcnv_chunk_kernel",
            "gd_emcnv_carry_kernel", "gd_emcnv_emit_kernel", "gd_emcnv_members_kernel")

pytestmark = pytest.mark.skipif(HIPCC is None, reason="needs hipcc")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    path = tmp_path_factory.mktemp("isa") / "api.s"
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                           "-I", os.path.join(H.ROOT, "include"), "-o", str(path),
                           os.path.join(H.ROOT, "goleft_amd", "csrc", "gd_api.hip")], stderr=subprocess.DEVNULL)
    text = path.read_text()
    meta = text[text.index("amdhsa.kernels:"):]
    out = {}
    for k in re.split(r"\n  - \.", meta)[1:]:
        g = lambda key: re.search(r"\.%s:\s+(\S+)" % key, "." + k).group(1)
        if "gd_emcnv_" in g("name"):
            out[g("name")] = dict(lds=int(g("group_segment_fixed_size")), scratch=int(g("private_segment_fixed_size")),
                                  vgpr=int(g("vgpr_count")), wg=int(g("max_flat_workgroup_size")))
    return out


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
