"""CPU: the emdepth kernels (goleft_amd/csrc/gd_emdepth.hpp) as hipcc compiles them for gfx950.

The mapping is one wavefront a row, four rows a workgroup, and no LDS at all: every cross-lane step is a wave-wide
shuffle.  What bounds the waves of a CU is therefore the vector registers alone.  The kernels are designed for FOUR
workgroups per CU (sixteen waves, four per SIMD, 128 registers a lane): a row is a chain of dependent float64 compares,
shuffles and library calls, and four waves a SIMD is what keeps its issue slots filled while one of them waits.  With
the Poisson term (log, lgamma, exp) inlined into the calls of a row's four registers the kernels took 221 - 234
registers -- two waves a SIMD -- and held to 128 by the compiler they spilled; with that term out of line they take
99 - 114.  So: no scratch (nothing is indexed by a runtime value, nothing spills), at most 128 registers, and LDS
(none) that lets four workgroups in."""
import os
import re
import shutil
import subprocess

import pytest

from tests import helpers as H

HIPCC = next((p for p in ("/opt/rocm/bin/hipcc", shutil.which("hipcc") or "") if p and os.path.exists(p)), None)
LDS_PER_CU = 160 * 1024
WORKGROUPS_PER_CU = 4

pytestmark = pytest.mark.skipif(HIPCC is None, reason="needs hipcc")


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    path = tmp_path_factory.mktemp("isa") / "api.s"
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                           "-I", os.path.join(H.ROOT, "include"), "-o", str(path),
                           os.path.join(H.ROOT, "goleft_amd", "csrc", "gd_api.hip")], stderr=subprocess.DEVNULL)
    return path.read_text()


@pytest.fixture(scope="module")
def kernels(asm):
    meta = asm[asm.index("amdhsa.kernels:"):]
    out = {}
    for k in re.split(r"\n  - \.", meta)[1:]:
        g = lambda key: re.search(r"\.%s:\s+(\S+)" % key, "." + k).group(1)
        if "gd_emdepth_kernel" in g("name"):
            out[g("name")] = dict(lds=int(g("group_segment_fixed_size")), scratch=int(g("private_segment_fixed_size")),
                                  vgpr=int(g("vgpr_count")), wg=int(g("max_flat_workgroup_size")))
    return out


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
