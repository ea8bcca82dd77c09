"""CPU: the indexcov kernels (gd_indexcov.hpp) as hipcc compiles them for gfx950 -- no scratch in any of them, and the
Gram kernel is the 8-bit integer matrix instruction."""
import os
import re
import shutil
import subprocess

import pytest

from tests import helpers as H

HIPCC = next((p for p in ("/opt/rocm/bin/hipcc", shutil.which("hipcc") or "") if p and os.path.exists(p)), None)

pytestmark = pytest.mark.skipif(HIPCC is None, reason="needs hipcc")

KERNELS = ("gd_ic_median_kernel", "gd_ic_depth_kernel", "gd_ic_pass_kernel", "gd_ic_cn_kernel", "gd_ic_rowsum_kernel",
           "gd_ic_gram_kernel", "gd_ic_gram_fin_kernel")


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
        out[g("name")] = dict(lds=int(g("group_segment_fixed_size")), scratch=int(g("private_segment_fixed_size")),
                              vgpr=int(g("vgpr_count")))
    return out


@pytest.mark.parametrize("name", KERNELS)
def test_indexcov_kernels_use_no_scratch(kernels, name):
    got = {k: v for k, v in kernels.items() if name in k}
    assert len(got) == 1, (name, sorted(got))
    (k, r), = got.items()
    assert r["scratch"] == 0, (k, r)


def test_gram_kernel_is_the_integer_matrix_instruction(asm, kernels):
    (name,) = [k for k in kernels if "gd_ic_gram_kernel" in k]
    body = asm[asm.index("\n%s:" % name):]
    body = body[:body.index("s_endpgm")]
    assert body.count("v_mfma_i32_16x16x64_i8") >= 4, body[:400]


def test_slot_and_pca8_arithmetic_is_not_contracted(asm, kernels):
    # d * c + 0.5 in two roundings (CountsAtDepth, the pca8 byte): a fused multiply-add would round once
    (name,) = [k for k in kernels if "gd_ic_pass_kernel" in k]
    body = asm[asm.index("\n%s:" % name):]
    body = body[:body.index("s_endpgm")]
    # (the kernel's other fused operations belong to the compiler's 64-bit integer division)
    for const in ("0x423aaaab", "0x45ffff00"):              # float32(70 * float32(2/3)), float32(65535) / 8
        lines = [ln for ln in body.splitlines() if const in ln]
        assert lines and all(ln.split()[0].startswith("v_mul_f32") for ln in lines), (const, lines)
