"""CPU: the indexcov kernels (gd_indexcov.hpp) as hipcc compiles them for gfx950 -- no scratch in any of them, and the
Gram kernel is the 8-bit integer matrix instruction."""
import pytest

from tests import helpers as H

pytestmark = pytest.mark.skipif(H.HIPCC is None, reason="needs hipcc")

KERNELS = ("gd_ic_median_kernel", "gd_ic_depth_kernel", "gd_ic_pass_kernel", "gd_ic_cn_kernel", "gd_ic_rowsum_kernel",
           "gd_ic_gram_kernel", "gd_ic_gram_fin_kernel")


@pytest.fixture(scope="module")
def asm():
    return H.api_asm()


@pytest.fixture(scope="module")
def kernels(asm):
    return H.kernel_metadata(asm)


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
