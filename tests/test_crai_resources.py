"""CPU: the .crai tiling kernels (gd_crai.hpp) as hipcc compiles them for gfx950 -- no scratch and no LDS, the slices handed
round with v_readlane (the state of a sequence lives in scalar registers), the IEEE double division of the write pass
with the product in front of it rounded on its own, and 8-byte stores for the fills."""
import re

import pytest

from tests import helpers as H

pytestmark = pytest.mark.skipif(H.HIPCC is None, reason="needs hipcc")


@pytest.fixture(scope="module")
def asm():
    return H.api_asm()


def kernel(asm, write):
    meta = asm[asm.index("amdhsa.kernels:"):]
    names = set(re.findall(r"\.name:\s+(\S*gd_crai_kernelILb%dE\S*)" % write, meta))
    assert len(names) == 1, names
    (name,) = names
    (k,) = [k for k in re.split(r"\n  - \.", meta)[1:] if name in k]
    text = asm[asm.index("\n%s:" % name):]
    ops = [ln.split()[0] for ln in text[:text.index("s_endpgm")].splitlines() if ln.startswith("\t") and ln.split()]
    return k, ops


@pytest.mark.parametrize("write", [0, 1])
def test_no_scratch_no_lds_and_the_slices_go_round_by_readlane(asm, write):
    k, ops = kernel(asm, write)
    g = lambda key: int(re.search(r"\.%s:\s+(\S+)" % key, "." + k).group(1))
    assert g("private_segment_fixed_size") == 0 and g("group_segment_fixed_size") == 0, k
    assert not any(o.startswith("scratch_") or o.startswith("ds_") for o in ops)
    assert sum(o.startswith("v_readlane_b32") for o in ops) >= 4          # alnStart and alnSpan, two words each
    assert g("vgpr_count") <= 64


def test_write_pass_divides_in_double_precision_and_stores_words(asm):
    _, ops = kernel(asm, 1)
    for need in ("v_div_scale_f64", "v_div_fmas_f64", "v_div_fixup_f64", "v_mul_f64"):
        assert any(o.startswith(need) for o in ops), need
    assert not any(o.startswith("v_rcp_f32") or o.startswith("v_div_scale_f32") for o in ops)
    # the product 100000 * sliceLen is a multiplication of its own, in front of the division's sequence
    assert ops.index(next(o for o in ops if o.startswith("v_mul_f64"))) < ops.index(next(o for o in ops if o.startswith("v_div_scale_f64")))
    assert any(o.startswith("global_store_dwordx2") for o in ops)


def test_count_pass_stores_nothing_but_its_two_results(asm):
    _, ops = kernel(asm, 0)
    assert sum(o.startswith("global_store") for o in ops) == 2
