"""CPU: the indexsplit kernel (gd_indexsplit.hpp) as hipcc compiles it for gfx950 -- no scratch, the IEEE double
division, and no fused multiply-add outside that division's own sequence (the quotient is added with its own rounding)."""
import re

import pytest

from tests import helpers as H

pytestmark = pytest.mark.skipif(H.HIPCC is None, reason="needs hipcc")


@pytest.fixture(scope="module")
def asm():
    return H.api_asm()


@pytest.fixture(scope="module")
def body(asm):
    meta = asm[asm.index("amdhsa.kernels:"):]
    names = re.findall(r"\.name:\s+(\S*gd_is_sum_kernel\S*)", meta)
    assert len(set(names)) == 1, names
    text = asm[asm.index("\n%s:" % names[0]):]
    return names[0], [ln.split() for ln in text[:text.index("s_endpgm")].splitlines() if ln.startswith("\t") and ln.split()]


def test_sum_kernel_uses_no_scratch_and_no_lds(asm, body):
    meta = asm[asm.index("amdhsa.kernels:"):]
    (k,) = [k for k in re.split(r"\n  - \.", meta)[1:] if body[0] in k]
    g = lambda key: int(re.search(r"\.%s:\s+(\S+)" % key, "." + k).group(1))
    assert g("private_segment_fixed_size") == 0 and g("group_segment_fixed_size") == 0, k
    assert not any(ins[0].startswith("scratch_") for ins in body[1])


def test_sum_kernel_divides_in_double_precision(body):
    ops = [ins[0] for ins in body[1]]
    for need in ("v_div_scale_f64", "v_div_fmas_f64", "v_div_fixup_f64"):
        assert any(o.startswith(need) for o in ops), need
    # (a product with a rounded 1e-9 would be a different number)
    assert ops.count("v_div_fixup_f64") >= 1 and not any(o.startswith("v_rcp_f32") or o.startswith("v_div_scale_f32") for o in ops)


def test_sum_kernel_adds_with_its_own_rounding(body):
    ops = [ins[0] for ins in body[1]]
    inside = False
    n_div = n_add_after = 0
    for i, o in enumerate(ops):
        if o.startswith("v_div_scale_f64"):
            inside = True
        elif o.startswith("v_div_fixup_f64"):
            inside = False
            n_div += 1
            # the accumulation follows the quotient as an addition of its own
            n_add_after += any(p.startswith("v_add_f64") for p in ops[i + 1:i + 4])
        elif re.match(r"v_(fma|fmac|mad)_f64", o):
            assert inside, (i, ops[max(0, i - 5):i + 5])
    assert n_div >= 1 and n_add_after == n_div
    # the loads of (sample, reference) offsets and counts are scalar
    assert sum(o.startswith("s_load_dword") for o in ops) >= 4
