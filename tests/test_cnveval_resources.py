"""CPU: the cnveval kernels (goleft_amd/csrc/gd_cnveval.hpp) as hipcc compiles them for gfx950.

DESIGN.md section 3.18 claims EIGHT workgroups of 256 work items per CU -- 32 wavefronts, eight per SIMD: a pair is a
binary search and a short walk of dependent loads from tables that sit in the L2, and other wavefronts are what fills
the wait.  That takes at most 64 registers a lane and an eighth of the LDS (the kernels use twelve 64-bit words).  A work
item's counters are named registers, nothing is indexed by a runtime value: no scratch."""
import shutil
import subprocess

import pytest

from tests import helpers as H

LDS_PER_CU = 160 * 1024
WORKGROUPS_PER_CU = 8
KERNELS = ("gd_cnveval_positive_kernel", "gd_cnveval_pairs_kernel")

pytestmark = pytest.mark.skipif(H.HIPCC is None, reason="needs hipcc")


@pytest.fixture(scope="module")
def asm():
    return H.api_asm()


@pytest.fixture(scope="module")
def kernels(asm):
    return {k: r for k, r in H.kernel_metadata(asm).items() if "gd_cnveval" in k}


def test_the_two_kernels_exist_under_their_names(kernels):
    assert len(kernels) == 2, sorted(kernels)
    for name in KERNELS:
        assert sum(name in k for k in kernels) == 1, (name, sorted(kernels))


def test_no_scratch_and_eight_workgroups_per_cu(asm, kernels):
    assert kernels
    for name, r in kernels.items():
        assert r["scratch"] == 0 and r["spill"] == 0 and r["sgpr_spill"] == 0, (name, r)
        assert r["wg"] == 256, (name, r)
        assert r["lds"] == 12 * 8, (name, r)
        assert r["lds"] * WORKGROUPS_PER_CU <= LDS_PER_CU, (name, r)
        assert r["vgpr"] <= 512 // WORKGROUPS_PER_CU, (name, r)                  # 8 workgroups x 4 waves = 8 waves per SIMD
        body = asm[asm.index("\n%s:" % name):]
        body = body[:body.index("s_endpgm")]
        assert "scratch_" not in body, name


def test_counters_are_64_bit_integer_atomics_and_the_division_is_ieee(asm, kernels):
    for name in kernels:
        body = asm[asm.index("\n%s:" % name):]
        body = body[:body.index("s_endpgm")]
        assert "global_atomic_add_x2" in body and "ds_add_u64" in body, name       # LDS first, then one add a cell
        assert "atomic_add_f" not in body and "cmpswap" not in body, name
        assert "v_div_fixup_f64" in body, name                                      # a division, not a reciprocal multiply
    positive = next(k for k in kernels if KERNELS[0] in k)
    body = asm[asm.index("\n%s:" % positive):]
    assert "global_atomic_or" in body[:body.index("s_endpgm")]


def test_the_library_exports_the_new_symbols():
    from goleft_amd import _hostlib, _lib
    nm = shutil.which("nm") or "/opt/rocm/lib/llvm/bin/llvm-nm"
    for so, names in ((_lib.SO_PATH, ("gd_cnveval", "gd_cnveval_timing")), (_hostlib.SO_PATH, ("gdh_cnveval_main", "gdh_cnveval_run"))):
        out = subprocess.check_output([nm, "-D", "--defined-only", so]).decode()
        exported = {ln.split()[2] for ln in out.splitlines() if len(ln.split()) == 3 and ln.split()[1] == "T"}
        for n in names:
            assert n in exported, (so, n)
    assert "gd_cnveval" in _lib.SYMBOLS and "gdh_cnveval_run" in _hostlib.SYMBOLS
