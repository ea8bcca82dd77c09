"""CPU: the indexer's kernels (goleft_amd/csrc/gd_bamguess.hpp, gd_bamdecode.hpp's IndexWalk, gd_baiindex.hpp) as hipcc
compiles them for gfx950.

The index walk runs beside the inflate kernel of the next range, whose six workgroups per CU leave 4 KB of LDS
(gd_bamdecode.hpp): a walk workgroup that needs more waits for an inflate workgroup to retire.  None of the new kernels
indexes anything by a runtime value in registers: no scratch, no spills."""
import shutil
import subprocess

import pytest

from tests import helpers as H

WALK_LDS = 4096
KERNELS = {"gd_bam_guess_kernel": 64, "gd_idx_walk_kernel": 64, "gd_idx_compact_kernel": 256, "gd_idx_tile_kernel": 256,
           "gd_idx_tscan_kernel": 256, "gd_idx_runs_kernel": 256, "gd_idx_linear_kernel": 256}

pytestmark = pytest.mark.skipif(H.HIPCC is None, reason="needs hipcc")


@pytest.fixture(scope="module")
def kernels():
    meta = H.kernel_metadata(H.api_asm())
    return {name: next(r for k, r in meta.items() if name in k) for name in KERNELS}


def test_the_kernels_exist_once_each_under_their_names():
    meta = H.kernel_metadata(H.api_asm())
    for name in KERNELS:
        assert sum(name in k for k in meta) == 1, name


def test_no_scratch_no_spills_and_the_launch_shapes(kernels):
    for name, r in kernels.items():
        assert r["scratch"] == 0 and r["spill"] == 0 and r["sgpr_spill"] == 0, (name, r)
        assert r["wg"] == KERNELS[name], (name, r)


def test_the_walk_stays_within_the_lds_the_inflate_kernel_leaves(kernels):
    assert 0 < kernels["gd_idx_walk_kernel"]["lds"] <= WALK_LDS, kernels["gd_idx_walk_kernel"]
    assert kernels["gd_bam_guess_kernel"]["lds"] == 0                            # (it runs beside the inflate kernel too)
    for name in ("gd_idx_tile_kernel", "gd_idx_tscan_kernel", "gd_idx_runs_kernel", "gd_idx_linear_kernel"):
        assert kernels[name]["lds"] <= WALK_LDS, (name, kernels[name])


def test_the_linear_index_is_a_64_bit_unsigned_minimum():
    asm = H.api_asm()
    name = next(k for k in H.kernel_metadata(asm) if "gd_idx_linear_kernel" in k)
    body = asm[asm.index("\n%s:" % name):]
    body = body[:body.index("s_endpgm")]
    assert "global_atomic_umin_x2" in body and "cmpswap" not in body


def test_the_libraries_export_the_new_symbols():
    from goleft_amd import _hostlib, _lib
    nm = shutil.which("nm") or "/opt/rocm/lib/llvm/bin/llvm-nm"
    for so, names in ((_lib.SO_PATH, ("gd_index_begin", "gd_index_decode", "gd_index_result", "gd_index_windows", "gd_index_timing")),
                      (_hostlib.SO_PATH, ("gdh_index_main", "gdh_index_run", "gdh_index_build", "gdh_index_free", "gdh_bai_assemble"))):
        out = subprocess.check_output([nm, "-D", "--defined-only", so]).decode()
        exported = {ln.split()[2] for ln in out.splitlines() if len(ln.split()) == 3 and ln.split()[1] == "T"}
        for n in names:
            assert n in exported, (so, n)
            assert n in (_lib.SYMBOLS if n.startswith("gd_") else _hostlib.SYMBOLS), n


def test_the_abi_numbers_stay():
    from goleft_amd import _lib
    lib = _lib.load()
    assert (lib.gd_abi_version(), lib.gd_abi_revision()) == (15, 3)
