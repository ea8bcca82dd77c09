"""CPU: what the .csi indexer adds to the libraries: the new entry points are exported and declared to
ctypes, the binning scheme travels in the kernels' jobs as run-time values -- tests/test_index_resources.py holds the seven
kernels to one instance each, no scratch, no spills --, and the ABI numbers stay."""
import shutil
import subprocess

import pytest

from tests import helpers as H


def test_the_libraries_export_the_new_symbols():
    from goleft_amd import _hostlib, _lib
    nm = shutil.which("nm") or "/opt/rocm/lib/llvm/bin/llvm-nm"
    for so, names in ((_lib.SO_PATH, ("gd_index_begin_csi", "gd_index_begin")),
                      (_hostlib.SO_PATH, ("gdh_csi_assemble", "gdh_index_build_csi", "gdh_csi_read", "gdh_bai_assemble", "gdh_index_build"))):
        out = subprocess.check_output([nm, "-D", "--defined-only", so]).decode()
        exported = {ln.split()[2] for ln in out.splitlines() if len(ln.split()) == 3 and ln.split()[1] == "T"}
        for n in names:
            assert n in exported, (so, n)
            assert n in (_lib.SYMBOLS if n.startswith("gd_") else _hostlib.SYMBOLS), n


def test_the_abi_numbers_stay():
    from goleft_amd import _lib
    lib = _lib.load()
    assert (lib.gd_abi_version(), lib.gd_abi_revision()) == (15, 3)


@pytest.mark.skipif(H.HIPCC is None, reason="needs hipcc")
def test_the_geometry_is_a_run_time_value_of_one_walk_and_one_linear_kernel():
    meta = H.kernel_metadata(H.api_asm())
    for name in ("gd_idx_walk_kernel", "gd_idx_linear_kernel"):
        hits = [k for k in meta if "gd_idx" in k and name[len("gd_idx"):-len("_kernel")] in k]
        assert len(hits) == 1, (name, hits)
        r = meta[hits[0]]
        assert r["scratch"] == 0 and r["spill"] == 0 and r["sgpr_spill"] == 0, (name, r)


def test_python_entry_points_take_the_format():
    import inspect
    from goleft_amd import index
    for fn in (index.build, index.build_stats, index.write):
        p = inspect.signature(fn).parameters
        assert p["csi"].default is False and p["min_shift"].default == 14, fn
