"""CPU: what dist adds to the libraries: the new entry points are exported and declared to ctypes,
the ABI numbers stay, the two kernels hold to their resources -- no scratch, no spills, workgroups of 256, one instance
each, the histogram kernel's LDS the 8192 uint32 bins DESIGN.md states plus its reduction slots, so that four workgroups
share a CU's 160 KiB --, and the Python methods have their signatures."""
import inspect
import shutil
import subprocess

import pytest

from tests import helpers as H


def test_the_libraries_export_the_new_symbols():
    from goleft_amd import _hostlib, _lib
    nm = shutil.which("nm") or "/opt/rocm/lib/llvm/bin/llvm-nm"
    for so, names in ((_lib.SO_PATH, ("gd_depth_hist", "gd_region_bins", "gd_dist_timing")),
                      (_hostlib.SO_PATH, ("gdh_dist_main", "gdh_dist_run"))):
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
def test_the_kernels_hold_to_their_resources():
    meta = H.kernel_metadata(H.api_asm())
    for name in ("gd_dh_hist_kernel", "gd_dh_region_bins_kernel"):
        hits = [k for k in meta if name in k]
        assert len(hits) == 1, (name, hits)
        r = meta[hits[0]]
        assert r["scratch"] == 0 and r["spill"] == 0 and r["sgpr_spill"] == 0 and r["wg"] == 256, (name, r)
    hist = meta[[k for k in meta if "gd_dh_hist_kernel" in k][0]]
    assert 8192 * 4 <= hist["lds"] <= 8192 * 4 + 128, hist               # the LDS range: 8192 bins of 4 bytes
    assert 4 * hist["lds"] <= 160 * 1024                                 # four workgroups a CU
    bins = meta[[k for k in meta if "gd_dh_region_bins_kernel" in k][0]]
    assert bins["lds"] <= 1024, bins                                     # 4 waves x 32 cuts


def test_the_python_entries_have_their_signatures():
    from goleft_amd import dist
    from goleft_amd.engine import DepthEngine
    p = inspect.signature(DepthEngine.depth_hist).parameters
    assert list(p) == ["self", "tids", "starts", "ends", "n_bins"]
    p = inspect.signature(DepthEngine.region_bins).parameters
    assert list(p) == ["self", "tids", "starts", "ends", "cuts"] and p["cuts"].default is None
    assert list(inspect.signature(DepthEngine.dist_timing).parameters) == ["self"]
    assert list(inspect.signature(dist.Main).parameters) == ["argv"]
