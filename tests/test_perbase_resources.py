"""CPU: what perbase adds to the libraries: the new entry points are exported and declared to
ctypes, the ABI numbers stay, the three kernels hold to their resources -- no scratch, no spills, workgroups of 256, at
most two instances of count and of emit (without and with cuts), one scan --, and the Python method has its signature."""
import inspect
import shutil
import subprocess

import pytest

from tests import helpers as H


def test_the_libraries_export_the_new_symbols():
    from goleft_amd import _hostlib, _lib
    nm = shutil.which("nm") or "/opt/rocm/lib/llvm/bin/llvm-nm"
    for so, names in ((_lib.SO_PATH, ("gd_perbase_runs", "gd_perbase_runs_timing")),
                      (_hostlib.SO_PATH, ("gdh_perbase_main", "gdh_perbase_run"))):
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
def test_the_kernels_use_no_scratch_and_have_at_most_two_instances():
    meta = H.kernel_metadata(H.api_asm())
    for name, most in (("gd_pb_count_kernel", 2), ("gd_pb_emit_kernel", 2), ("gd_pb_scan_kernel", 1)):
        hits = [k for k in meta if name in k]
        assert 1 <= len(hits) <= most, (name, hits)
        if most == 2:
            assert len(hits) == 2, (name, hits)              # without cuts and with them
        for k in hits:
            r = meta[k]
            assert r["scratch"] == 0 and r["spill"] == 0 and r["sgpr_spill"] == 0 and r["wg"] == 256, (k, r)
    emit = [meta[k] for k in meta if "gd_pb_emit_kernel" in k]
    assert all(32768 <= r["lds"] <= 32768 + 64 for r in emit), emit      # the chunk's runs: 4096 of 8 bytes


def test_perbase_runs_has_its_signature():
    from goleft_amd import perbase
    from goleft_amd.engine import DepthEngine
    p = inspect.signature(DepthEngine.perbase_runs).parameters
    assert list(p) == ["self", "tid", "start", "end", "cuts"]
    assert p["start"].default == 0 and p["end"].default is None and p["cuts"].default is None
    assert list(inspect.signature(DepthEngine.perbase_runs_timing).parameters) == ["self"]
    q = inspect.signature(perbase.Main).parameters
    assert list(q) == ["argv", "out_path"] and q["out_path"].default is None
