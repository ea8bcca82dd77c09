"""CPU: the four owners of goleft_amd/csrc/gd_own.hpp (device array, page-locked array, event, stream) under
AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone program that is its own HIP runtime
(tests/emul/own_asan_main.cpp: the allocation, free, create and destroy functions over malloc, counted per kind).  What
it holds them to: construction and destruction, moves that free nothing, a move-assignment that frees exactly the old
block, an idempotent reset, release, borrowed blocks and handles that are never given back, a failed allocation that
leaves the owner empty, a count of 0 that is one element, and at the end nothing alive and nothing freed twice."""
import os
import shutil
import subprocess

import pytest

from tests import helpers as H

GXX = shutil.which("g++")
CSRC = os.path.join(H.ROOT, "goleft_amd", "csrc")


def hip_include():
    """The directory of hip/hip_runtime_api.h: beside the compiler the library is built with."""
    roots = [os.path.dirname(os.path.dirname(os.path.realpath(H.HIPCC)))] if H.HIPCC else []
    roots += [os.environ.get("ROCM_PATH", ""), "/opt/rocm"]
    for r in roots:
        if r and os.path.exists(os.path.join(r, "include", "hip", "hip_runtime_api.h")):
            return os.path.join(r, "include")
    return None


@pytest.fixture(scope="module")
def asan_owners(tmp_path_factory):
    inc = hip_include()
    if GXX is None or inc is None:
        pytest.skip("no g++ or no HIP headers")
    exe = str(tmp_path_factory.mktemp("asan") / "own_asan")
    r = subprocess.run([GXX, "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-std=c++17",
                        "-D__HIP_PLATFORM_AMD__", "-I", inc, "-I", CSRC, "-o", exe,
                        os.path.join(H.ROOT, "tests", "emul", "own_asan_main.cpp")], capture_output=True, text=True)
    if r.returncode != 0 and "gd_own.hpp" not in r.stderr and "own_asan_main.cpp" not in r.stderr:
        pytest.skip("this toolchain has no sanitizer run time: " + r.stderr[-300:])
    assert r.returncode == 0, r.stderr[-3000:]             # (an error in the header or the program is a failure, not a skip)
    return exe


def test_owners_free_what_they_own_once(asan_owners):
    r = subprocess.run([asan_owners], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.stdout[-2000:], r.stderr[-3000:])


def test_owners_header_needs_only_the_runtime_api():
    """gd_own.hpp knows neither the context nor the ABI's error reporting: it stays compilable on the host alone."""
    text = open(os.path.join(CSRC, "gd_own.hpp")).read()
    code = "\n".join(line.split("//")[0] for line in text.splitlines())
    for word in ("gd_ctx", "HIPCHK", "fail(", "goleft_depth.h", "hip_runtime.h"):
        assert word not in code, word
