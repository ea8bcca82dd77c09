"""CPU: the indexer's two readers of untrusted bytes -- the candidate test (goleft_amd/csrc/gd_bamguess.hpp) and
bam_walk<IndexWalk> (gd_bamdecode.hpp) -- in a stand-alone host program (tests/emul/idxwalk_asan_main.cpp) built with
-fsanitize=address,undefined and run directly, nothing preloaded: the kernels run lane by lane with the inflated stream,
the member tables, the slots and every per-segment table behind guard pages, over the fixture streams and over truncated
and byte-flipped copies.  No sanitizer finding, no read outside a buffer, and on intact streams the slots are what a
direct parse of the records says."""
import os
import shutil
import struct
import subprocess

import pytest

from oracle import bamio
from tests import helpers as H

REF = os.path.join(H.GOLDEN, "ref")
CLANG = next((p for p in ("/opt/rocm/lib/llvm/bin/clang++", shutil.which("clang++") or "") if p and os.path.exists(p)), None)

pytestmark = pytest.mark.skipif(CLANG is None, reason="the kernel source is compiled for the host with clang")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("idxwalk") / "idxwalk_asan")
    r = subprocess.run([CLANG, "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-std=c++17", "-o", exe,
                        os.path.join(H.ROOT, "tests", "emul", "idxwalk_asan_main.cpp"), "-lz"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.fixture(scope="module")
def t_head(tmp_path_factory):
    """The first 150 kb of t.bam's records as a BAM of its own (the whole stream is 19 MB: too long lane by lane)."""
    d = bamio.bgzf_decompress(open(os.path.join(REF, "t.bam"), "rb").read())
    l_text, = struct.unpack_from("<i", d, 4)
    p = 8 + l_text
    n_ref, = struct.unpack_from("<i", d, p)
    p += 4
    for _ in range(n_ref):
        p += 8 + struct.unpack_from("<i", d, p)[0]
    while p < 150000:
        p += 4 + struct.unpack_from("<i", d, p)[0]
    path = str(tmp_path_factory.mktemp("thead") / "t_head.bam")
    open(path, "wb").write(bamio.bgzf_compress(d[:p], block=20000))
    return path


def run(program, args):
    return subprocess.run([program] + args, capture_output=True, text=True, timeout=600)


def test_intact_fixture_streams(program, t_head):
    r = run(program, [os.path.join(REF, "hla.bam"), os.path.join(REF, "t-empty.bam"), t_head])
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    lines = r.stdout.splitlines()
    assert lines[-1] == "ok" and len(lines) == 4
    assert " records 482 " in lines[0] and " records 0 " in lines[1]
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr


def test_truncated_and_byte_flipped_copies(program):
    r = run(program, ["--fuzz", "24", os.path.join(REF, "hla.bam")])
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    assert r.stdout.splitlines()[-1] == "ok"
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr
